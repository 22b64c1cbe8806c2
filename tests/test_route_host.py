"""CPU: the fused cell's route plan (macx_cell_route: the plan every launch of the cell follows) and the buffer layouts sized from it.

  * the layouts -- macx_saved_floats, macx_ws_floats(.., 1) and every MACX_SEG_* segment -- over flag file x kernel family x keep x
    tuning key x shape equal the integers recorded from the parent of the change that introduced the plan
    (tests/golden/route_layouts.json, tests/golden/make_route_layouts.py);
  * no field a layout reads moves with the compute-unit count or the dropout;
  * on 256 compute units every case of tests/test_gpu_cell_geometry.py takes the route its table names (tests/route_cases.py), the
    shapes of tests/gradient_scale_cases.py the routes they were chosen for, and the tuning keys and options that switch a route
    off do so."""
import ctypes as C
import json
import os

import pytest
import torch

import gradient_scale_cases as gsc
import route_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_layouts.json")
FILLER_FIELDS = ("fwd_fillers", "fill_y", "fill_stage0", "fill_write", "dkb_jobs", "dkb_fillers", "dkb_skip")
BIG = (42, 5, 196, 512, 2, 0)           # 129 64-row tiles on 256 compute units: forward and dKB fillers both active


from route_cases import dropout, route


def plan(macx, flags="args", shape=BIG, family="h2", tune=None, **kw):
    opts, shapes = rc.frozen(macx, flags, shape, family, tune)
    return route(macx, opts, shapes, **kw)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("flags", rc.FLAG_FILES)
def test_layouts_equal_the_recorded_ones(macx, golden, flags):
    shapes = rc.layout_shapes()
    assert [list(s) for s in shapes] == golden["shapes"]
    seen = 0
    for family in rc.FAMILIES:
        for tune in rc.TUNES:
            for keep in (0, 1):
                rows = golden["points"]["%s|%s|%d|%s" % (flags, family, keep, rc.tune_id(tune))]
                for k, shape in enumerate(shapes):
                    opts, sh = rc.frozen(macx, flags, shape, family, tune)
                    saved, ws, status = rows[k]
                    head = golden["heads"][flags][k] if isinstance(status, list) else [status] * (len(macx._lib.SEG) - 1)
                    assert rc.layout(macx, opts, sh, keep) == [saved, ws] + head + [status], (flags, family, rc.tune_id(tune), keep, shape)
                    seen += 1
    assert seen == len(rc.FAMILIES) * len(rc.TUNES) * 2 * len(shapes)


@pytest.mark.parametrize("family", rc.FAMILIES)
def test_layout_fields_move_with_neither_compute_units_nor_dropout(macx, family):
    drops = (None, dropout(macx), dropout(macx, 0.9, 0.85, 0.8))
    for flags in rc.FLAG_FILES:
        for tune in rc.TUNES:
            for shape in rc.layout_shapes():
                if shape[5] and family != "h2":
                    continue                              # (refused by macx_check: a d_logical cell off the H2 family)
                opts, sh = rc.frozen(macx, flags, shape, family, tune)
                plans = [route(macx, opts, sh, drop=dp, keep=keep, ncu=ncu) for dp in drops for keep in (0, 1) for ncu in (0, 64, 256, 304)]
                layout = [{f: v for f, v in r.items() if f not in FILLER_FIELDS} for r in plans]
                assert all(l == layout[0] for l in layout), (flags, family, rc.tune_id(tune), shape)


@pytest.mark.parametrize("row", rc.GEOMETRY, ids=["%s-B%d-N%d-d%d-p%d" % (r[0], r[1], r[3], r[4], r[5]) for r in rc.GEOMETRY])
def test_geometry_cases_take_the_routes_of_their_table(macx, row):
    flags, B, S, N, d, p, train, chain, rows, tiles, sb, kw, fwd_fill, dkb_fill = row
    dk, dlog = rc.padded(d)
    opts, sh = rc.frozen(macx, flags, (B, S, N, dk, p, dlog), "h2")
    from oracle import mac_oracle as mo
    cfg = mo.flag_file_config(flags)
    dp = dropout(macx, cfg.memoryDropout, cfg.readDropout, cfg.writeDropout) if train else None
    r = route(macx, opts, sh, drop=dp, keep=1, ncu=rc.NCU)
    assert r["family"] == 2
    assert (r["chain"], r["tile_rows"], r["tiles"]) == (chain, rows, tiles)
    assert (r["sb_deferred"], r["sb_wide"]) == {"step": (0, 0), "deferred": (1, 0), "wide": (1, 1)}[sb]
    assert r["wgrad_kw"] == kw
    assert (r["fwd_fillers"], r["dkb_fillers"]) == (fwd_fill, dkb_fill)
    assert r["fill_y"] == int(fwd_fill > 0) and (r["dkb_jobs"] > 0) == (dkb_fill > 0)


def test_gradient_scale_shapes_select_their_routes(macx):
    got = {}
    for name, (flags, S, N, d, p) in gsc.SHAPES.items():
        opts, sh = rc.frozen(macx, flags, (gsc.B, S, N, d, p, 0), "h2")
        got[name] = (route(macx, opts, sh), opts)
    r, _ = got["launch"]                 # the narrowest chain kernel, 64-row tiles, the deferred S_b contraction on its 128 x 128 kernel
    assert (r["chain"], r["tile_rows"], r["tiles"], r["sb_deferred"], r["sb_wide"], r["wgrad_kw"]) == (1, 64, 4, 1, 0, 1)
    r, _ = got["step_sb"]                # N < 32: S_b once per step, no per-tile sums
    assert (r["chain"], r["chain_sums"], r["sb_deferred"]) == (1, 0, 0)
    r, _ = got["nochain"]                # N < 16: one launch per product
    assert (r["chain"], r["tile_rows"], r["tiles"], r["sb_deferred"]) == (0, 0, 0, 0)
    r, _ = got["chain"]                  # d = 512 on 16-row tiles, the wide S_b kernel
    assert (r["chain"], r["tile_rows"], r["tiles"], r["sb_deferred"], r["sb_wide"]) == (1, 16, 49, 1, 1)
    r, o = got["selfatt"]                # self-attention: the write unit is several launches
    assert o.write_self_att == 1 and r["chain"] == 1 and r["fill_write"] == 0
    for name in ("launch", "chain"):     # the other two families run neither chain kernels nor deferred contractions
        for family, code in (("split", 1), ("native", 0)):
            flags, S, N, d, p = gsc.SHAPES[name]
            r = plan(macx, flags, (gsc.B, S, N, d, p, 0), family)
            assert (r["family"], r["chain"], r["chain_sums"], r["sb_deferred"], r["sb_wide"], r["fwd_fillers"], r["dkb_jobs"]) == (code, 0, 0, 0, 0, 0, 0)


def test_tuning_keys_switch_routes_off(macx):
    base = plan(macx)
    assert (base["chain"], base["tile_rows"], base["tiles"], base["sb_deferred"], base["sb_wide"]) == (1, 64, 129, 1, 1)
    assert (base["fwd_fillers"], base["fill_y"], base["fill_write"], base["dkb_jobs"], base["dkb_fillers"]) == (127, 1, 1, 3, 127)
    assert base["dkb_skip"] == 0 and base["dy_in_linear"] == 1 and base["dc_reduce_per_step"] == 0
    r = plan(macx, tune={"chain": 0})
    assert [r[f] for f in ("chain", "tile_rows", "tiles", "chain_sums", "sb_deferred", "sb_wide", "dy_in_linear", "dc_reduce_per_step")] == [0] * 8
    assert [r[f] for f in FILLER_FIELDS] == [0] * len(FILLER_FIELDS)
    r = plan(macx, tune={"sb_defer": 0})
    assert (r["chain"], r["chain_sums"], r["sb_deferred"], r["sb_wide"], r["dy_in_linear"], r["dc_reduce_per_step"]) == (1, 1, 0, 0, 0, 0)
    assert r["sb_slabs"] == 2 * r["sb_groups"] and base["sb_slabs"] == base["sb_groups"]          # p = 2: per step | one launch
    r = plan(macx, tune={"sb_wide": 0})
    assert (r["sb_deferred"], r["sb_wide"]) == (1, 0)
    r = plan(macx, tune={"pre_fill": 0})
    assert (r["fwd_fillers"], r["fill_y"], r["fill_stage0"], r["fill_write"]) == (0, 0, 0, 0) and r["dkb_fillers"] == 127
    r = plan(macx, tune={"pre_fill": 2})
    assert (r["fwd_fillers"], r["fill_y"], r["fill_write"]) == (127, 1, 0)
    r = plan(macx, tune={"dkb_fill": 0})
    assert (r["dkb_jobs"], r["dkb_fillers"], r["dkb_skip"]) == (0, 0, 0) and r["fwd_fillers"] == 127
    # more than 128 questions: the dy linear's PART form and the fillers' linear tiles do not reach that far
    r = plan(macx, shape=(129, 5, 196, 512, 2, 0))
    assert (r["dy_in_linear"], r["dc_reduce_per_step"], r["fwd_fillers"]) == (0, 1, 0)


def test_options_and_dropout_limit_what_the_fillers_take_over(macx):
    assert plan(macx)["fill_write"] == 1 and plan(macx, drop=dropout(macx))["fill_write"] == 1
    assert plan(macx, "args4")["fill_write"] == 0 and plan(macx, "args4")["fill_y"] == 1             # a gate
    assert plan(macx, "args3")["fill_write"] == 0                                                    # self-attention (and a gate)
    assert plan(macx, "args1")["fill_write"] == 0                                                    # recurrent control
    assert plan(macx, drop=dropout(macx, write=0.9))["fill_write"] == 0                              # write dropout
    for flags, field in (("args4", "write_gate"), ("args3", "write_self_att"), ("args1", "control_feed_prev")):
        assert getattr(rc.frozen(macx, flags, BIG, "h2")[0], field) == 1
    # stage 0 of the next step is prefetched only where it is a stage: read dropout, in a run that keeps its activations
    assert plan(macx, drop=dropout(macx, read=0.85), keep=1)["fill_stage0"] == 1
    assert plan(macx, drop=dropout(macx, read=0.85), keep=0)["fill_stage0"] == 0
    assert plan(macx, drop=dropout(macx, read=1.0), keep=1)["fill_stage0"] == 0
    assert plan(macx, drop=None, keep=1)["fill_stage0"] == 0


def test_no_device_means_no_fillers(macx):
    """ncu = 0 asks the current device, as a launch does: without one nothing rides on idle compute units"""
    r = plan(macx, ncu=0)
    if torch.cuda.is_available():
        assert r == plan(macx, ncu=torch.cuda.get_device_properties(0).multi_processor_count)
    else:
        assert [r[f] for f in FILLER_FIELDS] == [0] * len(FILLER_FIELDS)
    assert {f: v for f, v in r.items() if f not in FILLER_FIELDS} == {f: v for f, v in plan(macx).items() if f not in FILLER_FIELDS}


def test_a_refused_option_set_is_refused_as_macx_check_refuses_it(macx):
    L = macx._lib.lib()
    out = macx._lib.MacxRoute()
    opts, sh = rc.frozen(macx, "args", (3, 6, 49, 384, 2, 320), "native")          # a d_logical cell off the H2 family
    assert L.macx_cell_route(C.byref(opts), C.byref(sh), None, 1, rc.NCU, C.byref(out)) == L.macx_check(C.byref(opts), C.byref(sh)) == macx._lib.MACX_EUNSUPPORTED
    opts, sh = rc.frozen(macx, "args", (3, 6, 49, 200, 2, 0), "h2")                # a width that is no multiple of 128
    assert L.macx_cell_route(C.byref(opts), C.byref(sh), None, 1, rc.NCU, C.byref(out)) == L.macx_check(C.byref(opts), C.byref(sh)) == macx._lib.MACX_EINVAL
    opts, sh = rc.frozen(macx, "args", BIG, "h2")
    assert L.macx_cell_route(C.byref(opts), C.byref(sh), None, 1, rc.NCU, None) == macx._lib.MACX_EINVAL
