"""CPU: what tests/test_gpu_output_geometry.py rests on (cases, data, metrics: output_geometry_cases.py).

  * pin: classifier_fp64, the plain restatement every device figure is taken against, equals mo.output_classifier (logits and every
    gradient, 1e-12) on three cases, one of them in training;
  * fairness: the same restatement in fp32 stays within a third of every bound on every case and mode of the table;
  * table: every row takes the path it names under the restated launch rules, the issue's rows are all there, and the rules' C++ text
    still reads as restated (an edit that retires an edge fails here);
  * sizes: macx_output_saved_floats / _ws_floats equal the layout of include/macx.h for every row and return 0 for what out_check
    refuses."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import mac_oracle as mo
import output_geometry_cases as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-network_amd", "csrc")

_DATA = {}         # one case's data and fp64 references at a time


def data(macx, c):
    if _DATA.get("id") != c.id:
        _DATA.clear()
        _DATA.update(id=c.id, data=og.make_case(macx, mo, c))
        for train in c.modes:
            _DATA[train] = og.reference(c, *_DATA["data"], train)
    return _DATA


# ---- pin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid, train", [("B5-d64-h48-A17", True), ("B65-d64-h32-A33", False), ("B5-d64-h48-A17-word", True)])
def test_restatement_is_the_oracles_classifier(macx, cid, train):
    c = og.BY_ID[cid]
    cfg, out, mem, vq, answers = og.make_case(macx, mo, c)
    mine = og.reference(c, cfg, out, mem, vq, answers, train)
    prm = {k: v.detach().double().clone().requires_grad_(True) for k, v in out.to_reference_dict().items()}
    vs = mo.VarStore(params=prm, dtype=torch.float64)
    m, v = mem.double().requires_grad_(True), vq.double().requires_grad_(True)
    keep = float(out.keep) if train else 1.0
    assert (keep < 1.0) == train
    ref = mo.output_classifier(cfg, vs, m, v, output_keep=keep, masks=og.masks_for(c, keep, torch.float64) if train else None)
    (ref * mine["dl"].double()).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(mine["logits"], ref.detach())
    assert close(mine["d_memory"], m.grad) and close(mine["d_vecQ"], v.grad)
    for f, name in macx.output.REF_NAMES.items():
        assert close(mine[f], prm[name].grad), f
    assert float(mine["dl"].abs().max()) > 0 and all(float(s.min()) >= 0 for s in mine["sum_abs"].values())


# ---- fairness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", og.CASES, ids=lambda c: c.id)
def test_fp32_restatement_is_within_a_third_of_every_bound(macx, case):
    ref = data(macx, case)
    tol = og.tolerances()
    bad = []
    for train in case.modes:
        got = og.reference(case, *ref["data"], train, dtype=torch.float32, dl=ref[train]["dl"])
        e = og.errors(got, ref[train])
        og.log(og.line(case, "fp32", train, e))
        for k in og.METRICS:
            if not e[k] <= og.FAIR * tol[k]:
                bad.append("%s %.3e > %.1e / 3 (%s): %s" % (k, e[k], tol[k], "train" if train else "keep1", e["where"]))
    assert not bad, "\n".join(bad)


def test_the_data_is_what_the_table_says(macx):
    """biases non-zero, the softmax peaked, per-answer gradient scales orders of magnitude apart, A = 1's loss gradient exactly zero"""
    c = og.BY_ID["B65-d64-h48-A1845"]
    ref = data(macx, c)
    cfg, out, mem, vq, answers = ref["data"]
    assert all(float(getattr(out, f).detach().abs().min()) > 0 for f in ("outQuestion_b", "fc0_b", "fc1_b"))
    p = torch.softmax(ref[True]["logits"], dim=-1)
    assert float(p.amax(dim=1).median()) > 20.0 / c.A
    cols = ref[True]["fc1_W"].abs().amax(dim=0)
    assert float(cols.max() / cols.min()) > 1e3, "per-answer gradient scales"
    assert float(ref[True]["dl"].sum(dim=1).abs().max()) < 1e-6                    # (softmax - onehot) / B sums to zero per question
    one = og.BY_ID["B5-d64-h48-A1"]
    assert one.cot == "randn"
    lg = torch.randn(5, 1, dtype=torch.float64)
    ce = torch.softmax(lg, dim=-1)
    ce[:, 0] -= 1.0
    assert float(ce.abs().max()) == 0.0


# ---- table ----------------------------------------------------------------------------------------------------------------
def test_table_holds_the_issue_cases():
    have = {(c.B, c.d, c.H, c.A, c.b0, c.keep1, c.word != 0) for c in og.CASES}
    want = [(5, 64, 48, A, 4, False, False) for A in (1, 15, 16, 17, 1848)]
    want += [(65, 64, 48, 1845, 4, True, False), (64, 512, 512, 3129, 4, False, False)]
    want += [(B, 64, 32, 33, 4, B in (65, 129), False) for B in (1, 16, 17, 64, 65, 128, 129, 192, 193, 256)]
    want += [(3, 16, 16, 28, 4, True, False), (3, 1024, 1024, 28, 4, False, False), (3, 512, 16, 28, 4, False, False)]
    want += [(128, 512, 512, 1845, 4, True, False)]
    want += [(5, 64, 48, 17, (1 << 25) - 2, False, False), (5, 64, 48, 17, (1 << 24) - 2, False, False)]
    for w in want:
        assert w in have, w
    assert any(c.word != 0 for c in og.CASES)
    assert [c.id for c in og.CASES if c.cot == "randn"] == ["B5-d64-h48-A1"]


@pytest.mark.parametrize("case", og.CASES, ids=lambda c: c.id)
def test_case_takes_the_path_its_row_names(case):
    r = og.route(case)
    assert case.expect, case.id
    for k, v in case.expect.items():
        assert r[k] == v, (case.id, k, r[k], v)


def test_the_edges_the_table_was_chosen_for():
    routes = {c.id: og.route(c) for c in og.CASES}
    # before this table no test had B A > 2112: every case marked second_pass is new ground for crop_cols / add_bias / pad_cols
    assert sum(1 for r in routes.values() if r["second_pass"]) >= 5 and max(r["outer1_passes"] for r in routes.values()) == 98
    # both tile forms, the ragged last tile of one row in each, and rowsum's loop at 0, 1 and 2 iterations with and without the tail row
    assert {(r["tile"], r["last_tile_rows"]) for r in routes.values()} >= {(16, 1), (16, 16), (64, 1), (64, 64)}
    assert {(r["rowsum_iters"], r["rowsum_tail"]) for r in routes.values()} >= {(0, True), (1, False), (1, True), (2, False)}
    assert {r["rowsum_s1"] for r in routes.values()} >= {0, 1, 64}
    # the transposed pack: scalar and 16-byte path, each with and without a zero tail
    assert {(r["vec4"], r["zero_tail"] > 0) for r in routes.values()} == {(False, False), (False, True), (True, False), (True, True)}
    assert og.t_pack(1848) == (True, 2, 0) and og.t_pack(28) == (True, 1, 0) and og.t_pack(1845) == (False, 2, 1)
    assert {r["k_passes"] for r in routes.values()} >= {1, 2, 4} and {r["idle_waves"] for r in routes.values()} >= {0, 1, 3}
    # the wrap: inside the batch for layer 0 only; mask_for wraps with the kernel
    from oracle import dropout_hash as dh
    import numpy as np
    c = og.BY_ID["B5-d64-h48-A17-wrap"]
    m = dh.mask_for(og.SEED, 7, 0, 0.85, (c.B, 128), b0=c.b0)
    assert np.array_equal(m[2:], dh.mask_for(og.SEED, 7, 0, 0.85, (3, 128), b0=0)) and not np.array_equal(m[:2], m[2:4])
    assert not np.array_equal(m, dh.mask_for(og.SEED, 7, 0, 0.85, (c.B, 128), b0=c.b0, word=og.WORD))


def test_the_rules_read_as_restated():
    """the C++ text behind tile_rows, pad16, the vec4 condition, the grids and rowsum's loop"""
    api = open(os.path.join(CSRC, "macx_api.hip")).read()
    small = open(os.path.join(CSRC, "macx_small.hip.h")).read()
    flat = lambda s: re.sub(r"\s+", " ", s)
    api, small = flat(api), flat(small)
    assert "inline int pad16(int n) { return (n + 15) & ~15; }" in api
    assert "if (p.rows <= 128) { hipLaunchKernelGGL(small_linear_kernel<1>, dim3(p.n_out / 16, (p.rows + 15) / 16, nz)" in small
    assert "hipLaunchKernelGGL(small_linear_kernel<4>, dim3(p.n_out / 16, (p.rows + 63) / 64, nz)" in small
    assert "const bool vec4 = q.ld_k == 1 && (q.ld_j & 3) == 0 &&" in small and "if (vec4 && k0 + 4 <= q.k_src)" in small
    for kernel, grid in (("crop_cols_kernel", 16), ("add_bias_kernel", 16), ("pad_cols_kernel", 16)):
        assert "hipLaunchKernelGGL(%s, dim3(%d), dim3(256), 0, st" % (kernel, grid) in api, kernel
    assert "hipLaunchKernelGGL(outer_sum_kernel, dim3(64), dim3(256), 0, st, saved + L.x1, H, d_logits, A, B, H, A, G->fc1_W)" in api
    assert "pk.add(P->fc1_W, A, 1, H, Ap, saved + L.w1_p, H, A);" in api and "pk.add(P->fc1_W, 1, A, Ap, H, ws + W.w1T, A, H);" in api
    assert "for (; r + 64 < rows; r += 128) { s0 += src[(size_t)r * ld + i]; s1 += src[(size_t)(r + 64) * ld + i]; }" in small
    assert "const uint32_t idx = (row0 + (uint32_t)r) * (uint32_t)dl + (uint32_t)j;" in small
    assert "s->d < 16 || s->d % 16 || s->hidden < 16 || s->hidden % 16 || s->answers < 1" in api


# ---- sizes ----------------------------------------------------------------------------------------------------------------
def test_size_calls_equal_the_restated_layout(macx):
    L = macx._lib.lib()
    sh = lambda B, d, H, A, b0=0: C.byref(macx._lib.MacxOutShapes(B=B, d=d, hidden=H, answers=A, b0=b0))
    for c in og.CASES:
        assert L.macx_output_saved_floats(sh(c.B, c.d, c.H, c.A, c.b0 & 0x7FFFFFFF)) == og.saved_floats(c.B, c.d, c.H, c.A), c.id
        assert L.macx_output_ws_floats(sh(c.B, c.d, c.H, c.A, c.b0 & 0x7FFFFFFF)) == og.ws_floats(c.B, c.d, c.H, c.A), c.id
    for bad in ((5, 24, 48, 17), (5, 64, 8, 17), (5, 64, 48, 0), (0, 64, 48, 17)):
        assert L.macx_output_saved_floats(sh(*bad)) == 0 and L.macx_output_ws_floats(sh(*bad)) == 0, bad
