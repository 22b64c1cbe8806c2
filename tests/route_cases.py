"""The option sets and shapes over which the fused cell's buffer layouts and launch routes are pinned: shared by
tests/golden/make_route_layouts.py (which records the layouts of the checkout it runs from), tests/test_route_host.py (no GPU) and
tests/test_gpu_cell_geometry.py.  No GPU is touched here: the sizing exports and macx_cell_route answer on the host.

A shape is (B, S, N, d, p, d_logical)."""
import ctypes as C

FLAG_FILES = ("args", "args1", "args2", "args3", "args4")
FAMILIES = ("h2", "split", "native")
# the macx_opts.tune keys that reach a layout (None: the shipped table)
TUNES = (None, {"chain": 0}, {"sb_defer": 0}, {"sb_wide": 0}, {"native_waves": 4}, {"row_tiles": 2})
NCU = 256                 # compute units of the chip the geometry table below was observed on

# The cases of tests/test_gpu_cell_geometry.py and the route each takes on NCU compute units, default family and tuning table:
# flag file, B, S, N, d, p, train | chain (0: one launch per product), rows per tile, tiles, S_b route (step | deferred: the 128 x 128
# kernel | wide: the 128 x 256 one), kw = jw of the deferred weight-gradient contractions, fillers of chain_fwd, fillers of chain_bwd
GEOMETRY = [
    ("args", 3, 7, 49, 384, 2, True, 1, 64, 3, "deferred", 1, 0, 0),
    ("args1", 2, 5, 100, 384, 3, True, 1, 64, 4, "deferred", 1, 0, 0),
    ("args4", 3, 6, 20, 384, 2, False, 1, 64, 1, "step", 1, 0, 0),
    ("args", 2, 5, 209, 384, 2, True, 1, 64, 7, "deferred", 1, 0, 0),
    ("args", 3, 6, 49, 320, 2, True, 1, 64, 3, "deferred", 1, 0, 0),        # 320 runs zero-padded to 384 (d_logical = 320)
    ("args", 2, 5, 49, 640, 2, True, 0, 0, 0, "step", 1, 0, 0),
    ("args3", 2, 5, 33, 768, 2, True, 0, 0, 0, "step", 2, 0, 0),
    ("args", 1, 4, 16, 896, 1, False, 0, 0, 0, "step", 1, 0, 0),
    ("args", 21, 5, 196, 512, 2, True, 1, 32, 129, "wide", 2, 127, 0),
    ("args", 42, 5, 196, 512, 2, True, 1, 64, 129, "wide", 2, 127, 127),
    ("args", 16, 4, 256, 512, 1, True, 1, 16, 256, "wide", 2, 64, 0),
    ("args", 32, 4, 256, 512, 1, True, 1, 32, 256, "wide", 2, 0, 0),
    ("args", 17, 4, 241, 512, 1, True, 1, 32, 129, "wide", 2, 127, 0),
    ("args", 33, 4, 249, 512, 1, False, 1, 64, 129, "wide", 2, 127, 0),
    ("args", 3, 9, 196, 512, 2, False, 1, 16, 37, "wide", 2, 64, 0),
    ("args1", 5, 7, 49, 512, 3, False, 1, 16, 16, "wide", 2, 64, 0),
    ("args", 9, 5, 17, 256, 2, True, 1, 64, 3, "step", 2, 0, 0),
    ("args", 9, 5, 16, 256, 2, True, 1, 64, 3, "step", 2, 0, 0),
    ("args", 9, 5, 31, 256, 3, True, 1, 64, 5, "step", 2, 0, 0),
    ("args", 9, 5, 32, 256, 3, True, 1, 64, 5, "wide", 2, 0, 0),
    ("args1", 7, 5, 21, 128, 2, False, 1, 64, 3, "step", 1, 0, 0),
    ("args", 5, 4, 15, 256, 2, True, 0, 0, 0, "step", 2, 0, 0),
]


def padded(d):
    """(kernel width, d_logical) of a cell of logical width d: PaddedMACCell's rule"""
    dk = (d + 127) // 128 * 128
    return dk, (d if dk != d else 0)


def layout_shapes():
    """the shapes of the layout grid, in a fixed order"""
    import gradient_scale_cases as gsc
    out = []
    for row in GEOMETRY:
        dk, dlog = padded(row[4])
        out.append((row[1], row[2], row[3], dk, row[5], dlog))
    out += [(gsc.B, S, N, d, p, 0) for _, S, N, d, p in gsc.SHAPES.values()]
    out += [(4, 6, 49, d, 2, 0) for d in range(128, 1025, 128)]
    out += [(5, 6, N, 512, 2, 0) for N in (15, 16, 31, 32, 63, 64)]
    out += [(B, 5, 196, 512, 2, 0) for B in (128, 129)]
    out.append((64, 8, 196, 512, 12, 0))          # the benchmark's cell
    return list(dict.fromkeys(out))


def tune_id(tune):
    return "default" if not tune else ",".join("%s=%d" % kv for kv in sorted(tune.items()))


def frozen(macx, flags, shape, family, tune=None):
    """(MacxOpts, MacxShapes) of a flag file at a shape"""
    from oracle import mac_oracle as mo
    B, S, N, d, p, dlog = shape
    cfg = mo.flag_file_config(flags, netLength=p, memDim=d, ctrlDim=d, attDim=d)
    return macx.options.freeze(cfg, gemm=family, tune=tune), macx._lib.MacxShapes(B=B, S=S, N=N, d=d, p=p, b0=0, d_logical=dlog)


def dropout(macx, memory=1.0, read=1.0, write=1.0):
    return macx._lib.MacxDropout(keep_memory=memory, keep_read=read, keep_write=write, seed=7, mask_word=None)


def route(macx, opts, shapes, drop=None, keep=1, ncu=NCU):
    """macx_cell_route's answer as {field: value}; ncu = 0: for the current device, as a launch plans"""
    out = macx._lib.MacxRoute()
    macx._lib.check(macx._lib.lib().macx_cell_route(C.byref(opts), C.byref(shapes), C.byref(drop) if drop is not None else None, keep, ncu,
                                                    C.byref(out)), "macx_cell_route")
    return {f: getattr(out, f) for f, _ in out._fields_}


def describe(r):
    """a route in the words of the geometry table"""
    if not r["chain"]:
        return "per-product launches (family %d), wgrad kw=jw=%d" % (r["family"], r["wgrad_kw"])
    sb = ("deferred S_b, %s" % ("128x256" if r["sb_wide"] else "128x128")) if r["sb_deferred"] else "S_b per step"
    return ("chain, %d-row tiles x %d, %s, wgrad kw=jw=%d, fwd fillers %d, dKB fillers %d"
            % (r["tile_rows"], r["tiles"], sb, r["wgrad_kw"], r["fwd_fillers"], r["dkb_fillers"]))


def layout(macx, opts, shapes, keep):
    """what the sizing exports say: [saved floats, backward workspace floats, (offset, count) or the error code of every segment]"""
    L = macx._lib.lib()
    o, s = C.byref(opts), C.byref(shapes)
    out = [int(L.macx_saved_floats(o, s, keep)), int(L.macx_ws_floats(o, s, 1))]
    for seg in range(len(macx._lib.SEG)):
        off, cnt = C.c_size_t(0), C.c_size_t(0)
        rc = L.macx_saved_segment(o, s, keep, seg, C.byref(off), C.byref(cnt))
        out.append([int(off.value), int(cnt.value)] if rc == 0 else int(rc))
    return out
