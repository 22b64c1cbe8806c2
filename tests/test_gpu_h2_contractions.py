"""-m gpu: the H2 row contractions on their own -- wgrad_h2_kernel (+ wgrad_h2_factors_kernel), sb_h2_kernel, sb_h2w_kernel of
mac-network_amd/csrc/macx_wgrad_h2.hip.h through macx_h2_wgrad / macx_h2_sb -- against the fp64 product of the operands the kernels
multiply, EVERY ELEMENT within the derived bound of tests/h2_contraction_cases.py (tables, data, reference, bounds and their
derivation; tests/test_h2_contractions_host.py holds the tables to their paths and shows the bounds fair and sharp on the CPU).

One test function per kernel.  Every case:
  * the operands are converted by macx_h2_from_f32 into buffers pre-filled with 0xFF bytes (fp16 NaN in every pad row and every byte
    the producer leaves untouched, as a torch.empty `saved` / `ws` may hold); macx_h2_to_f32 gives back the CPU restatement of the
    format bit for bit; the results are finite, meet the bounds, and are bit-equal to a run on zero-filled buffers;
  * tensors lie further apart than one tensor is long; a second call gives the same bits; outputs and workspace sit between
    sentinel bands that stay intact;
  * an element whose bound is zero (an all-zero column, an all-zero question) is exactly zero.
wgrad_h2 at 256 x 256 also: MACX_TUNE_WGRAD_PIPE = 0 (the loop without the split issue) bit-equal to the default, and the pair form
(two contractions, one launch with grid.y = 2 at 2 / 3, two launches at 1) bit-equal to two single calls.
sb_h2w also: MACX_TUNE_SB_CONT = 0 bit-equal to the continuous stream wherever that runs; on three cases sb_h2_kernel on the same
inputs agrees with it within the sum of the two bounds.

`-s` or a failure prints one H2X line per case and tensor: worst observed / bound with the element, its output tile, the split or
question group, and the largest contributing row with its place in a 32-row stage.  Measured ratios: profiles/h2_contraction_errors.txt.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_kit
import h2_contraction_cases as hc
from abi_kit import Guarded, bits_equal, ptr

pytestmark = pytest.mark.gpu

EXTRA = 64                    # floats between one tensor's end and the next one's start


def _h2(macx, dev, x, fill):
    """x [nt][B][N][C] fp32 -> (buffer, stride in floats): nt H2 tensors of B * N rows, the buffer pre-filled with `fill` bytes"""
    L = macx._lib.lib()
    nt, B, N, Cc = x.shape
    stride = hc.h2_floats(B * N, Cc) + EXTRA
    assert stride == L.macx_h2_floats(B * N, Cc) + EXTRA and stride % 4 == 0
    buf = torch.full((nt * stride * 4,), fill, dtype=torch.uint8, device=dev).view(torch.float32)
    src = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for t in range(nt):
        macx._lib.check(L.macx_h2_from_f32(ptr(src[t]), B, N, Cc, ptr(buf[t * stride:]), None), "h2_from_f32")
    return buf, stride


def _round_trip(macx, dev, buf, stride, nt, rows, Cc):
    L = macx._lib.lib()
    out = torch.empty(nt, rows, Cc, device=dev)
    for t in range(nt):
        macx._lib.check(L.macx_h2_to_f32(ptr(buf[t * stride:]), rows, Cc, ptr(out[t]), None), "h2_to_f32")
    return out.cpu().numpy()


def _report(what, cid, name, got, ref, bound, where):
    r = hc.ratio(np.abs(got.astype(np.float64) - ref), bound)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    print("\nH2X %-6s %-34s %-5s worst observed / bound %.4f at %s  %s" % (what, cid, name, float(r[i]), tuple(int(v) for v in i), where(i)))
    return float(r[i]), i


# ================================================= wgrad_h2_kernel ================================================================
def _wgrad_call(macx, dev, c, bufs, strides, o=None, pair=None):
    """out (, out2) as guarded buffers + the guarded workspace; bufs = (A, G) H2 buffers"""
    L = macx._lib.lib()
    op = C.byref(o) if o is not None else None
    need = L.macx_h2_wgrad_ws_floats(op, c.nt, c.R, c.Kd, c.Jd, c.nsplit, int(pair is not None))
    assert need > 0
    ws = Guarded(need, dev)
    out = Guarded(c.Kd * c.Jd, dev)
    out2 = Guarded(c.Kd * c.Jd, dev) if pair is not None else None
    (a, g), (sa, sg) = bufs, strides
    a2, g2, sa2, sg2 = (pair[0][0], pair[0][1], pair[1][0], pair[1][1]) if pair is not None else (None, None, 0, 0)
    macx._lib.check(L.macx_h2_wgrad(op, c.nt, c.R, c.Kd, c.Jd, c.nsplit, ptr(a), sa, c.a_shared, ptr(g), sg, ptr(out.view),
                                    ptr(a2), sa2, c.a_shared, ptr(g2), sg2, ptr(out2.view) if out2 else None, ptr(ws.view), need, None),
                    "macx_h2_wgrad")
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and (out2 is None or out2.intact()), "wrote outside its buffers"
    return (out.np(c.Kd, c.Jd), out2.np(c.Kd, c.Jd) if out2 else None)


def _wgrad_buffers(macx, dev, c, fill):
    A, G = hc.wgrad_data(c)
    a, sa = _h2(macx, dev, A[:, None], fill)
    g, sg = _h2(macx, dev, G[:, None], fill)
    return (a, g), (sa, sg)


@pytest.mark.parametrize("c", hc.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_h2(macx, dev, c):
    M = c.nt * c.R
    o = hc.wgrad_operands(c, *hc.wgrad_data(c))
    ref = hc.wgrad_reference(o)
    bound, _ = hc.wgrad_bound(c, o)
    bufs, strides = _wgrad_buffers(macx, dev, c, 0xFF)
    nta = 1 if c.a_shared else c.nt
    A1 = _round_trip(macx, dev, bufs[0], strides[0], nta, c.R, c.Kd).reshape(-1, c.Kd)
    G1 = _round_trip(macx, dev, bufs[1], strides[1], c.nt, c.R, c.Jd).reshape(-1, c.Jd)
    assert bits_equal(A1[np.arange(M) % c.R] if c.a_shared else A1, o.A1) and bits_equal(G1, o.G1), "the format restatement is off"
    got, _ = _wgrad_call(macx, dev, c, bufs, strides)
    again, _ = _wgrad_call(macx, dev, c, bufs, strides)
    zero, _ = _wgrad_call(macx, dev, c, *_wgrad_buffers(macx, dev, c, 0))
    kw, jw = hc.wgrad_h2_kw(c.Kd), hc.wgrad_h2_jw(c.Jd)
    splits = hc.split_rows(M, c.nsplit)

    def where(i):
        m = int(np.argmax(np.abs(o.A1[:, i[0]].astype(np.float64) * o.G1[:, i[1]])))
        s = next(n for n, (b, e) in enumerate(splits) if b <= m < e)
        return "tile (%d,%d) of %dx%d, largest row %d: split %d, stage %d, row %d of the stage" % (
            i[0] // (128 * kw), i[1] // (128 * jw), 128 * kw, 128 * jw, m, s, (m - splits[s][0]) // 32, m % 32)

    worst, _ = _report("wgrad", c.id, "out", got, ref, bound, where)
    assert np.isfinite(got).all(), "not finite"
    assert worst <= 1.0
    assert (got[bound == 0] == 0).all()
    assert bits_equal(got, again), "a second call differs"
    assert bits_equal(got, zero), "NaN-filled pad rows change the result"
    if (c.Kd, c.Jd) == (256, 256):
        assert bits_equal(got, _wgrad_call(macx, dev, c, bufs, strides, o=abi_kit.opts(macx, wgrad_pipe=0))[0]), "WGRAD_PIPE = 0 differs"
        c2 = c._replace(seed=c.seed + 100)
        bufs2, strides2 = _wgrad_buffers(macx, dev, c2, 0xFF)
        single2, _ = _wgrad_call(macx, dev, c2, bufs2, strides2)
        o2 = hc.wgrad_operands(c2, *hc.wgrad_data(c2))
        assert float(hc.ratio(np.abs(single2.astype(np.float64) - hc.wgrad_reference(o2)), hc.wgrad_bound(c2, o2)[0]).max()) <= 1.0
        for pipe in (3, 2, 1):
            p1, p2 = _wgrad_call(macx, dev, c, bufs, strides, o=abi_kit.opts(macx, wgrad_pipe=pipe), pair=(bufs2, strides2))
            assert bits_equal(p1, got) and bits_equal(p2, single2), "the pair form at WGRAD_PIPE = %d differs from two single calls" % pipe


# ================================================= sb_h2_kernel / sb_h2w_kernel ===================================================
def _sb_buffers(macx, dev, c, fill):
    X, G, y, W = hc.sb_data(c)
    x, sx = _h2(macx, dev, X, fill)
    g, sg = _h2(macx, dev, G, fill)
    return (x, g, torch.from_numpy(y).to(dev), torch.from_numpy(W).to(dev)), (sx, sg)


def _sb_call(macx, dev, c, bufs, strides, o=None):
    """dW1a, dW1b [d][d], dy [nsteps][B][d] (None without dy)"""
    L = macx._lib.lib()
    op = C.byref(o) if o is not None else None
    need = L.macx_h2_sb_ws_floats(op, c.B, c.N, c.d, c.nsteps, c.qpg, c.wide)
    assert need == 2 * ((c.B + c.qpg - 1) // c.qpg) * c.d * c.d
    ws, dA, dB = Guarded(need, dev), Guarded(c.d * c.d, dev), Guarded(c.d * c.d, dev)
    nparts = 4 * c.d // 128
    dyp = Guarded(nparts * c.B * c.d, dev) if c.dy else None
    (x, g, y, W), (sx, sg) = bufs, strides
    macx._lib.check(L.macx_h2_sb(op, c.B, c.N, c.d, c.nsteps, c.qpg, c.wide, ptr(x), sx, ptr(g), sg, ptr(y), ptr(W), ptr(dA.view), ptr(dB.view),
                                 ptr(dyp.view) if dyp else None, ptr(ws.view), need, None), "macx_h2_sb")
    torch.cuda.synchronize()
    assert dA.intact() and dB.intact() and ws.intact() and (dyp is None or dyp.intact()), "wrote outside its buffers"
    parts = dyp.np(nparts, c.B, c.d) if dyp else None
    return dA.np(c.d, c.d), dB.np(c.d, c.d), parts


def _sb_case(macx, dev, c):
    """run one case; returns (got, ref, bound) of (dW1a, dW1b, dy) after every per-case assertion"""
    X, G, y, W = hc.sb_data(c)
    o = hc.sb_operands(c, X, G)
    ref, bound = hc.sb_reference(c, o, y, W), hc.sb_bound(c, o, y, W)
    bufs, strides = _sb_buffers(macx, dev, c, 0xFF)
    X1 = _round_trip(macx, dev, bufs[0], strides[0], c.nsteps, c.B * c.N, c.d)
    G1 = _round_trip(macx, dev, bufs[1], strides[1], c.nsteps, c.B * c.N, c.d)
    assert bits_equal(X1.reshape(o.X1.shape), o.X1) and bits_equal(G1.reshape(o.G1.shape), o.G1), "the format restatement is off"
    opts = abi_kit.opts(macx, sb_cont=c.cont) if c.wide else None
    got = _sb_call(macx, dev, c, bufs, strides, opts)
    again = _sb_call(macx, dev, c, bufs, strides, opts)
    zero = _sb_call(macx, dev, c, *_sb_buffers(macx, dev, c, 0), opts)
    groups = hc.sb_groups(c)
    tile_j = 256 if c.wide else 128

    def where(i):
        k, j = (i[2], None) if len(i) == 3 else i
        if j is None:
            return "question %d of step %d (group %d)" % (i[1], i[0], i[1] // c.qpg)
        w = np.abs(np.einsum("sbn,sbn->sbn", o.X1[..., k].astype(np.float64), o.G1[..., j]))
        s, b, n = np.unravel_index(int(np.argmax(w)), w.shape)
        return "tile (%d,%d) of 128x%d, largest row: step %d question %d (group %d of %d) row %d = stage %d, row %d of the stage" % (
            k // 128, j // tile_j, tile_j, s, b, b // c.qpg, len(groups), n, n // 32, n % 32)

    kern = "sb_h2w" if c.wide else "sb_h2"
    dy = got[2].astype(np.float64).sum(axis=0)[None] if c.dy else None          # the partials summed in fp64; nsteps = 1
    for name, g, r, b in (("dW1a", got[0], ref[0], bound[0]), ("dW1b", got[1], ref[1], bound[1]), ("dy", dy, ref[2], bound[2])):
        if g is None:
            continue
        worst, _ = _report(kern, c.id, name, g, r, b, where)
        assert np.isfinite(g).all(), "%s is not finite" % name
        assert worst <= 1.0, name
        assert (g[b == 0] == 0).all(), "%s: an element whose reference is exactly zero is not" % name
    for a, b, what in ((got, again, "a second call differs"), (got, zero, "NaN-filled pad rows change the result")):
        assert all(bits_equal(u, v) for u, v in zip(a, b) if u is not None), what
    return got, ref, bound, bufs, strides


@pytest.mark.parametrize("c", hc.NARROW_CASES, ids=lambda c: c.id)
def test_sb_h2(macx, dev, c):
    _sb_case(macx, dev, c)


@pytest.mark.parametrize("c", hc.WIDE_CASES, ids=lambda c: c.id)
def test_sb_h2w(macx, dev, c):
    got, ref, bound, bufs, strides = _sb_case(macx, dev, c)
    if hc.sb_cont(c.nsteps, c.N, c.qpg, c.cont):
        per_step = _sb_call(macx, dev, c, bufs, strides, abi_kit.opts(macx, sb_cont=0))
        assert bits_equal(got[0], per_step[0]) and bits_equal(got[1], per_step[1]), "SB_CONT = 0 differs from the continuous stream"
    if c in hc.BOTH_CASES:
        n = c._replace(wide=0)
        X, G, y, W = hc.sb_data(c)
        nb = hc.sb_bound(n, hc.sb_operands(n, X, G), y, W)
        narrow = _sb_call(macx, dev, n, bufs, strides)
        for i, name in enumerate(("dW1a", "dW1b")):
            r = hc.ratio(np.abs(narrow[i].astype(np.float64) - got[i]), bound[i] + nb[i])
            print("\nH2X both   %-34s %-5s |narrow - wide| / (sum of the two bounds) %.4f" % (c.id, name, float(r.max())))
            assert float(hc.ratio(np.abs(narrow[i].astype(np.float64) - ref[i]), nb[i]).max()) <= 1.0 and float(r.max()) <= 1.0, name
