"""-m gpu: the standalone contraction entry points -- macx_linear, macx_wgrad, macx_pack_weight, macx_h2_pack_weight(transpose = 1)
-- each on its own through the C ABI, against fp64 / a byte-for-byte layout built on the CPU.

macx_linear (small_linear_kernel<1> up to 128 rows, <4> above; 16-wide k-groups dealt to 4 waves, 8 groups per pass of the outer
loop = 512 k): per element
    |out - ref| <= (Ktot + 8) 2^-24 (sum_k |x w| + |b| + |bias_const|) + 4 ulp(ref)
the worst case of an fp32 chain of Ktot products + the 4-wave combine + the two bias adds, carried through an activation of slope
<= 1, plus the activation's own evaluation at the bound test_gpu_ops.py holds the op kernels to.  The result is bit-identical on a
second call and in all three GEMM families, rows outside [0, rows) of the output are never written, malformed calls return
MACX_EINVAL and write nothing.

macx_wgrad in the families 2 (H2: the process default; 32-row split granule, 128 x 256 tiles where Jd % 256 == 0), 1 (split-bf16)
and 0 (native f32), with nsplit == 1 (t.part = out) and nsplit > 1 (slab + slab_reduce) in every family, on contiguous operands
and on column slices of wider matrices (lda in {Kd + 4, Kd + 128, 2 Kd}, ldg in {Jd + 4, 2 Jd}; 1e30 outside the slice), on
N(0,1) data and on rows scaled by e^(+-4) with 1e-30 / -3e20 / 65504 / 0 entries.  Per element, per unit of S = sum_m |A G|:
    family 0:     err / S <= (M + nsplit + 4) 2^-24                       (fp32 chain + fixed-order slab sum)
    families 1/2: max and mean of err / S <= 1.5 x family 0's on the same data + 2^-23
    everywhere:   err / S < 1e-6
(for M = 1 the exact-zero entry is left out of the special values: the one-term sum would have S = 0.)

macx_pack_weight: the three documented byte layouts of include/macx.h, compared bit for bit; BF16X3 against the round-to-nearest
residual chain through torch.bfloat16, whose three pieces add up to the fp32 value EXACTLY in fp64 for every element of the input
(checked on the CPU first); the transpose bit (16-byte fast path, and the scalar path from a source 4 bytes off a 16-byte boundary);
nothing written behind the documented size.

macx_h2_pack_weight(W^T, transpose = 1) == macx_h2_pack_weight(W, 0) bit for bit (planes + exponent word), and a product on the
transposed pack meets the bound of test_gpu_h2.py::test_h2_gemm_error_is_fp32_class.

`-s` prints one GEMMX line per case.  Measured on an MI355X when this file was added (55 tests, 2.6 s for the whole file):
  macx_linear   largest err / bound over the 17 cases 0.113 (rows = 129, k = 16, n_out = 512, RELU; 0.16 of that bound is the 4 ulp
                term); next 0.025 (1 x 16 x 16), 0.021 (129 x 48 x 16 ELU); every K >= 112 case below 0.01.  Nothing above half.
  macx_wgrad    largest err / S: family 0 4.88e-07 (M = 257, 256 x 384, wide; 0.031 of its bound), families 1 and 2 5.08e-07 (M = 64,
                128 x 256, wide).  Largest err / bound of family 0: 0.176 (M = 33, wide); at M = 1 it is 2^-24 / (6 x 2^-24) = 0.166:
                one rounding.  Ratio of maxima family 1 / family 0 and family 2 / family 0: 0.48 .. 2.24, the largest at M = 1
                (1.33e-07 against one rounding of 5.9e-08: six bf16 terms, fp32 adds), 1.72 at most for M > 1 (family 2, M = 129,
                N(0,1)); ratio of means 0.46 .. 1.32.  Against 1.5 x family 0 + 2^-23: largest 0.68 (family 1) and 0.76 (family 2,
                M = 65, 256 x 384, wide) for the maxima, 0.34 for the means.  Those two and the 5.08e-07 against the 1e-6 cap sit
                ABOVE HALF of their bounds, and the bounds stand: a kernel exactly as accurate as the native one sits at
                1 / 1.5 = 0.67 of the relative bound by construction -- it separates "fp32-class" from "twice the native error",
                not good from perfect -- and under e^(+-4) row scales a handful of rows carry each sum, so the native fp32 chain
                itself reaches 4.9e-07 of S on this data (N(0,1) data: all families <= 2.2e-07).
  h2 pack^T     product error per unit of sum |a w| + |b|: max 2.4e-07 .. 2.8e-07, mean 1.6e-08 .. 2.1e-08.
Family 2 runs the same split-bf16 kernel as family 1 here (wgrad_any); only nsplit's tile width and the 32-row split granule differ,
so the two agree bit for bit wherever one split holds all rows (M <= 64) and where 64-row splits are both granules' (M = 1001).
"""
import ctypes as C

import pytest
import torch

from abi_kit import GUARD, SENT, Guarded, bits, ptr
from helpers import default_gemm_mode

pytestmark = pytest.mark.gpu

def _ulp32(ref64):
    r = ref64.float()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


# ================================================= 1. macx_linear =================================================================
ACTS = {"NON": lambda t: t, "TANH": torch.tanh, "SIGMOID": torch.sigmoid, "ELU": torch.nn.functional.elu, "RELU": torch.relu}

# every value of rows {1, 15, 16, 17, 128, 129, 191, 1000} (one ragged 16-row tile, full, full + 1; the <1>/<4> switch at 128/129;
# a ragged 64-row tile; many workgroups), of (k1, k2) {(16,0), (48,0): waves without a k-group; (64,16), (112,16), (512,16): a second
# segment off a 64-k boundary; (528,0), (1040,0): a single group in the 2nd / 3rd pass; (256,256)}, of n_out {16, 48, 512}, of the
# five activations, and bias_const != 0 -- each at least twice, 17 of the 960 combinations
LINEAR_CASES = [
    (1, 16, 0, 16, "NON", 0.25), (15, 48, 0, 48, "TANH", -0.5), (16, 64, 16, 16, "SIGMOID", 0.25), (17, 112, 16, 48, "ELU", 0.25),
    (128, 512, 16, 16, "RELU", -0.5), (129, 528, 0, 48, "TANH", 0.25), (191, 1040, 0, 16, "ELU", -0.5),
    (1000, 256, 256, 512, "SIGMOID", 0.25), (1000, 1040, 0, 512, "NON", -0.5), (129, 16, 0, 512, "RELU", 0.25),
    (128, 1040, 0, 48, "SIGMOID", -0.5), (17, 528, 0, 512, "NON", 0.25), (191, 64, 16, 48, "RELU", 0.25),
    (1, 512, 16, 512, "ELU", 0.25), (15, 256, 256, 16, "TANH", 0.25), (16, 112, 16, 512, "NON", -0.5),
    (129, 48, 0, 16, "ELU", -0.5),
]


def _linear_inputs(rows, k1, k2, n_out):
    g = torch.Generator().manual_seed(rows * 7919 + k1 * 31 + k2 * 3 + n_out)
    x1 = torch.randn(rows, k1, generator=g)
    x2 = torch.randn(rows, k2, generator=g) if k2 else None
    W = torch.randn(k1 + k2, n_out, generator=g) / (k1 + k2) ** 0.5
    b = torch.randn(n_out, generator=g)
    return x1, x2, W, b


def _call_linear(macx, x1, k1, x2, k2, rows, wp, b, bc, n_out, act, out):
    return macx._lib.lib().macx_linear(ptr(x1), k1, ptr(x2), k2, rows, ptr(wp), ptr(b), bc, n_out, macx._lib.ACT[act], ptr(out), None)


@pytest.mark.parametrize("rows,k1,k2,n_out,act,bc", LINEAR_CASES)
def test_linear_against_fp64(macx, dev, rows, k1, k2, n_out, act, bc):
    L = macx._lib.lib()
    x1, x2, W, b = _linear_inputs(rows, k1, k2, n_out)
    xin = (x1 if x2 is None else torch.cat([x1, x2], dim=1)).double()
    ref = ACTS[act](xin @ W.double() + b.double() + bc)
    S = xin.abs() @ W.double().abs() + b.double().abs() + abs(bc)
    bound = (k1 + k2 + 8) * 2.0 ** -24 * S + 4.0 * _ulp32(ref)
    x1d, Wd, bd = x1.to(dev), W.to(dev), b.to(dev)
    x2d = x2.to(dev) if x2 is not None else None
    wp = torch.empty_like(Wd)
    macx._lib.check(L.macx_pack_weight(ptr(Wd), k1 + k2, n_out, 0, ptr(wp), None), "pack")
    # a ragged tile's clamped rows would land behind row rows - 1: up to 63 rows of n_out floats, all inside the guard zone
    outs = [Guarded(rows * n_out, dev, after=64 * n_out + GUARD) for _ in range(5)]
    try:
        for o, mode in zip(outs, (None, None, 0, 1, 2)):
            if mode is not None:
                L.macx_gemm_mode(mode)
            macx._lib.check(_call_linear(macx, x1d, k1, x2d, k2, rows, wp, bd, bc, n_out, act, o.view), "linear")
    finally:
        L.macx_gemm_mode(default_gemm_mode())
    torch.cuda.synchronize()
    got = outs[0].view.cpu().double().reshape(rows, n_out)
    ratio = (got - ref).abs() / bound
    worst = int(ratio.argmax())
    print("\nGEMMX linear rows=%d k=(%d,%d) n_out=%d %s: err/bound %.4f at (%d,%d), of which activation ulps %.2f"
          % (rows, k1, k2, n_out, act, float(ratio.max()), worst // n_out, worst % n_out,
             float(4.0 * _ulp32(ref).reshape(-1)[worst] / bound.reshape(-1)[worst])))
    assert torch.isfinite(got).all()
    assert float(ratio.max()) <= 1.0, "err/bound %.3f at row %d column %d" % (float(ratio.max()), worst // n_out, worst % n_out)
    for o in outs:
        assert o.intact(), "macx_linear wrote outside rows [0, %d) of its output" % rows
    assert torch.equal(bits(outs[0].view), bits(outs[1].view)), "second call differs"
    for o, mode in zip(outs[2:], (0, 1, 2)):
        assert torch.equal(bits(outs[0].view), bits(o.view)), "family %d differs" % mode


def test_linear_guards(macx, dev):
    rows, k1, k2, n_out = 8, 32, 16, 16
    x1 = torch.randn(rows * k1 + 8, device=dev)
    x2 = torch.randn(rows, k2, device=dev)
    wp = torch.randn(k1 + k2, n_out, device=dev)
    b = torch.randn(n_out, device=dev)
    off = x1[1:]                                   # 4 bytes past a 16-byte boundary
    assert x1.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    bad = {"k1 = 24": (x1, 24, None, 0, rows, n_out), "n_out = 8": (x1, k1, None, 0, rows, 8),
           "k2 > 0, x2 NULL": (x1, k1, None, k2, rows, n_out), "x2 set, k2 = 0": (x1, k1, x2, 0, rows, n_out),
           "x1 off a 16-byte boundary": (off, k1, None, 0, rows, n_out), "rows = 0": (x1, k1, None, 0, 0, n_out)}
    for what, (a1, kk1, a2, kk2, r, n) in bad.items():
        o = Guarded(rows * n_out, dev)
        assert _call_linear(macx, a1, kk1, a2, kk2, r, wp, b, 0.25, n, "NON", o.view) == macx._lib.MACX_EINVAL, what
        torch.cuda.synchronize()
        assert o.untouched(), what
    o = Guarded(rows * n_out, dev)                # the same operands, well-formed: the guards above did not reject a legal call
    macx._lib.check(_call_linear(macx, x1, k1, x2, k2, rows, wp, b, 0.25, n_out, "NON", o.view), "linear")
    torch.cuda.synchronize()
    assert o.intact() and bool((o.view != SENT).all())


# ================================================= 2. macx_wgrad ==================================================================
# (M, Kd, Jd, lda - Kd as a key, ldg - Jd as a key); keys: 0 contiguous, "+4", "+128", "x2".  M = 1 .. 64: nsplit == 1 (one split
# per 64 rows at least), M = 65 .. 1001: nsplit = 2 .. 16, in every family (test_wgrad_cases_take_both_routes)
WGRAD_CASES = [
    (1, 128, 128, 0, 0), (1, 128, 256, "+128", "x2"), (31, 128, 256, "+4", "+4"), (32, 128, 128, "x2", "x2"),
    (33, 256, 384, "+128", "+4"), (63, 128, 128, "+4", "x2"), (64, 128, 256, "+128", "x2"), (65, 128, 128, "x2", "+4"),
    (65, 256, 384, 0, 0), (129, 128, 256, "+4", "+4"), (257, 128, 128, 0, 0), (257, 256, 384, "+128", "x2"),
    (1001, 128, 256, "x2", "+4"), (1001, 256, 384, "+4", "x2"),
]
_LD = {0: lambda n: (n, 0), "+4": lambda n: (n + 4, 4), "+128": lambda n: (n + 128, 64), "x2": lambda n: (2 * n, 36)}   # (ld, first column)


def _wgrad_data(M, Kd, Jd, data):
    g = torch.Generator().manual_seed(M * 131 + Kd + Jd)
    A = torch.randn(M, Kd, generator=g)
    G = torch.randn(M, Jd, generator=g)
    if data == "wide":
        A = A * torch.exp(4 * torch.randn(M, 1, generator=g))
        G = G * torch.exp(4 * torch.randn(M, 1, generator=g))
        A[0, :7] = torch.tensor([1e-30, -3e20, 1.0, -1.0, 65504.0, 1e-8, 3.14159274])
        if M > 1:
            A[0, 7] = 0.0
    return A, G


def _strided(X, kind, dev):
    """X as a column slice of a wider row-major device matrix whose other columns hold 1e30 -> (owner, pointer, ld)"""
    ld, c0 = _LD[kind](X.shape[1])
    full = torch.full((X.shape[0], ld), 1e30)
    full[:, c0:c0 + X.shape[1]] = X
    full = full.to(dev)
    ptr = full.data_ptr() + 4 * c0
    assert ptr % 16 == 0 and ld % 4 == 0
    return full, C.c_void_p(ptr), ld


@pytest.mark.parametrize("data", ["wide", "normal"])
@pytest.mark.parametrize("M,Kd,Jd,lda_kind,ldg_kind", WGRAD_CASES)
def test_wgrad_three_families(macx, dev, M, Kd, Jd, lda_kind, ldg_kind, data):
    L = macx._lib.lib()
    A, G = _wgrad_data(M, Kd, Jd, data)
    ref = A.double().t() @ G.double()
    S = A.double().abs().t() @ G.double().abs()
    assert bool((S > 0).all()) and bool(torch.isfinite(S).all())          # no element is skipped
    Af, Ap, lda = _strided(A, lda_kind, dev)
    Gf, Gp, ldg = _strided(G, ldg_kind, dev)
    stats, keep = {}, []
    try:
        for mode in (0, 1, 2):
            L.macx_gemm_mode(mode)
            ns = L.macx_wgrad_splits(M, Kd, Jd)
            assert ns >= 1
            outs = [Guarded(Kd * Jd, dev), Guarded(Kd * Jd, dev)]
            ws = Guarded(ns * Kd * Jd, dev)
            for o in outs:
                macx._lib.check(L.macx_wgrad(Ap, lda, Gp, ldg, M, Kd, Jd, ptr(o.view), ptr(ws.view), None), "wgrad")
            keep.append((mode, ns, outs, ws))
    finally:
        L.macx_gemm_mode(default_gemm_mode())
    torch.cuda.synchronize()
    for mode, ns, outs, ws in keep:
        got = outs[0].view.cpu().double().reshape(Kd, Jd)
        assert torch.isfinite(got).all()
        e = (got - ref).abs() / S
        stats[mode] = (float(e.max()), float(e.mean()), ns)
        assert outs[0].intact() and outs[1].intact() and ws.intact(), "family %d wrote out of bounds" % mode
        assert torch.equal(bits(outs[0].view), bits(outs[1].view)), "family %d: second call differs" % mode
    (m0, a0, ns0), (m1, a1, ns1), (m2, a2, ns2) = stats[0], stats[1], stats[2]
    b0 = (M + ns0 + 4) * 2.0 ** -24
    print("\nGEMMX wgrad M=%d %dx%d lda=%d ldg=%d %s: err/S max (mean) family 0 %.3e (%.3e) = %.3f of its bound, nsplit %d | 1 %.3e (%.3e) "
          "x%.2f, nsplit %d | 2 %.3e (%.3e) x%.2f, nsplit %d"
          % (M, Kd, Jd, lda, ldg, data, m0, a0, m0 / b0, ns0, m1, a1, m1 / max(m0, 1e-300), ns1, m2, a2, m2 / max(m0, 1e-300), ns2))
    assert m0 <= b0, (m0, b0)
    for mode, (mx, mean, _) in ((1, stats[1]), (2, stats[2])):
        assert mx <= 1.5 * m0 + 2.0 ** -23, (mode, mx, m0)
        assert mean <= 1.5 * a0 + 2.0 ** -23, (mode, mean, a0)
    assert max(m0, m1, m2) < 1e-6, stats


def test_wgrad_cases_take_both_routes(macx, dev):
    """in every family WGRAD_CASES holds cases with nsplit == 1 (the kernel writes `out`) and with nsplit > 1 (slab + slab_reduce)"""
    L = macx._lib.lib()
    try:
        for mode in (0, 1, 2):
            L.macx_gemm_mode(mode)
            ns = [L.macx_wgrad_splits(M, Kd, Jd) for M, Kd, Jd, _, _ in WGRAD_CASES]
            assert min(ns) == 1 and max(ns) > 1, (mode, ns)
    finally:
        L.macx_gemm_mode(default_gemm_mode())


def test_wgrad_guards(macx, dev):
    L = macx._lib.lib()
    M, Kd, Jd = 8, 128, 128
    A = torch.randn(M, 2 * Kd, device=dev)
    G = torch.randn(M, 2 * Jd, device=dev)
    ws = Guarded(2 * Kd * Jd, dev)
    bad = {"Kd = 64": (2 * Kd, M, 64, Jd, ws.view), "Jd = 192": (2 * Kd, M, Kd, 192, ws.view), "lda = Kd + 2": (Kd + 2, M, Kd, Jd, ws.view),
           "M = 0": (2 * Kd, 0, Kd, Jd, ws.view), "ws NULL": (2 * Kd, M, Kd, Jd, None)}
    for what, (lda, m, kd, jd, w) in bad.items():
        o = Guarded(Kd * 2 * Jd, dev)
        assert L.macx_wgrad(ptr(A), lda, ptr(G), 2 * Jd, m, kd, jd, ptr(o.view), ptr(w), None) == macx._lib.MACX_EINVAL, what
        torch.cuda.synchronize()
        assert o.untouched() and ws.untouched(), what
    assert L.macx_wgrad_splits(M, 64, Jd) == macx._lib.MACX_EINVAL and L.macx_wgrad_splits(0, Kd, Jd) == macx._lib.MACX_EINVAL


# ================================================= 3. macx_pack_weight ============================================================
PACK_SPECIALS = [0.0, 1.0, -1.0, 65504.0, 3.14159274]


def _pack_input(K, n_out):
    """N(0,1) x 2^u, u uniform in [-12, 12], + the special values: fp32 values whose three-piece bf16 chain is exact (no subnormals)"""
    g = torch.Generator().manual_seed(K * 1000 + n_out)
    W = torch.randn(K, n_out, generator=g) * torch.exp2((torch.rand(K, n_out, generator=g) * 2 - 1) * 12)
    W.reshape(-1)[:len(PACK_SPECIALS)] = torch.tensor(PACK_SPECIALS)
    return W


def _bf16_chain(W):
    h1 = W.to(torch.bfloat16)
    r1 = W - h1.float()
    h2 = r1.to(torch.bfloat16)
    h3 = (r1 - h2.float()).to(torch.bfloat16)
    return h1, h2, h3


def _expected_pack(W, fmt):
    """include/macx.h's layouts as int32 words"""
    K, n_out = W.shape
    if fmt == 0:                                   # out[Q][g][j][e] = W[16Q + 4g + e][j]
        return bits(W.reshape(K // 16, 4, 4, n_out).permute(0, 1, 3, 2).reshape(-1))
    if fmt == 2:                                   # out[kt][j][kk] = W[32 kt + kk][j]
        return bits(W.reshape(K // 32, 32, n_out).permute(0, 2, 1).reshape(-1))
    planes = [h.reshape(K // 32, 32, n_out).permute(0, 2, 1) for h in _bf16_chain(W)]       # [K/32][3][n_out][32] bf16
    return torch.stack(planes, dim=1).contiguous().reshape(-1).view(torch.int32)


def _pack(macx, dev, src, K, n_out, flags):
    n = K * n_out * 3 // 2 if (flags >> 1) == 1 else K * n_out
    o = Guarded(n, dev)
    macx._lib.check(macx._lib.lib().macx_pack_weight(src, K, n_out, flags, ptr(o.view), None), "pack")
    torch.cuda.synchronize()
    assert o.intact(), "macx_pack_weight(flags = %d) wrote behind its %d floats" % (flags, n)
    return bits(o.view)


@pytest.mark.parametrize("K,n_out", [(16, 16), (32, 48), (96, 16), (512, 128)])
def test_pack_weight_byte_layout(macx, dev, K, n_out):
    W = _pack_input(K, n_out)
    # CPU first: the chain reconstructs every element exactly, and no piece is subnormal
    h = _bf16_chain(W)
    assert torch.equal(h[0].double() + h[1].double() + h[2].double(), W.double())
    tiny = torch.finfo(torch.float32).tiny
    assert all(bool(((p.float() == 0) | (p.float().abs() >= tiny)).all()) for p in h + (W,))
    Wd = W.to(dev)
    Wt = W.t().contiguous().to(dev)                                         # [n_out, K]
    shifted = torch.empty(K * n_out + 8, device=dev)
    shifted[1:1 + K * n_out] = Wt.reshape(-1)
    assert shifted.data_ptr() % 16 == 0
    off = C.c_void_p(shifted.data_ptr() + 4)                                # W^T from 4 bytes past a 16-byte boundary: the scalar path
    for fmt in (0, 1, 2):
        if fmt and K % 32:
            assert macx._lib.lib().macx_pack_weight(ptr(Wd), K, n_out, fmt << 1, ptr(shifted), None) == macx._lib.MACX_EINVAL
            continue
        want = _expected_pack(W, fmt)
        got = _pack(macx, dev, ptr(Wd), K, n_out, fmt << 1)
        assert torch.equal(got, want), "format %d: %d of %d words differ from include/macx.h's layout" % (fmt, int((got != want).sum()), want.numel())
        got_t = _pack(macx, dev, ptr(Wt), K, n_out, (fmt << 1) | 1)
        assert torch.equal(got_t, got), "format %d: the transposed source packs differently" % fmt
        if fmt == 0:
            got_s = _pack(macx, dev, off, K, n_out, 1)
            assert torch.equal(got_s, got), "format 0: the scalar path of a transposed source packs differently"
        if fmt == 1:                                                        # "exact split": what the GPU wrote adds up to W in fp64
            pl = got.view(torch.bfloat16).reshape(K // 32, 3, n_out, 32).double().sum(dim=1)                 # [K/32][n_out][32]
            assert torch.equal(pl.permute(0, 2, 1).reshape(K, n_out), W.double())


# ================================================= 4. macx_h2_pack_weight, transpose = 1 ==========================================
@pytest.mark.parametrize("K,n_out", [(128, 128), (128, 384), (512, 256)])
def test_h2_pack_weight_transposed(macx, dev, K, n_out):
    L = macx._lib.lib()
    B, N = 2, 49
    g = torch.Generator().manual_seed(4 + K + n_out)
    A = torch.randn(B, N, K, generator=g) * torch.exp(4 * torch.randn(B, N, 1, generator=g))
    A[0, 0, :8] = torch.tensor([1e-30, -3e20, 1.0, -1.0, 65504.0, 1e-8, 3.14159274, 0.0])
    W = torch.randn(K, n_out, generator=g) / 22            # asymmetric: a pack that ignored the flag multiplies by another matrix
    b = torch.randn(n_out, generator=g)
    ref = A.double().reshape(-1, K) @ W.double() + b.double()
    scale = A.double().abs().reshape(-1, K) @ W.double().abs() + b.double().abs() + 1e-300
    Ad, Wd, bd = A.to(dev), W.to(dev), b.to(dev)
    Wt = W.t().contiguous().to(dev)
    n = K * n_out + 16                                     # the documented size
    plain, trans = Guarded(n, dev), Guarded(n, dev)
    macx._lib.check(L.macx_h2_pack_weight(ptr(Wd), K, n_out, 0, ptr(plain.view), None), "h2 pack")
    macx._lib.check(L.macx_h2_pack_weight(ptr(Wt), K, n_out, 1, ptr(trans.view), None), "h2 pack^T")
    hA = torch.empty(L.macx_h2_floats(B * N, K), device=dev)
    hO = torch.empty(L.macx_h2_floats(B * N, n_out), device=dev)
    out = torch.empty(B * N, n_out, device=dev)
    macx._lib.check(L.macx_h2_from_f32(ptr(Ad), B, N, K, ptr(hA), None), "from")
    macx._lib.check(L.macx_h2_gemm_planes(ptr(hA), B, N, K, ptr(trans.view), n_out, ptr(bd), 0, ptr(hO), None), "planes")
    macx._lib.check(L.macx_h2_to_f32(ptr(hO), B * N, n_out, ptr(out), None), "to")
    torch.cuda.synchronize()
    assert plain.intact() and trans.intact()
    pb, tb = bits(plain.view), bits(trans.view)
    assert torch.equal(pb[:K * n_out + 1], tb[:K * n_out + 1]), "%d plane words differ, exponent %d vs %d" % (
        int((pb[:K * n_out] != tb[:K * n_out]).sum()), int(pb[K * n_out]), int(tb[K * n_out]))
    e = (out.cpu().double() - ref).abs() / scale
    emax, emean = float(e.max()), float(e.mean())
    print("\nGEMMX h2 pack^T K=%d n_out=%d: product err per unit of sum|a w| + |b| max %.3e mean %.3e" % (K, n_out, emax, emean))
    assert emax < 1e-6 and emean < 5e-8, (emax, emean)
