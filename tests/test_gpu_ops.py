"""-m gpu: the ops.py primitives as single kernels (macx_op_*, mac-network_amd/csrc/macx_ops.hip.h), macx_embed_lookup_bwd and
macx_run_status_reset on their own, through the C ABI, against plain torch fp64 on the same fp32 inputs (dropout sites: against
oracle.dropout_hash.keep_mask).  The generic modules reach these kernels only at widths that are multiples of 8 and far below the
4096 x 256 thread grid cap; here: odd sizes, a second pass of the grid-stride loop, empty splits of the ROWS reduction, softmax rows of
length 0, the 32-bit wrap of the dropout index.

Bounds.  An elementwise result: 4 ulp of the fp64 result rounded to fp32 (what tanhf, expf and 1/sqrtf are held to).  A sum over k
terms: k 2^-23 sum |terms|.  Softmax and its backward are neither; their bounds are derived where they are used."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_kit import ptr, stream
from oracle import dropout_hash as dh
from helpers import make_case
from test_gpu_cell import build_cell

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
OVER_CAP = 1 + 4096 * 256 + 77        # op_grid caps the launch at 4096 workgroups of 256 threads: the loop takes a second pass
PRELU, RSQRT_EPS = 16, 17             # MACX_OP_PRELU, MACX_OP_RSQRT_EPS
ADD, MUL = 0, 1
B_SAME, B_MID, B_CHANNEL, B_ROW = 0, 1, 2, 3
R_MID, R_LAST, R_ROWS = 0, 1, 2
SITE_ENC_INPUT = 11


def _ulps(got, ref64):
    """(largest error in ulps of the fp64 reference rounded to fp32, its flat index)"""
    ref32 = ref64.to(torch.float32).abs()
    ulp = (torch.nextafter(ref32, torch.full_like(ref32, float("inf"))) - ref32).double()
    e = ((got.detach().cpu().double() - ref64).abs() / ulp).reshape(-1)
    i = int(e.argmax())
    return float(e[i]), i


def _assert_ulps(got, ref64, what, k=4.0):
    e, i = _ulps(got, ref64)
    print("\nOPS %s: %.2f ulp at %d" % (what, e, i))
    assert e <= k, "%s: %.2f ulp at flat index %d: got %r, fp64 %r" % (what, e, i, float(got.reshape(-1)[i]), float(ref64.reshape(-1)[i]))


SPECIALS = [0.0, -0.0, 1e-30, -1e-30, 10.0, -10.0, 30.0, -30.0, 60.0, -60.0]     # exact zero, +-tiny, large |x|


def _act_inputs(act, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    if act == RSQRT_EPS:                                    # a variance: >= 0
        x = x.abs()
        sp = [0.0, 1e-30, 1e-6, 1.0, 1e6, 1e12]
    else:
        sp = SPECIALS
    if n == 1:
        x[0] = 0.0
    elif n >= len(sp):
        x[:len(sp)] = torch.tensor(sp)
        x[-1] = sp[-1]                                       # (one in the loop's second pass where there is one)
    dy = torch.randn(n, generator=g)
    dy = torch.where(dy.abs() < 0.01, torch.full_like(dy, 0.01), dy)        # (no product near the denormal range)
    return x, dy


def _act_ref(act, x64, alpha64, inner):
    """fp64 activation of a flat tensor; PRELU: relu(x) - alpha[c] relu(-x), c = index % inner (ops.py:171-173)"""
    F = torch.nn.functional
    if act == 0:
        return x64 * 1.0
    if act == 1:
        return torch.tanh(x64)
    if act == 2:
        return torch.sigmoid(x64)
    if act == 3:
        return F.elu(x64)
    if act == 4:
        return torch.relu(x64)
    if act == PRELU:
        c = torch.arange(x64.numel()) % inner
        return torch.where(x64 > 0, x64, alpha64[c] * x64)
    return 1.0 / torch.sqrt(x64 + alpha64[0])


ACTS = [("NON", 0), ("TANH", 1), ("SIGMOID", 2), ("ELU", 3), ("RELU", 4), ("PRELU", PRELU), ("RSQRT_EPS", RSQRT_EPS)]


@pytest.mark.parametrize("n", [1, 255, 257, OVER_CAP])
@pytest.mark.parametrize("aname,act", ACTS)
def test_op_act_forward_and_backward(macx, dev, aname, act, n):
    """out = act(x) and dx = dy act'(x) (autograd on the fp64 activation) to 4 ulp; PRELU's dalpha_elem = dy min(x, 0) elementwise;
    RELU'(0) = 0 and PRELU'(0) = alpha (the kernels test v > 0)."""
    L = macx._lib.lib()
    inners = [1, 7, 100, 512] if act == PRELU else [7]
    for inner in inners:
        x, dy = _act_inputs(act, n, seed=act * 100 + inner)
        alpha = None
        if act == PRELU:
            alpha = torch.rand(inner, generator=torch.Generator().manual_seed(inner)) * 0.5 + 0.05
        elif act == RSQRT_EPS:
            alpha = torch.tensor([1e-5])
        xd, dyd = x.to(dev), dy.to(dev)
        ad = alpha.to(dev) if alpha is not None else None
        out, dx = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
        de = torch.full((n,), float("nan"), device=dev) if act == PRELU else None
        macx._lib.check(L.macx_op_act(act, ptr(xd), ptr(ad), n, inner, ptr(out), stream(dev)), "macx_op_act")
        macx._lib.check(L.macx_op_act_bwd(act, ptr(xd), ptr(ad), ptr(dyd), n, inner, ptr(dx), ptr(de), stream(dev)), "macx_op_act_bwd")
        torch.cuda.synchronize()
        x64 = x.double().requires_grad_(True)
        a64 = alpha.double().requires_grad_(True) if alpha is not None else None
        ref = _act_ref(act, x64, a64, inner)
        ref.backward(dy.double())
        dref = x64.grad
        if act in (1, 2):
            # autograd differentiates through the OUTPUT (1 - y^2, y (1 - y)), which cancels even in fp64 once y rounds to 1
            # (|x| = 30, 60 above): the closed form from the input is the reference there, autograd wherever it is well conditioned
            xd64 = x.double()
            closed = dy.double() * (torch.cosh(xd64) ** -2 if act == 1 else torch.sigmoid(xd64) * torch.sigmoid(-xd64))
            mild = xd64.abs() <= 5
            assert float(((dref - closed).abs() / closed.abs())[mild].max()) < 1e-9
            dref = closed
        tag = "%s n=%d inner=%d" % (aname, n, inner)
        _assert_ulps(out, ref.detach(), "act " + tag)
        _assert_ulps(dx, dref, "act_bwd " + tag)
        if act == PRELU:
            _assert_ulps(de, dy.double() * torch.clamp(x.double(), max=0.0), "dalpha_elem " + tag)
        zero = (x == 0).nonzero().reshape(-1)
        if act == 4:
            assert float(dx.cpu()[zero].abs().max()) == 0.0
        if act == PRELU:
            c = zero % inner
            assert torch.equal(dx.cpu()[zero], dy[zero] * alpha[c]) and float(de.cpu()[zero].abs().max()) == 0.0


@pytest.mark.parametrize("rows,inner", [(37, 7), (5, 100), (1, 512), (2049, 512)])
def test_prelu_dalpha_after_rows_reduction(macx, dev, rows, inner):
    """d alpha[c] = sum over rows of dalpha_elem (macx_op_reduce ROWS, as generic.py chains them) against autograd's d alpha:
    `rows` terms per channel; (2049, 512) is past the grid cap of the elementwise kernel"""
    L = macx._lib.lib()
    n = rows * inner
    x, dy = _act_inputs(PRELU, n, seed=rows)
    alpha = torch.rand(inner, generator=torch.Generator().manual_seed(1)) * 0.5 + 0.05
    xd, dyd, ad = x.to(dev), dy.to(dev), alpha.to(dev)
    dx, de = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ws = torch.full((64 * inner,), float("nan"), device=dev)
    da = torch.full((inner,), float("nan"), device=dev)
    macx._lib.check(L.macx_op_act_bwd(PRELU, ptr(xd), ptr(ad), ptr(dyd), n, inner, ptr(dx), ptr(de), stream(dev)), "macx_op_act_bwd")
    macx._lib.check(L.macx_op_reduce(R_ROWS, ptr(de), rows, 1, inner, ptr(da), ptr(ws), stream(dev)), "macx_op_reduce")
    torch.cuda.synchronize()
    x64, a64 = x.double(), alpha.double().requires_grad_(True)
    _act_ref(PRELU, x64, a64, inner).backward(dy.double())
    terms = (dy.double() * torch.clamp(x64, max=0.0)).reshape(rows, inner)
    tol = (rows + 1) * EPS * terms.abs().sum(dim=0) + 1e-300            # rows terms + the rounding of each product
    err = (da.cpu().double() - a64.grad).abs()
    print("\nOPS prelu dalpha rows=%d inner=%d: worst err / tol %.3f" % (rows, inner, float((err / tol).max())))
    assert bool((err <= tol).all()), float((err / tol).max())


def _binary_case(shape, bmode, g):
    outer, mid, inner = shape
    n = outer * mid * inner
    a = torch.randn(n, generator=g)
    nb = {B_SAME: n, B_MID: outer * inner, B_CHANNEL: inner, B_ROW: outer * mid}[bmode]
    b = torch.randn(nb, generator=g)
    a3 = a.double().reshape(outer, mid, inner)
    b64 = b.double()
    bb = {B_SAME: lambda: b64.reshape(outer, mid, inner), B_MID: lambda: b64.reshape(outer, 1, inner),
          B_CHANNEL: lambda: b64.reshape(1, 1, inner), B_ROW: lambda: b64.reshape(outer, mid, 1)}[bmode]()
    return a, b, a3, bb


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 196, 128), (9, 911, 128)])      # the last: 1,049,472 elements, past the grid cap
@pytest.mark.parametrize("bmode", [B_SAME, B_MID, B_CHANNEL, B_ROW])
@pytest.mark.parametrize("op", [ADD, MUL])
def test_op_binary(macx, dev, op, bmode, shape):
    """out = scale (a + b) | scale (a * b), b broadcast by mode, scale != 1: two roundings, inside the 4 ulp bound"""
    L = macx._lib.lib()
    outer, mid, inner = shape
    n = outer * mid * inner
    a, b, a3, bb = _binary_case(shape, bmode, torch.Generator().manual_seed(op * 10 + bmode))
    scale = float(np.float32(0.37))
    ad, bd = a.to(dev), b.to(dev)
    out = torch.full((n,), float("nan"), device=dev)
    macx._lib.check(L.macx_op_binary(op, bmode, ptr(ad), ptr(bd), n, mid, inner, scale, ptr(out), stream(dev)), "macx_op_binary")
    torch.cuda.synchronize()
    ref = scale * (a3 * bb if op == MUL else a3 + bb)          # (fl(a + b) is within 2^-24 of the SUM: cancellation costs nothing)
    _assert_ulps(out.reshape(a3.shape), ref, "binary %s mode %d %s" % ("MUL" if op == MUL else "ADD", bmode, shape))


def test_op_binary_refuses_a_size_its_broadcast_does_not_divide(macx, dev):
    L = macx._lib.lib()
    a = torch.zeros(100, device=dev)
    out = torch.zeros(100, device=dev)
    assert L.macx_op_binary(ADD, B_MID, ptr(a), ptr(a), 100, 5, 7, 1.0, ptr(out), stream(dev)) == macx._lib.MACX_EINVAL
    assert L.macx_op_binary(MUL, B_CHANNEL, ptr(a), ptr(a), 100, 1, 7, 1.0, ptr(out), stream(dev)) == macx._lib.MACX_EINVAL
    assert L.macx_op_binary(MUL, B_ROW, ptr(a), ptr(a), 100, 1, 7, 1.0, ptr(out), stream(dev)) == macx._lib.MACX_EINVAL
    assert L.macx_op_binary(MUL, B_MID, ptr(a), ptr(a), 100, 5, 10, 1.0, ptr(out), stream(dev)) == macx._lib.MACX_OK
    torch.cuda.synchronize()


def _reduce(macx, dev, mode, x, outer, mid, inner, n_out):
    L = macx._lib.lib()
    xd = x.to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((n_out,), float("nan"), device=dev)
        ws = torch.full((64 * inner,), float("nan"), device=dev) if mode == R_ROWS else None      # (NaN: an unwritten split would show)
        macx._lib.check(L.macx_op_reduce(mode, ptr(xd), outer, mid, inner, ptr(out), ptr(ws), stream(dev)), "macx_op_reduce")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])                    # fixed summation order
    return outs[0]


def _assert_sum(got, terms64, dim, k, what):
    ref = terms64.sum(dim=dim)
    tol = k * EPS * terms64.abs().sum(dim=dim) + 1e-300
    err = (got.double().reshape(ref.shape) - ref).abs()
    print("\nOPS %s: worst err / (k 2^-23 sum|terms|) %.3f" % (what, float((err / tol).max())))
    assert bool((err <= tol).all()), (what, float((err / tol).max()))


@pytest.mark.parametrize("outer,mid,inner", [(1, 1, 1), (3, 196, 100), (2, 1000, 257)])
def test_op_reduce_mid(macx, dev, outer, mid, inner):
    x = torch.randn(outer, mid, inner, generator=torch.Generator().manual_seed(mid))
    got = _reduce(macx, dev, R_MID, x, outer, mid, inner, outer * inner)
    _assert_sum(got, x.double(), 1, mid, "reduce MID %s" % ((outer, mid, inner),))
    if mid == 1:
        assert torch.equal(got.reshape(x[:, 0].shape), x[:, 0])


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("inner", [1, 63, 64, 65, 1000])
def test_op_reduce_last(macx, dev, rows, inner):
    x = torch.randn(rows, inner, generator=torch.Generator().manual_seed(inner))
    got = _reduce(macx, dev, R_LAST, x, rows, 1, inner, rows)
    _assert_sum(got, x.double(), 1, inner, "reduce LAST %s" % ((rows, inner),))


@pytest.mark.parametrize("outer", [1, 5, 63, 64, 65, 1000])
@pytest.mark.parametrize("inner", [1, 100, 300])
def test_op_reduce_rows(macx, dev, outer, inner):
    """the 64-way row split: fewer rows than splits leave empty splits, which must contribute exact zeros (one row: the sum IS the row)"""
    x = torch.randn(outer, inner, generator=torch.Generator().manual_seed(outer))
    got = _reduce(macx, dev, R_ROWS, x, outer, 1, inner, inner)
    assert bool(torch.isfinite(got).all())
    _assert_sum(got, x.double(), 0, outer, "reduce ROWS %s" % ((outer, inner),))
    if outer == 1:
        assert torch.equal(got, x[0])


def _masked_softmax64(x64, lens):
    n = x64.shape[1]
    col = torch.arange(n).reshape(1, n)
    keep = col < torch.clamp(lens, max=n).reshape(-1, 1)
    return torch.softmax(torch.where(keep, x64, torch.full_like(x64, float("-inf"))), dim=1), keep


def _softmax_tol(x, keep, a64):
    """(|x_c - m| + n + 4) 2^-23 a_c (+ the smallest normal number): derived in test_op_softmax_forward_and_backward"""
    x64 = x.double()
    m = torch.where(keep, x64, torch.full_like(x64, float("-inf"))).amax(dim=1, keepdim=True)
    return ((x64 - m).abs() + x.shape[1] + 4) * EPS * a64 + 2.0 ** -126


@pytest.mark.parametrize("rows", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_op_softmax_forward_and_backward(macx, dev, rows, n):
    """softmax over the last axis with the length mask of ops.expMask, and dx = a (da - sum a da) against autograd.
    Bounds (fp32 round-off of the kernel's own operation order, 2^-23 per rounding):
      a_c = exp(x_c - m) / s: the subtraction rounds to |x_c - m| 2^-24, which exp turns into that RELATIVE error; expf and the two
      roundings of 1 / s and the product add 4 more, the sum s over <= n terms of like sign n more:  |err| <= (|x_c - m| + n + 4) 2^-23 a_c;
      dx_c = a_c (da_c - t), t = sum a da over n terms: |err| <= |a_c| (n + 2) 2^-23 (sum |a da| + |da_c|) + 2 * 2^-23 |dx_c|
      (the kernel is given the fp32 rounding of the fp64 a that autograd differentiates: one more rounding of a, counted in n + 2).
    Masked columns are exact zeros; every row sums to 1 within n 2^-23."""
    L = macx._lib.lib()
    g = torch.Generator().manual_seed(rows * 1000 + n)
    x = torch.randn(rows, n, generator=g) * 3
    x[0, 0] = 80.0
    if n > 1:
        x[0, -1] = -80.0
        x[-1, n // 2] = -80.0
    da = torch.randn(rows, n, generator=g)
    variants = [("no lengths", None, 1), ("lengths", [n, 1, n + 5, max(1, n // 2), n, 2][:rows], 1)]
    if rows % 3 == 0:
        variants.append(("rows_per_len 3", [max(1, n - 1), 1][:rows // 3], 3))
    xd, dad = x.to(dev), da.to(dev)
    for what, lens, rpl in variants:
        ld = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
        out = torch.full((rows, n), float("nan"), device=dev)
        macx._lib.check(L.macx_op_softmax(ptr(xd), ptr(ld), rpl, rows, n, ptr(out), stream(dev)), "macx_op_softmax")
        torch.cuda.synchronize()
        row_len = torch.tensor(lens).repeat_interleave(rpl)[:rows] if lens is not None else torch.full((rows,), n)
        x64 = x.double().requires_grad_(True)
        a64, keep = _masked_softmax64(x64, row_len)
        got = out.cpu()
        assert float(got[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0
        tol = _softmax_tol(x, keep, a64.detach())
        err = (got.double() - a64.detach()).abs()
        ok = keep & (err > tol)
        print("\nOPS softmax rows=%d n=%d %s: worst err / tol %.3f" % (rows, n, what, float((err / tol)[keep].max())))
        assert not bool(ok.any()), (what, float((err / tol)[keep].max()))
        assert float((got.double().sum(dim=1) - 1.0).abs().max()) <= n * EPS
        # backward: the kernel differentiates the fp32 attention it is given
        a32 = a64.detach().to(torch.float32)
        dx = torch.full((rows, n), float("nan"), device=dev)
        a32d = a32.to(dev)
        macx._lib.check(L.macx_op_softmax_bwd(ptr(a32d), ptr(dad), rows, n, ptr(dx), stream(dev)), "macx_op_softmax_bwd")
        torch.cuda.synchronize()
        a64.backward(da.double())
        ad = a64.detach()
        btol = ad * (n + 2) * EPS * ((ad * da.double()).abs().sum(dim=1, keepdim=True) + da.double().abs()) + 2 * EPS * x64.grad.abs() + 2.0 ** -126
        berr = (dx.cpu().double() - x64.grad).abs()
        print("OPS softmax_bwd rows=%d n=%d %s: worst err / tol %.3f" % (rows, n, what, float((berr / btol).max())))
        assert bool((berr <= btol).all()), (what, float((berr / btol).max()))


@pytest.mark.parametrize("n", [1, 65])
def test_op_softmax_row_of_length_zero_is_nan(macx, dev, n):
    """softmax over no columns: the reference's 0 / 0 -- a NaN row; the rows next to it are untouched"""
    L = macx._lib.lib()
    x = torch.randn(3, n, generator=torch.Generator().manual_seed(n))
    lens = torch.tensor([n, 0, 1], dtype=torch.int32)
    xd, ld = x.to(dev), lens.to(dev)
    out = torch.full((3, n), 7.0, device=dev)
    macx._lib.check(L.macx_op_softmax(ptr(xd), ptr(ld), 1, 3, n, ptr(out), stream(dev)), "macx_op_softmax")
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[1]).all())
    a64, keep = _masked_softmax64(x[[0, 2]].double(), lens[[0, 2]])
    assert bool(torch.isfinite(got[[0, 2]]).all())
    assert bool(((got[[0, 2]].double() - a64).abs() <= _softmax_tol(x[[0, 2]], keep, a64))[keep].all())
    assert float(got[2, 1:].abs().max() if n > 1 else 0.0) == 0.0


@pytest.mark.parametrize("first,n", [(0, 1000), (2 ** 32 - 5, 100), (12345, OVER_CAP)])
def test_op_dropout_matches_the_numpy_stream(macx, dev, first, n):
    """out = x / keep * mask(seed, site, step, first + index); first = 2^32 - 5: the index wraps in 32 bits"""
    L = macx._lib.lib()
    seed, site, step, keep = 1234, dh.SITE_WRITE_INFO, 3, 0.85
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    xd = x.to(dev)
    for word in (None, 0xC0FFEE11):
        out = torch.full((n,), float("nan"), device=dev)
        if word is None:
            rc = L.macx_op_dropout(ptr(xd), n, seed, site, step, keep, first, ptr(out), stream(dev))
        else:
            wt = torch.tensor([word - (1 << 32)], dtype=torch.int32, device=dev)
            rc = L.macx_op_dropout_w(ptr(xd), n, seed, site, step, keep, first, ptr(wt), ptr(out), stream(dev))
        macx._lib.check(rc, "macx_op_dropout")
        torch.cuda.synchronize()
        mask = torch.from_numpy(dh.keep_mask(seed, site, step, keep, first, n, word=word or 0))
        got = out.cpu()
        assert float(got[mask == 0].abs().max() if bool((mask == 0).any()) else 0.0) == 0.0
        assert bool((got[mask == 1] != 0).all())
        _assert_ulps(got, x.double() / float(np.float32(keep)) * mask.double(), "dropout first=%d n=%d word=%s" % (first, n, word))


def test_op_dropout_keep_one_is_the_identity_and_bad_keeps_are_refused(macx, dev):
    L = macx._lib.lib()
    n = 1000
    x = torch.randn(n, generator=torch.Generator().manual_seed(1))
    x[:3] = torch.tensor([0.0, -0.0, 1e-30])
    xd = x.to(dev)
    out = torch.full((n,), float("nan"), device=dev)
    macx._lib.check(L.macx_op_dropout(ptr(xd), n, 7, 5, 0, 1.0, 2 ** 32 - 5, ptr(out), stream(dev)), "macx_op_dropout")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), x.view(torch.int32))
    for keep in (0.0, -0.1, 1.5, float("nan")):
        assert L.macx_op_dropout(ptr(xd), n, 7, 5, 0, keep, 0, ptr(out), stream(dev)) == macx._lib.MACX_EINVAL


@pytest.mark.parametrize("keep", [1.0, 0.8])
@pytest.mark.parametrize("E", [4, 7, 300, 1100])           # 1100: grid.y = 2 (1024 columns per workgroup)
def test_embed_lookup_bwd(macx, dev, E, keep):
    """d_emb[v - 1] = sum over the rows r with ids[r] == v of dx[r] * mask / keep (element index (first_row + r) E + c, site
    SITE_ENC_INPUT); pad rows (id 0) are skipped, a vocabulary row nobody looked up is written as zeros.  k rows per id: k 2^-23
    sum |terms|, + 2 for the rounding of each term's x * (1 / keep)."""
    L = macx._lib.lib()
    rows, V, ld, first_row, seed = 600, 37, E + 5, 77, 4321
    g = torch.Generator().manual_seed(E)
    ids = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)      # repeats; id V - 1 is left to the explicit entries
    ids[ids == 5] = 0                                                       # nobody looks word 5 up; more pad rows
    ids[:4] = torch.tensor([0, V, V, 1], dtype=torch.int32)                 # the pad id, the last id (twice), the first
    ids[-1] = V
    dx = torch.randn(rows, ld, generator=g)
    idd, dxd = ids.to(dev), dx.to(dev)
    outs = []
    for _ in range(2):
        demb = torch.full((V, E), float("nan"), device=dev)
        macx._lib.check(L.macx_embed_lookup_bwd(ptr(idd), ptr(dxd), rows, E, ld, V, keep, seed, first_row, ptr(demb), stream(dev)),
                        "macx_embed_lookup_bwd")
        torch.cuda.synchronize()
        outs.append(demb.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    mask = torch.from_numpy(dh.keep_mask(seed, SITE_ENC_INPUT, 0, keep, first_row * E, rows * E)).reshape(rows, E).double()
    terms = dx[:, :E].double() * mask / float(np.float32(keep))
    looked = ids > 0
    idx = (ids[looked] - 1).long()
    ref = torch.zeros(V, E, dtype=torch.float64).index_add_(0, idx, terms[looked])
    mag = torch.zeros(V, E, dtype=torch.float64).index_add_(0, idx, terms[looked].abs())
    k = torch.zeros(V, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    assert int(k[4]) == 0 and int(k[V - 1]) >= 3
    tol = (k.reshape(V, 1) + 2) * EPS * mag
    err = (outs[0].double() - ref).abs()
    print("\nOPS embed_lookup_bwd E=%d keep=%.1f: worst err / tol %.3f" % (E, keep, float((err / (tol + 1e-300)).max())))
    assert bool((err <= tol).all()), float((err / (tol + 1e-300)).max())
    assert float(outs[0][4].abs().max()) == 0.0


def test_run_status_reset_zeroes_the_status_words(macx, dev):
    """after a small d = 512 forward macx_run_status is OK; after macx_run_status_reset the 16 words of MACX_SEG_STATUS read zero.
    (The words are put there by writing them, never by making a run fail.)"""
    L = macx._lib.lib()
    cfg, vq, words, lengths, kb = make_case("args", 5, 5, 49, 512, 2)
    cell, params, _ = build_cell(macx, dev, cfg, vq, words, lengths, kb, False)
    with torch.no_grad():
        cell.run()
    run = cell._run
    args = (C.byref(run.opts), C.byref(run.shapes), run.keep, ptr(run.saved), C.c_size_t(run.saved_floats))
    bits, first = C.c_uint32(99), C.c_int32(99)
    assert L.macx_run_status(*args, stream(dev), C.byref(bits), C.byref(first)) == macx._lib.MACX_OK
    assert (bits.value, first.value) == (0, -1)
    off, cnt = C.c_size_t(0), C.c_size_t(0)
    assert L.macx_saved_segment(C.byref(run.opts), C.byref(run.shapes), run.keep, macx._lib.SEG["status"], C.byref(off), C.byref(cnt)) == 0
    assert cnt.value == 16
    status = run.saved.view(torch.int32)[off.value: off.value + 16]
    before = run.saved.clone()
    status.copy_(torch.arange(1, 17, dtype=torch.int32, device=dev))
    assert L.macx_run_status(*args, stream(dev), C.byref(bits), C.byref(first)) == macx._lib.MACX_EWAIT
    assert (bits.value, first.value) == (1, 1)
    assert L.macx_run_status_reset(*args, stream(dev)) == macx._lib.MACX_OK
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert torch.equal(run.saved.view(torch.int32), before.view(torch.int32))        # nothing but the 16 words changed (they were 0 before)
    assert L.macx_run_status(*args, stream(dev), C.byref(bits), C.byref(first)) == macx._lib.MACX_OK
    assert L.macx_run_status_reset(*args[:3], None, C.c_size_t(run.saved_floats), stream(dev)) == macx._lib.MACX_EINVAL
    assert L.macx_run_status_reset(*args[:4], C.c_size_t(run.saved_floats - 1), stream(dev)) == macx._lib.MACX_ESMALL
