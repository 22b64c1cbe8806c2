"""-m gpu: the length-aware gather of questions that share images (macx_kb_gather_l / macx_kb_gather_bwd_l) on its own.  Every
comparison is one of bits: the forward against indexing with the rows behind each image's size zeroed, the per-question lengths
against clamp(image_lengths)[index], the backward against the ascending fp32 loop on the CPU restricted to the live rows.

Shapes (G, B, N, d): (3, 5, 9, 8) -- a block of 18 quads, far below one 1,024-quad chunk; (3, 5, 70, 64) -- 16 quads per row, so row
64 starts exactly at quad 1,024 and the sizes 1 / 64 / 65 / 70 put the live / padded boundary before, on and behind a chunk edge
(and 64 rows = 1,024 quads = four of the backward kernel's 256-quad chunks).  Sizes 0 and N + 3 exercise the clamp.  The padded rows
of every source hold NaN: a kernel that read them would show it."""
import pytest
import torch

from abi_kit import Guarded, bits_equal, ptr

pytestmark = pytest.mark.gpu

SMALL, EDGE = (3, 5, 9, 8), (3, 5, 70, 64)
# (shape, index, image_lengths)
CASES = {"small, image 1 unnamed": (SMALL, [2, 0, 0, 2, 0], [4, 9, 1]),
         "small, clamp 0 and N+3": (SMALL, [1, 2, 0, 1, 1], [0, 12, 5]),
         "edge 1/64/65": (EDGE, [2, 0, 1, 2, 0], [1, 64, 65]),
         "edge 70/64/65, image 1 unnamed": (EDGE, [0, 2, 2, 0, 2], [70, 64, 65]),
         "edge 65/1/64": (EDGE, [1, 0, 2, 2, 1], [65, 1, 64]),
         "edge, clamp 0 and N+3": (EDGE, [0, 1, 2, 1, 0], [0, 73, 64]),
         "small, index out of range": (SMALL, [2, -1, 0, 3, 0], [4, 9, 1]),
         "edge, index out of range": (EDGE, [3, 0, 1, -1, 0], [64, 65, 1])}


def clamp(lengths, N):
    return [min(max(x, 1), N) for x in lengths]


def forward(macx, src, index, lengths, shape, dev):
    """macx_kb_gather_l into guarded outputs: (rc, kb buffer, kb [B,N,d], lengths buffer, kb_lengths [B])"""
    G, B, N, d = shape
    kbuf, lbuf = Guarded(B * N * d, dev), Guarded(B, dev, dtype=torch.int32, fill=-12345)      # (the default sentinel is no int32)
    kb, kbl = kbuf.view.fill_(float("nan")), lbuf.view.fill_(-7)                                # the outputs' pre-fill
    rc = macx._lib.lib().macx_kb_gather_l(ptr(src), ptr(index), ptr(lengths), G, B, N, d, ptr(kb), ptr(kbl), None)
    torch.cuda.synchronize()
    return rc, kbuf, kb.view(B, N, d), lbuf, kbl


def backward(macx, dkb, index, lengths, shape, dev):
    G, B, N, d = shape
    buf = Guarded(G * N * d, dev)
    out = buf.view.fill_(float("nan"))
    rc = macx._lib.lib().macx_kb_gather_bwd_l(ptr(dkb), ptr(index), ptr(lengths), G, B, N, d, ptr(out), None)
    torch.cuda.synchronize()
    return rc, buf, out.view(G, N, d)


@pytest.fixture(scope="module")
def data():
    """per case, on the CPU, computed once: the source with NaN in every image's padded rows and the expected gather; the output
    gradient with NaN in every question's padded rows and the expected ascending sum"""
    out = {}
    for case, ((G, B, N, d), index, lengths) in CASES.items():
        g = torch.Generator().manual_seed(len(case))
        L = clamp(lengths, N)
        src = torch.randn(G, N, d, generator=g)
        for i in range(G):
            src[i, L[i]:] = float("nan")
        want = torch.zeros(B, N, d)
        want_len = torch.empty(B, dtype=torch.int32)
        dkb = torch.randn(B, N, d, generator=g)
        want_bwd = torch.zeros(G, N, d)
        for b, i in enumerate(index):                     # b ascending: the order of the kernel's plain fp32 adds
            if 0 <= i < G:
                want[b, :L[i]] = src[i, :L[i]]
                want_len[b] = L[i]
                dkb[b, L[i]:] = float("nan")
                want_bwd[i, :L[i]] += dkb[b, :L[i]]
            else:
                want[b] = float("nan")
                want_len[b] = N
        out[case] = (src, want, want_len, dkb, want_bwd)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_forward_copies_the_live_rows_and_zeroes_the_rest(macx, dev, data, case):
    shape, index, lengths = CASES[case]
    G, B, N, d = shape
    src, want, want_len, _, _ = data[case]
    idx, lens = torch.tensor(index, dtype=torch.int32, device=dev), torch.tensor(lengths, dtype=torch.int32, device=dev)
    rc, kbuf, kb, lbuf, kbl = forward(macx, src.to(dev), idx, lens, shape, dev)
    assert rc == 0 and kbuf.intact() and lbuf.intact()
    assert bits_equal(kb.cpu(), want)                     # +0.0 by bit pattern in the padded rows; NaN only for an index out of range
    assert torch.equal(kbl.cpu(), want_len)
    L = clamp(lengths, N)
    for b, i in enumerate(index):
        if 0 <= i < G:
            assert not bool(torch.isnan(kb[b]).any()), b
            assert bool((kb[b, L[i]:].view(torch.int32) == 0).all()), b
        else:
            assert bool((kb[b].view(torch.int32) == 0x7FC00000).all()) and int(kbl[b]) == N, b


@pytest.mark.parametrize("case", list(CASES))
def test_backward_sums_the_live_rows_and_zeroes_the_rest(macx, dev, data, case):
    shape, index, lengths = CASES[case]
    G, B, N, d = shape
    _, _, _, dkb, want = data[case]
    idx, lens = torch.tensor(index, dtype=torch.int32, device=dev), torch.tensor(lengths, dtype=torch.int32, device=dev)
    rc, buf, got = backward(macx, dkb.to(dev), idx, lens, shape, dev)
    assert rc == 0 and buf.intact()
    assert torch.equal(got.cpu(), want)                   # ascending b, plain fp32 adds: bit for bit; no NaN came through
    L = clamp(lengths, N)
    for i in range(G):
        assert bool((got[i, L[i]:].view(torch.int32) == 0).all()), i
        if i not in index:                                # an image no question names: all zeros, every element written
            assert bool((got[i].view(torch.int32) == 0).all()), i
    if "unnamed" in case:
        assert 1 not in index


@pytest.mark.parametrize("shape, index", [(SMALL, [2, 0, 0, 2, 0]), (EDGE, [1, 0, 2, 2, 1]), (SMALL, [2, -1, 0, 3, 0])])
def test_null_lengths_are_the_plain_gather(macx, dev, shape, index):
    G, B, N, d = shape
    L = macx._lib.lib()
    g = torch.Generator().manual_seed(5)
    src, dkb = torch.randn(G, N, d, generator=g).to(dev), torch.randn(B, N, d, generator=g).to(dev)
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    rc, kbuf, kb, lbuf, kbl = forward(macx, src, idx, None, shape, dev)
    plain = torch.full((B, N, d), float("nan"), device=dev)
    assert rc == 0 and L.macx_kb_gather(ptr(src), ptr(idx), G, B, N, d, ptr(plain), None) == 0
    rc, buf, got = backward(macx, dkb, idx, None, shape, dev)
    plain_bwd = torch.full((G, N, d), float("nan"), device=dev)
    assert rc == 0 and L.macx_kb_gather_bwd(ptr(dkb), ptr(idx), G, B, N, d, ptr(plain_bwd), None) == 0
    torch.cuda.synchronize()
    assert bits_equal(kb, plain) and bits_equal(got, plain_bwd)
    assert kbuf.intact() and buf.intact() and lbuf.intact()
    assert bool((kbl == -7).all())                        # without lengths there are none to hand on


def test_full_lengths_are_the_plain_gather_too(macx, dev):
    G, B, N, d = EDGE
    index = [1, 0, 2, 2, 1]
    g = torch.Generator().manual_seed(6)
    src, dkb = torch.randn(G, N, d, generator=g).to(dev), torch.randn(B, N, d, generator=g).to(dev)
    idx, lens = torch.tensor(index, dtype=torch.int32, device=dev), torch.full((G,), N, dtype=torch.int32, device=dev)
    rc, _, kb, _, kbl = forward(macx, src, idx, lens, EDGE, dev)
    assert rc == 0 and torch.equal(kb, src[idx.long()]) and bool((kbl == N).all())
    rc, _, got = backward(macx, dkb, idx, lens, EDGE, dev)
    want = torch.zeros(G, N, d)
    for b, i in enumerate(index):
        want[i] += dkb[b].cpu()
    assert rc == 0 and torch.equal(got.cpu(), want)


def test_refusals(macx, dev):
    L = macx._lib.lib()
    x, out = torch.zeros(2 * 2 * 6, device=dev), torch.zeros(2 * 2 * 6, device=dev)
    idx, lens, kbl = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in range(3)]
    # N * d = 12 is a multiple of 4, d = 6 is not: a row is no whole number of 16-byte quads
    assert L.macx_kb_gather_l(ptr(x), ptr(idx), ptr(lens), 2, 2, 2, 6, ptr(out), ptr(kbl), None) == macx._lib.MACX_EINVAL
    assert L.macx_kb_gather_bwd_l(ptr(x), ptr(idx), ptr(lens), 2, 2, 2, 6, ptr(out), None) == macx._lib.MACX_EINVAL
    assert L.macx_kb_gather_l(ptr(x), ptr(idx), ptr(lens), 2, 2, 3, 4, ptr(out), None, None) == macx._lib.MACX_EINVAL    # no kb_lengths_out
    assert L.macx_kb_gather_l(ptr(x), ptr(idx), ptr(lens), 0, 2, 3, 4, ptr(out), ptr(kbl), None) == macx._lib.MACX_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0).all())                         # nothing was launched


def test_kb_gather_function_with_lengths(macx, dev):
    """stem.kb_gather(kb_images, index, image_lengths) under autograd: (kb, kb_lengths) and the gradient are the exports'"""
    case = "edge 70/64/65, image 1 unnamed"
    shape, index, lengths = CASES[case]
    G, B, N, d = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(G, N, d, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(B, N, d, generator=g).to(dev)
    idx, lens = torch.tensor(index, dtype=torch.int64, device=dev), torch.tensor(lengths, dtype=torch.int64, device=dev)
    kb, kbl = macx.stem.kb_gather(x, idx, lens)
    assert kbl.dtype == torch.int32 and not kbl.requires_grad
    kb.backward(dout)
    idx32, lens32 = idx.to(torch.int32), lens.to(torch.int32)
    rc, _, want, _, want_len = forward(macx, x.detach(), idx32, lens32, shape, dev)
    rc2, _, want_grad = backward(macx, dout, idx32, lens32, shape, dev)
    assert rc == 0 and rc2 == 0
    assert bits_equal(kb.detach(), want) and torch.equal(kbl, want_len) and bits_equal(x.grad, want_grad)
    assert torch.equal(kbl.cpu(), torch.tensor(clamp(lengths, N), dtype=torch.int32)[torch.tensor(index)])
    assert type(macx.stem.kb_gather(x.detach(), idx32)) is torch.Tensor          # without lengths: the call of before


@pytest.mark.parametrize("N, d", [(2, 4), (2, 6)])
def test_kb_gather_function_without_lengths_is_the_plain_export(macx, dev, N, d):
    """stem.kb_gather(kb_images, index) -- one autograd function on macx_kb_gather_l / _bwd_l with NULL lengths -- against
    macx_kb_gather / macx_kb_gather_bwd called directly: the same bits forward and backward.  The smallest shape with a repeated
    (1) and an unused (0) image; d = 6: N * d % 4 == 0 with d % 4 != 0, which the plain exports take and the call must still take."""
    G, B = 2, 3
    L = macx._lib.lib()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(G, N, d, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(B, N, d, generator=g).to(dev)
    idx = torch.tensor([1, 1, 1], dtype=torch.int32, device=dev)
    kb = macx.stem.kb_gather(x, idx)
    assert type(kb) is torch.Tensor
    kb.backward(dout)
    want, want_grad = torch.full((B, N, d), float("nan"), device=dev), torch.full((G, N, d), float("nan"), device=dev)
    assert L.macx_kb_gather(ptr(x.detach()), ptr(idx), G, B, N, d, ptr(want), None) == 0
    assert L.macx_kb_gather_bwd(ptr(dout), ptr(idx), G, B, N, d, ptr(want_grad), None) == 0
    torch.cuda.synchronize()
    assert bits_equal(kb.detach(), want) and bits_equal(x.grad, want_grad)
    assert bool((x.grad[0].view(torch.int32) == 0).all())
