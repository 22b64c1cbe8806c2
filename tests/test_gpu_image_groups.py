"""-m gpu: questions that share images.  macx_kb_gather / macx_kb_gather_bwd on their own (bit equality with indexing and with an
ascending fp32 loop, guard bands, NaN poison for an index out of range, refusals), `image_index=` on the whole tower in evaluation and
in training with a stem that keeps everything, and `CapturedTowerForward(images=G)` replaying several groupings from one graph.

Shapes of the kernel tests: the smallest legal call (one quad); 5 x 132 = 660 floats per block (165 quads: no multiple of the
256-quad or the 1024-quad chunk) with an unsorted, repeating index that leaves one image out; and the workload's block (196 x 512
floats: 25 forward chunks, 98 backward chunks per block) for B = 64."""
import pytest
import torch

from abi_kit import SENT, Guarded, bits_equal, ptr
from helpers import rel_err, max_abs
from test_gpu_encoder import make_questions

pytestmark = pytest.mark.gpu

GRAD_TOL = 3e-5     # the project's gradient bound (tests/test_gpu_configs.py): relative to each tensor's largest entry
CASES = {"one quad": (1, 1, 1, 4, [0]),
         "odd block, image 3 unused": (4, 7, 5, 132, [2, 0, 0, 1, 2, 2, 0]),
         "workload block": (2, 64, 196, 512, [b % 2 for b in range(64)])}


def gather(macx, src, index, G, B, N, d, dev, bwd=False, fill=None):
    """one call of macx_kb_gather (src [G,N,d] -> [B,N,d]) or macx_kb_gather_bwd (src [B,N,d] -> [G,N,d]) into a guarded output
    (pre-filled with `fill`) -> (return code, the Guarded, the output)"""
    L = macx._lib.lib()
    rows = G if bwd else B
    buf = Guarded(rows * N * d, dev)
    out = buf.view
    if fill is not None:
        out.fill_(fill)
    f = L.macx_kb_gather_bwd if bwd else L.macx_kb_gather
    rc = f(ptr(src), ptr(index), G, B, N, d, ptr(out), None)
    torch.cuda.synchronize()
    return rc, buf, out.view(rows, N, d)


# ---- a. the gather forward on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_gather_forward_equals_indexing(macx, dev, case):
    G, B, N, d, index = CASES[case]
    src = torch.randn(G, N, d, generator=torch.Generator().manual_seed(1)).to(dev)
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    rc, buf, kb = gather(macx, src, idx, G, B, N, d, dev)
    assert rc == 0
    assert torch.equal(kb, src[idx.long()])
    assert buf.intact()                                         # nothing outside kb[0 .. B*N*d) is written
    rc2, _, kb2 = gather(macx, src, idx, G, B, N, d, dev)
    assert rc2 == 0 and bits_equal(kb, kb2)                     # calling twice: identical bits


@pytest.mark.parametrize("case, at, bad", [("one quad", 0, -1), ("one quad", 0, 1), ("odd block, image 3 unused", 3, -1),
                                           ("odd block, image 3 unused", 6, 4), ("workload block", 63, 2)])
def test_gather_forward_poisons_an_index_out_of_range(macx, dev, case, at, bad):
    """an index of -1 or G is not dereferenced: that question's block is all quiet NaN, every other block exact, the call returns 0"""
    G, B, N, d, index = CASES[case]
    index = list(index)
    index[at] = bad
    src = torch.randn(G, N, d, generator=torch.Generator().manual_seed(2)).to(dev)
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    rc, buf, kb = gather(macx, src, idx, G, B, N, d, dev)
    assert rc == 0 and buf.intact()
    assert bool(torch.isnan(kb[at]).all())
    assert bool((kb[at].view(torch.int32) == 0x7FC00000).all())
    others = [b for b in range(B) if b != at]
    if others:
        o = torch.tensor(others, device=dev)
        assert torch.equal(kb[o], src[idx.long()[o]])


# ---- b. the gather backward on its own -----------------------------------------------------------------------------------------
def ascending_sum(dkb, index, G):
    """dkb_images on the CPU: fp32, b ascending, plain IEEE adds"""
    acc = torch.zeros(G, *dkb.shape[1:], dtype=torch.float32)
    for b in range(dkb.shape[0]):
        acc[index[b]] += dkb[b]
    return acc


@pytest.fixture(scope="module")
def backward_cases():
    out = {}
    for case, (G, B, N, d, index) in CASES.items():
        dkb = torch.randn(B, N, d, generator=torch.Generator().manual_seed(3))
        out[case] = (dkb, ascending_sum(dkb, index, G))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_gather_backward_equals_the_ascending_sum(macx, dev, backward_cases, case):
    G, B, N, d, index = CASES[case]
    dkb, want = backward_cases[case]
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    rc, buf, got = gather(macx, dkb.to(dev), idx, G, B, N, d, dev, bwd=True, fill=float("nan"))      # output pre-filled with NaN
    assert rc == 0 and buf.intact()
    assert torch.equal(got.cpu(), want)                         # ascending b, plain fp32 adds: bit for bit
    for g in set(range(G)) - set(index):                        # an image no question names: exactly zero, every element written
        assert bool((got[g].view(torch.int32) == 0).all())
    if case.startswith("odd"):
        assert set(range(G)) - set(index) == {3}
    rc2, _, got2 = gather(macx, dkb.to(dev), idx, G, B, N, d, dev, bwd=True, fill=float("nan"))
    assert rc2 == 0 and bits_equal(got, got2)


@pytest.mark.parametrize("case", ["one quad", "odd block, image 3 unused"])
def test_kb_gather_function_agrees_with_index_select(macx, dev, case):
    """_KBGather against torch.index_select under autograd, fp32.  Outputs are copies: equal.  With one question per image (the
    smallest shape) the gradient is a copy too: equal.  With repeats the two sum the same <= 3 terms per element, possibly in
    another order; either sum is within (n - 1) roundings of 2^-24 relative to sum |terms| of the exact value, so they differ by
    at most 2 (n - 1) 2^-24 sum |terms|, n = 3."""
    G, B, N, d, index = CASES[case]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(G, N, d, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(B, N, d, generator=g).to(dev)
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    y = macx.stem.kb_gather(x, idx)
    y.backward(dout)
    xr = x.detach().clone().requires_grad_(True)
    yr = torch.index_select(xr, 0, idx.long())
    yr.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(y, yr)
    if B == 1:
        assert torch.equal(x.grad, xr.grad)
    else:
        mag = torch.zeros_like(xr).index_add_(0, idx.long(), dout.abs())
        assert bool(((x.grad - xr.grad).abs() <= 2 * 2 * 2.0 ** -24 * mag).all())
        assert bool((x.grad[3] == 0).all())


# ---- c. refusals ---------------------------------------------------------------------------------------------------------------
def test_gather_refusals(macx, dev):
    L = macx._lib.lib()
    EINVAL = macx._lib.MACX_EINVAL
    src, out = torch.zeros(2, 3, 4, device=dev), torch.full((5, 3, 4), SENT, device=dev)
    idx = torch.zeros(5, dtype=torch.int32, device=dev)
    for f in (L.macx_kb_gather, L.macx_kb_gather_bwd):
        assert f(ptr(src), ptr(idx), 2, 5, 3, 2, ptr(out), None) == EINVAL         # N * d = 6: no whole number of 16-byte quads
        assert f(ptr(src), ptr(idx), 0, 5, 3, 4, ptr(out), None) == EINVAL         # G = 0
        assert f(ptr(src), ptr(idx), 2, 0, 3, 4, ptr(out), None) == EINVAL
        assert f(None, ptr(idx), 2, 5, 3, 4, ptr(out), None) == EINVAL            # a null pointer, each of the three
        assert f(ptr(src), None, 2, 5, 3, 4, ptr(out), None) == EINVAL
        assert f(ptr(src), ptr(idx), 2, 5, 3, 4, None, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                        # nothing was launched
    assert L.macx_kb_gather(ptr(src), ptr(idx), 2, 5, 3, 4, ptr(out), None) == 0   # (the legal call of the same buffers)
    torch.cuda.synchronize()
    assert torch.equal(out, src[idx.long()])


# ---- d, e. the tower ----------------------------------------------------------------------------------------------------------
B, G, H, W, CIN, D, P, S, A, V, E = 6, 3, 4, 3, 128, 256, 2, 6, 7, 12, 20
INDEX = [1, 1, 0, 2, 0, 1]


def make_net(macx, dev, **over):
    """the net of test_gpu_encoder.py::test_full_tower_ids_to_logits_gradients"""
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D, encDim=D, wrdEmbDim=E, outClassifierDims=[32],
                                        answerWordsNum=A)
    cfg.stemDim = 128
    for k, v in over.items():
        setattr(cfg, k, v)
    return macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=CIN, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)


def tower_inputs(dev, seed=6):
    img = torch.relu(torch.randn(G, H * W, CIN, generator=torch.Generator().manual_seed(seed)))
    q, lengths = make_questions(B, S, V, seed=3, min_len=2)
    return img.to(dev), q.to(dev), lengths.to(dev), torch.tensor(INDEX, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("stem", ["fused", "generic"])
def test_tower_eval_with_shared_images(macx, dev, stem):
    """net(images_g, q, len, image_index=idx) against (1) the decomposition by hand on the same modules, the stem's output indexed
    by torch: logits and every kb attention bit for bit; (2) the duplicated run net(images_g[idx], q, len): bit for bit as well.
    Why (2) can be exact: a row of the stem's output is one MFMA dot product over its own receptive field; the general convolution
    (generic stem) is exact fp32, and the fused stem's fp16-plane kernels share one exponent per operand TENSOR, taken from its
    largest magnitude -- the same in both runs as long as every image is named by some question, which INDEX does.  (An unused
    image holding the batch's largest feature would move that exponent; the bound then is the project's logits criterion.)
    The logits criterion, <= 1e-4 with identical argmax, is asserted besides."""
    net = make_net(macx, dev, **({"stemKernelSize": 1} if stem == "generic" else {}))
    assert type(net.stem) is (macx.GenericStem if stem == "generic" else macx.Stem)
    cfg = net.config
    images, q, lengths, idx = tower_inputs(dev)
    with torch.no_grad():
        logits = net(images, q, lengths, image_index=idx, check_index=True).clone()
        att = [a.clone() for a in net.last_cell.attentions["kb"]]
        # (1) by hand
        words, vecQ = net.enc(q, lengths)
        kb = net.stem(images)[idx.long()].contiguous()
        cell = macx.MACCell(vecQuestions=vecQ, questionWords=words, questionCntxWords=words, questionLengths=lengths, knowledgeBase=kb,
                            memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout, batchSize=B,
                            train=False, config=cfg, params=net.cell, netLength=P)
        hand = net.out(cell.run().memory, vecQ).clone()
        hand_att = [a.clone() for a in cell.attentions["kb"]]
        # (2) duplicated
        dup = net(images[idx.long()].contiguous(), q, lengths).clone()
        dup_att = [a.clone() for a in net.last_cell.attentions["kb"]]
    torch.cuda.synchronize()
    assert logits.shape == (B, A) and bool(torch.isfinite(logits).all())
    assert torch.equal(logits, hand)
    assert len(att) == P and all(torch.equal(a, b) for a, b in zip(att, hand_att))
    print("grouped vs duplicated: max |d logits| = %.3e" % max_abs(logits, dup))
    assert max_abs(logits, dup) <= 1e-4 and torch.equal(logits.argmax(1), dup.argmax(1))
    assert torch.equal(logits, dup)
    assert all(torch.equal(a, b) for a, b in zip(att, dup_att))
    # questions 0, 1 and 5 look at the same image with different words: the index, not the position, selects the block
    assert not torch.equal(logits[0], logits[1])


def test_tower_eval_with_shared_images_takes_the_feed_dict_layout(macx, dev):
    net = make_net(macx, dev)
    images, q, lengths, idx = tower_inputs(dev)
    nchw = images.reshape(G, H, W, CIN).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        a = net(images, q, lengths, image_index=idx).clone()
        b = net(nchw, q, lengths, image_index=idx.long()).clone()          # [G, C, H, W], and an int64 index
    assert torch.equal(a, b)
    with pytest.raises(IndexError):
        net(images, q, lengths, image_index=idx + 1, check_index=True)


def test_tower_train_with_shared_images(macx, dev):
    """train=True with stemDropout = 1.0, fixed seed, CE loss: every parameter gradient of the grouped run against the duplicated
    run.  The stem's gradients see another sum order over the questions (the gather's backward adds the questions of an image
    first): GRAD_TOL = 3e-5 of each tensor's maximum.  Encoder, cell and classifier gradients: bit for bit, as the knowledge base is
    (test_tower_eval_with_shared_images)."""
    net = make_net(macx, dev, stemDropout=1.0)
    images, q, lengths, idx = tower_inputs(dev)
    ans = torch.tensor([1, 5, 2, 0, 6, 3], device=dev)

    def run(images, **kw):
        for t in net.tensors():
            t.grad = None
        logits = net(images, q, lengths, train=True, seed=21, **kw)
        loss, _ = net.loss_and_pred(logits, ans)
        loss.backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), float(loss.detach()), [None if t.grad is None else t.grad.clone() for t in net.tensors()]

    lg, loss_g, grads_g = run(images, image_index=idx)
    ld, loss_d, grads_d = run(images[idx.long()].contiguous())
    assert torch.equal(lg, ld) and loss_g == loss_d
    stem_ids = {id(t) for t in net.stem.tensors()}
    names = {id(t): "%s[%d]" % (m, i) for m in ("enc", "stem", "cell", "out") for i, t in enumerate(getattr(net, m).tensors())}
    bad = {}
    for t, a, b in zip(net.tensors(), grads_g, grads_d):
        assert (a is None) == (b is None), names[id(t)]
        if a is None:                                           # (a parameter this option set does not use)
            continue
        if id(t) in stem_ids:
            assert float(b.abs().max()) > 0, names[id(t)]
            e = rel_err(a, b)
            print("%s: grouped vs duplicated gradient, relative to the maximum: %.3e" % (names[id(t)], e))
            if not e < GRAD_TOL:
                bad[names[id(t)]] = e
        elif not torch.equal(a, b):
            bad[names[id(t)]] = rel_err(a, b)
    assert not bad, bad
    assert len(stem_ids) == 4


# ---- f. captured ---------------------------------------------------------------------------------------------------------------
def test_captured_tower_forward_with_shared_images(macx, dev):
    net = make_net(macx, dev)
    fwd = macx.CapturedTowerForward(net, B=B, S=S, H=H, W=W, imageInDim=CIN, images=G)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    assert fwd.images.shape == (G, H * W, CIN) and fwd.image_index.shape == (B,) and fwd.image_index.dtype == torch.int32
    graph = fwd.graph
    seen = []
    for seed, index in ((6, INDEX), (7, [2, 2, 2, 0, 0, 2])):              # two groupings (the second leaves image 1 out), one graph
        images, q, lengths, _ = tower_inputs(dev, seed=seed)
        idx = torch.tensor(index, dtype=torch.int32, device=dev)
        with torch.no_grad():
            ref = net(images, q, lengths, image_index=idx).clone()
            att_kb = [a.clone() for a in net.last_cell.attentions["kb"]]
            att_q = [a.clone() for a in net.last_cell.attentions["question"]]
        got = fwd(images, q, lengths, image_index=idx)
        torch.cuda.synchronize()
        assert fwd.graph is graph and fwd.captured
        assert bits_equal(got, ref)
        assert torch.equal(fwd.pred.long(), ref.argmax(dim=1))
        assert len(fwd.attentions["kb"]) == P and all(bits_equal(a, b) for a, b in zip(att_kb, fwd.attentions["kb"]))
        assert all(bits_equal(a, b) for a, b in zip(att_q, fwd.attentions["question"]))
        seen.append(ref)
    assert not torch.equal(seen[0], seen[1])
    fwd.check()
    with pytest.raises(ValueError, match="image_index"):
        fwd.load(images, q, lengths)
    with pytest.raises(IndexError):
        fwd.load(images, q, lengths, image_index=idx + 1)
    plain = macx.CapturedTowerForward(net, B=B, S=S, H=H, W=W, imageInDim=CIN)
    assert plain.captured and plain.images.shape[0] == B
    with pytest.raises(ValueError, match="image_index"):
        plain.load(images[idx.long()], q, lengths, image_index=idx)
