"""The whole tower from one HIP graph (macx.CapturedTowerForward / CapturedTowerTrainStep) and what it stands on: the encoder's,
the stem's and the output unit's entry points under a run's mask word (macx_*_w), the optimizer step with its rate in device memory
(macx_adam_ema_step_p) and the one-launch gradient gather (macx_gather_flat).  Everything here is an equality of bits, except the
kept fraction of one dropout site (a 4 sigma binomial bound).

Shapes: the smallest that reach every tail -- B = 6 (half-empty question block of the LSTM step), S = 7 with lengths 7 (full) and 1,
5 x 5 cells (N = 25: no multiple of 16 or 64, >= 16 as the H2 chain needs), d = 256 (h = 128, the fused encoder's minimum),
wrdEmbDim = 20 (padded embedding columns), 28 answers (padded to 32), p = 3."""
import math

import numpy as np
import pytest
import torch

from abi_kit import bits_equal, ptr
from oracle import dropout_hash as dh

pytestmark = pytest.mark.gpu

B, S, H, W, CIN, D, E, VOCAB, P, ANSWERS = 6, 7, 5, 5, 128, 256, 20, 11, 3, 28
LENGTHS = [7, 1, 3, 7, 5, 2]
SITE_FC0, SITE_ENC_INPUT, SITE_QUESTION = 7, 11, 12


def config(macx, **over):
    return macx.configs.flag_file_config("args", **dict(dict(netLength=P, memDim=D, ctrlDim=D, attDim=D, encDim=D, wrdEmbDim=E,
                                                             outClassifierDims=[128]), **over))


def make_net(macx, dev, seed=0, cfg=None, **kw):
    kw = dict(dict(vocab=VOCAB, H=H, W=W, imageInDim=CIN, answerWordsNum=ANSWERS), **kw)
    return macx.MACNet(cfg if cfg is not None else config(macx), generator=torch.Generator().manual_seed(seed), **kw).to(dev)


def inputs(dev, seed, b=B, s=S, lengths=LENGTHS, hw=H * W, cin=CIN, vocab=VOCAB):
    g = torch.Generator().manual_seed(seed)
    images = torch.relu(torch.randn(b, hw, cin, generator=g))
    lengths = torch.tensor(lengths, dtype=torch.int32)
    q = torch.randint(1, vocab + 1, (b, s), generator=g, dtype=torch.int32)
    q = q * (torch.arange(s).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)
    ans = torch.randint(0, ANSWERS, (b,), generator=g, dtype=torch.int32)
    return images.to(dev), q.to(dev), lengths.to(dev), ans.to(dev)


def word_tensor(dev, word):
    word &= 0xFFFFFFFF
    return torch.tensor([word - (1 << 32) if word >= (1 << 31) else word], dtype=torch.int32, device=dev)


# ---- one (outputs, gradients) run per module: `call(**kw)` runs the module with the same inputs, seed and output gradient --------
def module_runner(macx, dev, name):
    net = make_net(macx, dev, seed=3)
    images, q, lengths, _ = inputs(dev, 5)
    g = torch.Generator().manual_seed(9)
    mod = {"enc": net.enc, "stem": net.stem, "out": net.out}[name]
    if name == "enc":
        args, douts = (q, lengths), [torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, D, generator=g).to(dev)]
    elif name == "stem":
        args, douts = (images,), [torch.randn(B, H * W, D, generator=g).to(dev)]
    else:
        args = (torch.randn(B, D, generator=g).to(dev).requires_grad_(True), torch.randn(B, D, generator=g).to(dev).requires_grad_(True))
        douts = [torch.randn(B, ANSWERS, generator=g).to(dev)]

    def call(scale=1.0, train=True, **kw):
        leaves = list(mod.tensors()) + [a for a in args if a.is_floating_point() and a.requires_grad]
        for t in leaves:
            t.grad = None
        outs = mod(*args, train=train, seed=77, b0=2, **kw)
        outs = list(outs) if isinstance(outs, tuple) else [outs]
        torch.autograd.backward(outs, [d * scale for d in douts])
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], [t.grad.clone() for t in leaves]

    return call, args


@pytest.mark.parametrize("name", ["enc", "stem", "out"])
def test_w_entry_points(macx, dev, name):
    call, _ = module_runner(macx, dev, name)
    same = lambda x, y: all(bits_equal(a, b) for a, b in zip(x[0] + x[1], y[0] + y[1]))
    old = call()                                           # the old path: the keyword is not passed
    assert same(old, call(mask_word=None))
    assert same(old, call(mask_word=word_tensor(dev, 0)))  # the _w entry points on a word of 0: the plain seed's masks
    w1, w2 = word_tensor(dev, 0x9E3779B9), word_tensor(dev, 0xC0FFEE11)
    r1 = call(mask_word=w1)
    assert same(r1, call(mask_word=w1))                    # same word, same masks
    r2 = call(mask_word=w2)
    assert not bits_equal(r1[0][-1], r2[0][-1]) and not bits_equal(old[0][-1], r1[0][-1])      # other word, other masks
    # the word is read when the kernel runs: rewriting the SAME tensor changes the masks of the next call
    w1.copy_(w2)
    assert same(r2, call(mask_word=w1))
    # for fixed masks the module is linear in the output gradient: a backward pass that hashed with another word than the forward
    # pass would not be (the activation gradient sits behind other masks), and doubling is exact in binary floating point
    r2x = call(scale=2.0, mask_word=w2)
    assert all(bits_equal(a, b) for a, b in zip(r2[0], r2x[0]))
    assert all(bits_equal(2.0 * a, b) for a, b in zip(r2[1], r2x[1]))
    # evaluation ignores the word (keep = 1 everywhere)
    assert all(bits_equal(a, b) for a, b in zip(call(train=False)[0], call(train=False, mask_word=w2)[0]))


def test_w_masks_are_those_of_seed_and_word(macx, dev):
    """Against the mask definition itself (oracle.dropout_hash, site key XOR word): vecQuestions is zero exactly where the question
    dropout's mask of (seed, word) is, the embedding gradient where the input dropout's mask is (every token once), and the output
    unit's d_memory where the first classifier layer's input mask is."""
    word = 0x5BD1E995
    wt = word_tensor(dev, word)
    net = make_net(macx, dev, seed=3)
    with torch.no_grad():                         # (zero LSTM biases would leave the final state of an all-pad question exactly 0)
        for bias in (net.enc.fw_bias, net.enc.bw_bias):
            bias.copy_(0.1 * torch.randn(bias.shape, generator=torch.Generator().manual_seed(12)))
    _, _, lengths, _ = inputs(dev, 5)
    q = torch.zeros(B, S, dtype=torch.int32)
    q.view(-1)[:7] = torch.arange(1, 8, dtype=torch.int32)            # question 0: ids 1..7
    q[1, 0] = 8
    q[2, :3] = torch.tensor([9, 10, 11], dtype=torch.int32)           # every id once; the other questions hold id 0 (the zero row)
    q = q.to(dev)
    words, vecQ = net.enc(q, lengths, train=True, seed=77, b0=2, mask_word=wt)
    g = torch.Generator().manual_seed(1)
    torch.autograd.backward([words, vecQ], [torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, D, generator=g).to(dev)])
    torch.cuda.synchronize()
    mq = dh.mask_for(77, SITE_QUESTION, 0, net.enc.keep_q, (B, D), b0=2, word=word)
    assert np.array_equal(vecQ.detach().cpu().numpy() != 0, mq != 0)
    assert not np.array_equal(mq, dh.mask_for(77, SITE_QUESTION, 0, net.enc.keep_q, (B, D), b0=2, word=0))
    mi = dh.mask_for(77, SITE_ENC_INPUT, 0, net.enc.keep_in, (B, S, E), b0=2, word=word)
    demb = net.enc.emb.grad.cpu().numpy()
    for b, s in [(0, k) for k in range(7)] + [(1, 0)] + [(2, k) for k in range(3)]:
        v = int(q[b, s])
        assert np.array_equal(demb[v - 1] != 0, mi[b, s] != 0), (b, s)
    mem = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    logits = net.out(mem, vecQ.detach(), train=True, seed=77, b0=2, mask_word=wt)
    logits.backward(torch.randn(B, ANSWERS, generator=g).to(dev))
    torch.cuda.synchronize()
    m0 = dh.mask_for(77, SITE_FC0, 0, net.out.keep, (B, 2 * D), b0=2, word=word)[:, :D]
    assert np.array_equal(mem.grad.cpu().numpy() != 0, m0 != 0)


def test_question_dropout_keeps_its_fraction_under_a_word(macx, dev):
    b = 64
    net = make_net(macx, dev, seed=3)
    g = torch.Generator().manual_seed(2)
    lengths = torch.randint(1, S + 1, (b,), generator=g, dtype=torch.int32)
    q = torch.randint(1, VOCAB + 1, (b, S), generator=g, dtype=torch.int32)
    q = (q * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)).to(dev)
    with torch.no_grad():
        _, vecQ = net.enc(q, lengths.to(dev), train=True, seed=123, mask_word=word_tensor(dev, 0x1234ABCD))
    n, drop = vecQ.numel(), 1.0 - net.enc.keep_q
    zeros = float((vecQ == 0).sum()) / n
    sigma = math.sqrt(drop * (1.0 - drop) / n)
    print("zero fraction %.5f, expected %.5f, sigma %.5f" % (zeros, drop, sigma))
    assert abs(zeros - drop) < 4 * sigma


def test_adam_step_with_the_rate_in_device_memory(macx, dev):
    L = macx._lib.lib()
    n, b1, b2, eps, clip, decay = 1003, 0.9, 0.999, 1e-8, 8.0, 0.999
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    state = [[p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), p0.clone().to(dev),
              torch.empty(1024, device=dev), torch.zeros(1, device=dev)] for _ in range(2)]
    lr_t = torch.zeros(1, device=dev)
    lr, norms = 1e-2, []
    for t, scale in enumerate([1.0, 0.1, 1.0, 0.1, 0.5], start=1):       # ||g|| ~ 31.7 * scale: clipped at 8 on steps 1, 3, 5
        if t == 3:
            lr = 0.5e-2
        grad = (torch.randn(n, generator=g) * scale).to(dev)
        a, b = state
        macx._lib.check(L.macx_adam_ema_step(n, ptr(a[0]), ptr(grad), ptr(a[1]), ptr(a[2]), ptr(a[3]), lr, b1, b2, eps, t, clip, decay, ptr(a[4]),
                                             ptr(a[5]), None), "macx_adam_ema_step")
        lr_t.fill_(macx.optim.FlatAdamEMA.bias_corrected_lr(lr, b1, b2, t))
        macx._lib.check(L.macx_adam_ema_step_p(n, ptr(b[0]), ptr(grad), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(lr_t), b1, b2, eps, clip, decay,
                                               ptr(b[4]), ptr(b[5]), None), "macx_adam_ema_step_p")
        torch.cuda.synchronize()
        for i, what in enumerate(("params", "m", "v", "ema")):
            assert bits_equal(a[i], b[i]), (t, what)
        assert bits_equal(a[5], b[5]), (t, "norm")
        norms.append(float(a[5]))
    assert min(norms) < clip < max(norms)                                # both sides of the clip were stepped
    assert not torch.equal(state[0][0].cpu(), p0)


def test_gather_flat(macx, dev):
    L = macx._lib.lib()
    sizes = [1, 3, 4, 1021, 4096, 130]
    offsets, off = [], 0
    for k in sizes:
        offsets.append(off)
        off += (k + 3) & ~3
    g = torch.Generator().manual_seed(6)
    pool = torch.randn(sum(sizes) + 64, generator=g).to(dev)
    srcs, at = [], 0
    for i, k in enumerate(sizes):
        lo = at + (1 if i == 3 else 0)            # the 1021-float source starts 4 bytes off a 16-byte boundary: the scalar path
        srcs.append(pool[lo:lo + k])
        at += (k + 3) & ~3
    srcs[2] = None                                # a parameter that got no gradient: zero-filled
    assert srcs[3].data_ptr() % 16 == 4 and srcs[4].data_ptr() % 16 == 0
    sentinel = -12345.0
    want = torch.full((off + 8,), sentinel, device=dev)
    for s, o, k in zip(srcs, offsets, sizes):
        if s is None:
            want[o:o + k].zero_()
        else:
            want[o:o + k].copy_(s)
    rows = [x for s, o, k in zip(srcs, offsets, sizes) for x in (0 if s is None else s.data_ptr(), o, k)]
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    flat = torch.full((off + 8,), sentinel, device=dev)
    macx._lib.check(L.macx_gather_flat(ptr(table), len(sizes), ptr(flat), None), "macx_gather_flat")
    torch.cuda.synchronize()
    assert bits_equal(flat, want)                 # slices, the zero slice and every pad float (still the sentinel)
    pads = torch.ones(off + 8, dtype=torch.bool)
    for o, k in zip(offsets, sizes):
        pads[o:o + k] = False
    assert int(pads.sum()) == 3 + 1 + 3 + 2 + 8 and bool((flat.cpu()[pads] == sentinel).all())
    assert bool((flat[offsets[2]:offsets[2] + 4] == 0).all())


def test_captured_tower_forward_equals_eager(macx, dev):
    net = make_net(macx, dev)
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)

    def eager(images, q, lengths):
        with torch.no_grad():
            logits = net(images, q, lengths, train=False)
            return logits.clone(), [a.clone() for a in net.last_cell.attentions["kb"]], [a.clone() for a in net.last_cell.attentions["question"]]

    for seed in (1, 2, 3):
        images, q, lengths, _ = inputs(dev, seed)
        ref, att_kb, att_q = eager(images, q, lengths)
        got = fwd(images, q, lengths)
        torch.cuda.synchronize()
        assert bits_equal(ref, got)
        assert torch.equal(fwd.pred.long(), ref.argmax(dim=1))
        assert len(fwd.attentions["kb"]) == P and all(bits_equal(a, b) for a, b in zip(att_kb, fwd.attentions["kb"]))
        assert all(bits_equal(a, b) for a, b in zip(att_q, fwd.attentions["question"]))
    # parameters are read at replay time: one optimizer step between two calls
    opt = macx.optim.FlatAdamEMA(net.tensors(), lr=1e-2)
    # (re-pointing the parameters at the optimizer's flat buffer changes their storage: a new capture, as the class says)
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN)
    before = fwd(images, q, lengths).clone()
    assert bits_equal(before, ref)
    opt.step(flat_grad=torch.randn(opt.flat.numel(), generator=torch.Generator().manual_seed(8)).to(dev))
    ref2, att_kb, _ = eager(images, q, lengths)
    got2 = fwd.replay()
    torch.cuda.synchronize()
    assert bits_equal(ref2, got2) and not bits_equal(ref2, before)
    assert all(bits_equal(a, b) for a, b in zip(att_kb, fwd.attentions["kb"]))
    fwd.check()
    with pytest.raises(IndexError):
        fwd.load(images, q + VOCAB + 1, lengths)
    with pytest.raises(ValueError):
        fwd.load(images, q, lengths + S)


@pytest.fixture(scope="module")
def tower_step(macx, dev):
    """ONE captured step for the tests below (and the optimizer's state around its construction)"""
    net = make_net(macx, dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
    before = [b.clone() for b in (opt.flat, opt.m, opt.v, opt.ema)]
    step = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, H=H, W=W, imageInDim=CIN, seed=1234)
    torch.cuda.synchronize()
    untouched = [bits_equal(a, b) for a, b in zip(before, (opt.flat, opt.m, opt.v, opt.ema))] + [opt.t == 0]
    return net, bucket, opt, step, untouched


def test_constructing_a_captured_step_trains_nothing(tower_step):
    _, _, _, step, untouched = tower_step
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert untouched == [True] * 5, dict(zip(("params", "m", "v", "ema", "t"), untouched))


def test_captured_tower_train_step_equals_eager(macx, dev, tower_step):
    net, bucket, opt, step, _ = tower_step
    assert step.captured
    state = step._state()
    ref = make_net(macx, dev)                              # identically initialised
    rbucket = macx.dp.TowerBuckets(ref)                    # per-tensor copy_ gather
    ropt = macx.optim.FlatAdamEMA(rbucket.tensors(), lr=1e-3)
    assert bits_equal(ropt.flat, opt.flat)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    try:
        for it in range(3):
            images, q, lengths, ans = inputs(dev, 20 + it)
            if it == 2:
                opt.lr = ropt.lr = 0.5e-3                  # the captured optimizer follows a changed rate
            step.load(images, q, lengths, ans)
            step.replay(iteration=it)
            word.copy_(word_tensor(dev, macx.graph.mix32(it)))
            for t in ref.tensors():
                t.grad = None
            logits = ref(images, q, lengths, train=True, seed=1234, check_ids=False, mask_word=word)
            loss, pred = ref.loss_and_pred(logits, ans)
            rbucket.begin_step(B, B)
            loss.backward()
            rbucket.allreduce_(B, B)
            norm = ropt.step(flat_grad=rbucket.flat)
            torch.cuda.synchronize()
            pairs = {"loss": (step.loss, loss.detach()), "logits": (step.logits, logits.detach()), "pred": (step.pred, pred),
                     "norm": (step.norm, norm), "flat gradient": (bucket.flat, rbucket.flat), "m": (opt.m, ropt.m), "v": (opt.v, ropt.v),
                     "ema": (opt.ema, ropt.ema), "flat parameters": (opt.flat, ropt.flat)}
            for what, (a, b) in pairs.items():
                assert bits_equal(a.reshape(-1), b.reshape(-1)), (it, what)
            for i, (a, b) in enumerate(zip(net.tensors(), ref.tensors())):
                assert bits_equal(a.detach(), b.detach()), (it, "parameter", i)
            assert opt.t == ropt.t == it + 1
            assert math.isfinite(float(loss)) and float(norm) > 0
        step.check()
    finally:
        opt.lr = 1e-3
        step._restore(state)


def test_captured_tower_train_step_draws_fresh_masks(dev, tower_step):
    _, _, _, step, _ = tower_step
    assert step.captured
    state = step._state()
    try:
        step.load(*inputs(dev, 31))
        losses = []
        for it in (5, 5, 6):
            step._restore(state)
            step.replay(iteration=it)
            losses.append(float(step.loss))
        assert losses[0] == losses[1] and losses[0] != losses[2], losses
    finally:
        step._restore(state)


def test_captured_tower_train_step_at_the_workload_shape(macx, dev):
    b, s, hw, cin, d, p, vocab = 64, 50, 14, 1024, 512, 12, 90
    cfg = macx.configs.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d)
    net = macx.MACNet(cfg, vocab=vocab, generator=torch.Generator().manual_seed(0)).to(dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, b, s, H=hw, W=hw, imageInDim=cin, seed=7, verify=True)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(3, s + 1, (b,), generator=g, dtype=torch.int32).tolist()
    step.load(*inputs(dev, 3, b=b, s=s, lengths=lengths, hw=hw * hw, cin=cin, vocab=vocab))
    loss = step.replay(iteration=0)
    step.check()
    assert math.isfinite(float(loss)) and math.isfinite(float(step.norm)) and opt.t == 1
    assert step.logits.shape == (b, 28) and step.pred.shape == (b,)
