"""-m gpu: knowledge-base sizes and image groups on the captured paths.  `kb_lengths=True` on CapturedForward / CapturedTrainStep /
CapturedDPTrainStep, `kb_lengths=True`, `images=G` and `image_lengths=True` on the tower's classes, and the read unit's export with
lengths (macx_read_fwd_l).  Everything here is an equality of bits with the eager calls, which tests/test_gpu_kb_lengths.py and
tests/test_gpu_image_groups.py pin to the oracle -- plus exact zeros where a question's knowledge base ends.

Cell shapes (B, S, N, d, p): (3, 5, 20, 128, 2), the flag file's cell at its smallest width, and (2, 5, 49, 256, 2), which runs the
H2 chain kernels.  Tower: B = 6, S = 7, 5 x 5 cells, 128 input channels, d = 256, p = 3 (tests/test_gpu_tower_graph.py's net)."""
import ctypes as C
import math

import pytest
import torch

import abi_kit
from abi_kit import bits_equal, ptr

pytestmark = pytest.mark.gpu

CELL_SHAPES = [(3, 5, 20, 128, 2), (2, 5, 49, 256, 2)]
# two sets of sizes per shape: N, 1 and one in between; then others, so that a replay has to read them again
SIZES = {20: ([7, 20, 1], [20, 3, 12]), 49: ([1, 30], [49, 17])}


def cell_setup(macx, dev, shape):
    B, S, N, d, p = shape
    cfg = macx.configs.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d)
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(0)).to(dev)
    x = [t.to(dev) for t in macx.configs.synthetic_inputs(B, S, N, d, seed=1)]
    sizes = [torch.tensor(s, dtype=torch.int32, device=dev) for s in SIZES[N]]
    return cfg, params, x, sizes


def padded_are_zero(t, sizes):
    """t[b, sizes[b]:] is +0.0 by bit pattern for every question"""
    return all(bool((t[b, int(n):].contiguous().view(torch.int32) == 0).all()) for b, n in enumerate(sizes))


# ---- the cell's captured classes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_captured_forward_reads_the_lengths_when_it_runs(macx, dev, shape):
    B, S, N, d, p = shape
    cfg, params, (vq, words, lengths, kb), (first, second) = cell_setup(macx, dev, shape)
    cap = macx.CapturedForward(cfg, params, B, S, N, kb_lengths=True)
    assert cap.captured, "the capture's self-check failed in this process: %r" % (cap.verify_report,)
    assert cap.kb_lengths.dtype == torch.int32 and cap.kb_lengths.shape == (B,)

    def eager(sizes):
        with torch.no_grad():
            cell = macx.MACCell(vq, words, words, lengths, kb, 1.0, 1.0, 1.0, B, False, config=cfg, params=params, kb_lengths=sizes)
            return cell.run().memory.clone(), [a.clone() for a in cell.attentions["kb"]]

    want, want_att = eager(first)
    got = cap(vq, words, lengths, kb, kb_lengths=first).clone()
    got_att = [a.clone() for a in cap.attentions["kb"]]
    torch.cuda.synchronize()
    assert bits_equal(got, want) and len(got_att) == p and all(bits_equal(a, b) for a, b in zip(got_att, want_att))
    assert all(padded_are_zero(a, first) for a in got_att)
    # other lengths written into the static tensor, nothing else: the replay follows them
    cap.kb_lengths.copy_(second)
    got2 = cap.replay().clone()
    want2, want_att2 = eager(second)
    torch.cuda.synchronize()
    assert bits_equal(got2, want2) and all(bits_equal(a, b) for a, b in zip(cap.attentions["kb"], want_att2))
    assert all(padded_are_zero(a, second) for a in cap.attentions["kb"])
    assert not bits_equal(got2, got)
    cap.check()
    with pytest.raises(TypeError, match="kb_lengths"):
        cap.load(vq, words, lengths, kb)
    with pytest.raises(ValueError, match="kb_lengths"):
        cap.load(vq, words, lengths, kb, kb_lengths=second + N)


@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_captured_train_step_with_lengths_equals_eager(macx, dev, shape):
    B, S, N, d, p = shape
    cfg, params, (vq, words, lengths, kb), sizes = cell_setup(macx, dev, shape)
    gm = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(dev)
    step = macx.CapturedTrainStep(cfg, params, B, S, N, seed=77, kb_lengths=True)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    step.load(vq, words, lengths, kb, gm, kb_lengths=sizes[0])
    mems = []
    for it, L in enumerate(sizes):
        step.kb_lengths.copy_(L)
        mem = step.replay(iteration=it).clone()
        got = [t.grad.clone() for t in step._leaves()]
        # the eager step by hand, on copies of the inputs, under the same seed and mask word
        vq2, w2, kb2 = [t.detach().clone().requires_grad_(True) for t in (vq, words, kb)]
        captured_grads = [t.grad for t in params.tensors()]          # the tensors the graph writes: put back below
        for t in params.tensors():
            t.grad = None
        cell = macx.MACCell(vq2, w2, w2, lengths, kb2, cfg.memoryDropout, cfg.readDropout, cfg.writeDropout, B, True, config=cfg,
                            params=params, seed=77, mask_word=step.mask_word, kb_lengths=L)
        st = cell.run()
        torch.autograd.backward([st.memory], [gm])
        torch.cuda.synchronize()
        want = [vq2.grad, w2.grad, kb2.grad] + [t.grad for t in params.tensors()]
        assert bits_equal(mem, st.memory.detach())
        assert len(got) == len(want) == 3 + len(params.tensors())
        for i, (a, b) in enumerate(zip(got, want)):
            assert bits_equal(a, b), (it, i)
        assert padded_are_zero(got[2], L)                 # knowledgeBase.grad behind each question's size
        assert bool((got[2][0, 0] != 0).any())
        for t, g in zip(params.tensors(), captured_grads):
            t.grad = g
        mems.append(mem)
    assert not bits_equal(mems[0], mems[1])
    step.check()


def test_captured_dp_step_with_lengths_equals_its_uncaptured_run(macx, dev):
    """one process, no process group, GradBucket over the parameters' flat buffer, global_batch = B: the two graph replays give the
    flat gradient, the memory and the input gradients of the same class issuing its launches one by one"""
    shape = CELL_SHAPES[0]
    B, S, N, d, p = shape
    cfg, params, (vq, words, lengths, kb), sizes = cell_setup(macx, dev, shape)
    params.requires_grad_(True)
    gm = torch.randn(B, d, generator=torch.Generator().manual_seed(3)).to(dev)
    bucket = macx.dp.GradBucket(params.tensors(), params=params)
    seen = {}
    for capture in (True, False):
        step = macx.CapturedDPTrainStep(cfg, params, bucket, B=B, S=S, N=N, global_batch=B, seed=11, capture=capture, kb_lengths=True)
        assert step.captured == capture
        step.load(vq, words, lengths, kb, gm, kb_lengths=sizes[0])
        for it, L in enumerate(sizes):
            step.kb_lengths.copy_(L)
            mem = step.step(iteration=it)
            torch.cuda.synchronize()
            assert all(t.grad is not None and t.grad.data_ptr() >= bucket.flat.data_ptr() for t in params.tensors())
            seen[(capture, it)] = [bucket.flat.clone(), mem.clone(), step.d_vecQuestions.clone(), step.d_words.clone(),
                                   step.d_knowledgeBase.clone()]
            assert padded_are_zero(seen[(capture, it)][4], L)
        step.check()
        with pytest.raises(TypeError, match="kb_lengths"):
            step.load(vq, words, lengths, kb, gm)
        for t in params.tensors():
            t.grad = None
        del step
    for it in range(len(sizes)):
        for i, (a, b) in enumerate(zip(seen[(True, it)], seen[(False, it)])):
            assert bits_equal(a, b), (it, i)
        assert bool(torch.isfinite(seen[(True, it)][0]).all()) and float(seen[(True, it)][0].abs().max()) > 0
    assert not bits_equal(seen[(True, 0)][0], seen[(True, 1)][0])


def test_classes_built_without_lengths_refuse_them(macx, dev):
    shape = CELL_SHAPES[0]
    B, S, N, d, p = shape
    cfg, params, (vq, words, lengths, kb), sizes = cell_setup(macx, dev, shape)
    gm = torch.zeros(B, d, device=dev)
    cap = macx.CapturedForward(cfg, params, B, S, N, warmup=1, verify=False)
    assert cap.kb_lengths is None
    with pytest.raises(TypeError, match="kb_lengths"):
        cap.load(vq, words, lengths, kb, kb_lengths=sizes[0])
    with pytest.raises(TypeError, match="kb_lengths"):
        cap(vq, words, lengths, kb, kb_lengths=sizes[0])
    step = macx.CapturedTrainStep(cfg, params, B, S, N, seed=1, warmup=1, verify=False)
    with pytest.raises(TypeError, match="kb_lengths"):
        step.load(vq, words, lengths, kb, gm, kb_lengths=sizes[0])
    for t in params.tensors():
        t.grad = None
    params.requires_grad_(True)
    bucket = macx.dp.GradBucket(params.tensors(), params=params)
    dp = macx.CapturedDPTrainStep(cfg, params, bucket, B=B, S=S, N=N, global_batch=B, seed=1, warmup=1, capture=False)
    with pytest.raises(TypeError, match="kb_lengths"):
        dp.load(vq, words, lengths, kb, gm, kb_lengths=sizes[0])


# ---- the read unit's export ------------------------------------------------------------------------------------------------------
def test_read_unit_export_with_lengths(macx, dev):
    """macx_read_fwd_l against the first step of a cell run with the same lengths (its initial memory and first control go in), full
    lengths and NULL against macx_read_fwd, and macx_read_bwd on the `saved` it wrote: exact zeros behind each question's size"""
    lib, L = macx._lib, macx._lib.lib()
    B, S, N, d = 3, 5, 20, 128
    cfg = macx.configs.flag_file_config("args", netLength=1, memDim=d, ctrlDim=d, attDim=d)
    params = macx.MACCellParams(cfg, 1, generator=torch.Generator().manual_seed(0)).to(dev)
    vq, words, lengths, kb = [t.to(dev) for t in macx.configs.synthetic_inputs(B, S, N, d, seed=1)]
    sizes = torch.tensor([7, 20, 1], dtype=torch.int32, device=dev)
    cell = macx.MACCell(vq, words, words, lengths, kb.clone().requires_grad_(True), 1.0, 1.0, 1.0, B, False, config=cfg, params=params,
                        kb_lengths=sizes)
    cell.run()
    run = cell._run
    assert run.keep == 1 and run.shapes.p == 1
    memory, control = cell._memories_all[0].clone(), cell._controls_all[1].clone()
    want_att, want_info = cell._att_kb[0].clone(), cell._infos_all[0].clone()
    head = (C.byref(run.opts), C.byref(run.shapes), C.byref(run.drop), C.byref(run.pstruct))
    saved_floats = L.macx_saved_floats(C.byref(run.opts), C.byref(run.shapes), 1)
    st = abi_kit.stream(dev)

    def read(sizes_or_none, plain=False):
        saved = torch.empty(saved_floats, dtype=torch.float32, device=dev)
        info, att = torch.full((B, d), float("nan"), device=dev), torch.full((B, N), float("nan"), device=dev)
        if plain:
            rc = L.macx_read_fwd(*head, ptr(kb), ptr(memory), ptr(control), ptr(saved), saved_floats, ptr(info), ptr(att), st)
        else:
            rc = L.macx_read_fwd_l(*head, ptr(kb), ptr(sizes_or_none), ptr(memory), ptr(control), ptr(saved), saved_floats, ptr(info), ptr(att), st)
        lib.check(rc, "macx_read_fwd(_l)")
        return saved, info, att

    _, info0, att0 = read(None, plain=True)
    for full in (None, torch.full((B,), N, dtype=torch.int32, device=dev)):
        _, info, att = read(full)
        torch.cuda.synchronize()
        assert bits_equal(info, info0) and bits_equal(att, att0)
    saved, info, att = read(sizes)
    torch.cuda.synchronize()
    assert bits_equal(att, want_att) and bits_equal(info, want_info)
    assert padded_are_zero(att, sizes) and not bits_equal(att, att0)
    # the backward twin that is not needed: macx_read_bwd multiplies by that zero
    gstruct, grads = lib.MacxParamGrads(), {}
    for f in lib.PARAM_FIELDS:
        t = getattr(params, f, None) if f in params.fields else None
        if t is not None:
            grads[f] = torch.full_like(t, float("nan"))
        setattr(gstruct, f, grads[f].data_ptr() if t is not None else None)
    ws_floats = L.macx_ws_floats(C.byref(run.opts), C.byref(run.shapes), 1)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
    dinfo = torch.randn(B, d, generator=torch.Generator().manual_seed(4)).to(dev)
    dkb, dmem, dctl = torch.full_like(kb, float("nan")), torch.empty(B, d, device=dev), torch.empty(B, d, device=dev)
    lib.check(L.macx_read_bwd(*head, ptr(kb), ptr(saved), saved_floats, ptr(ws), ws_floats, ptr(dinfo), C.byref(gstruct), ptr(dkb), ptr(dmem),
                              ptr(dctl), st), "macx_read_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dkb).all()) and padded_are_zero(dkb, sizes)
    assert all(bool((dkb[b, :int(n)] != 0).any()) for b, n in enumerate(sizes))
    assert bool(torch.isfinite(dmem).all()) and bool(torch.isfinite(dctl).all())


# ---- the tower -------------------------------------------------------------------------------------------------------------------
B, S, H, W, CIN, D, E, VOCAB, P, ANSWERS, G = 6, 7, 5, 5, 128, 256, 20, 11, 3, 28, 3
N = H * W
LENGTHS = [7, 1, 3, 7, 5, 2]
INDEX = ([1, 1, 0, 1, 0, 1], [2, 0, 0, 2, 2, 1])          # the first leaves image 2 unnamed
IMAGE_SIZES = ([25, 1, 9], [4, 25, 17])
KB_SIZES = ([25, 1, 9, 13, 25, 2], [3, 25, 1, 8, 19, 25])


def make_net(macx, dev, seed=0, **over):
    known = vars(macx.configs.default_config())
    cfg = macx.configs.flag_file_config("args", **dict(dict(netLength=P, memDim=D, ctrlDim=D, attDim=D, encDim=D, wrdEmbDim=E,
                                                            outClassifierDims=[128]), **{k: v for k, v in over.items() if k in known}))
    for k, v in over.items():                 # (flags the modules read with their own defaults, e.g. the stem's)
        setattr(cfg, k, v)
    return macx.MACNet(cfg, vocab=VOCAB, H=H, W=W, imageInDim=CIN, answerWordsNum=ANSWERS,
                       generator=torch.Generator().manual_seed(seed)).to(dev)


def inputs(dev, seed, images=B):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(images, N, CIN, generator=g))
    lengths = torch.tensor(LENGTHS, dtype=torch.int32)
    q = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32)
    q = q * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)
    ans = torch.randint(0, ANSWERS, (B,), generator=g, dtype=torch.int32)
    return x.to(dev), q.to(dev), lengths.to(dev), ans.to(dev)


def i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def test_captured_tower_forward_with_kb_lengths(macx, dev):
    net = make_net(macx, dev)
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN, kb_lengths=True)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    images, q, lengths, _ = inputs(dev, 1)
    seen = []
    for k, sizes in enumerate(KB_SIZES):
        sizes = i32(sizes, dev)
        with torch.no_grad():
            want = net(images, q, lengths, train=False, kb_lengths=sizes).clone()
            want_att = [a.clone() for a in net.last_cell.attentions["kb"]]
        if k == 0:
            got = fwd(images, q, lengths, kb_lengths=sizes)
        else:                                             # the device tensor rewritten, nothing loaded
            fwd.kb_lengths.copy_(sizes)
            got = fwd.replay()
        torch.cuda.synchronize()
        assert bits_equal(got, want) and all(bits_equal(a, b) for a, b in zip(fwd.attentions["kb"], want_att))
        assert all(padded_are_zero(a, sizes) for a in fwd.attentions["kb"])
        seen.append(got.clone())
    assert not bits_equal(seen[0], seen[1])
    fwd.check()
    with pytest.raises(TypeError, match="kb_lengths"):
        fwd.load(images, q, lengths)
    with pytest.raises(ValueError, match="kb_lengths"):
        fwd.load(images, q, lengths, kb_lengths=i32([0] * B, dev))


def test_captured_tower_forward_with_image_lengths(macx, dev):
    net = make_net(macx, dev)
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN, images=G, image_lengths=True)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    assert fwd.image_lengths.shape == (G,) and fwd.kb_lengths is None
    images, q, lengths, _ = inputs(dev, 2, images=G)
    seen = []
    for k, (index, sizes) in enumerate(zip(INDEX, IMAGE_SIZES)):
        index, sizes = i32(index, dev), i32(sizes, dev)
        with torch.no_grad():
            want = net(images, q, lengths, train=False, image_index=index, image_lengths=sizes).clone()
            want_att = [a.clone() for a in net.last_cell.attentions["kb"]]
            # ... and the pipeline composed by hand from what existed before: stem, plain gather, padding zeroed in torch, the
            # per-question sizes indexed in torch
            per_question = sizes.clamp(1, N)[index.long()]
            kb = macx.stem.kb_gather(net.stem(images, train=False), index)
            live = (torch.arange(N, device=dev)[None, :] < per_question[:, None])[:, :, None]
            kb = torch.where(live, kb, torch.zeros_like(kb))
            words, vecQ = net.enc(q, lengths, train=False)
            cfg = net.config
            cell = macx.MACCell(vecQuestions=vecQ, questionWords=words, questionCntxWords=words, questionLengths=lengths, knowledgeBase=kb,
                                memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout, batchSize=B,
                                train=False, config=cfg, params=net.cell, netLength=P, kb_lengths=per_question)
            by_hand = net.out(cell.run().memory, vecQ, train=False).clone()
        if k == 0:
            got = fwd(images, q, lengths, image_index=index, image_lengths=sizes)
        else:                                             # index and sizes rewritten on the device, nothing loaded
            fwd.image_index.copy_(index)
            fwd.image_lengths.copy_(sizes)
            got = fwd.replay()
        torch.cuda.synchronize()
        assert bits_equal(got, want) and bits_equal(got, by_hand)
        assert all(bits_equal(a, b) for a, b in zip(fwd.attentions["kb"], want_att))
        assert all(padded_are_zero(a, per_question) for a in fwd.attentions["kb"])
        seen.append(got.clone())
    assert not bits_equal(seen[0], seen[1])
    fwd.check()
    with pytest.raises(TypeError, match="image_lengths"):
        fwd.load(images, q, lengths, image_index=index)
    with pytest.raises(ValueError, match="image_lengths"):
        fwd.load(images, q, lengths, image_index=index, image_lengths=sizes + N)


@pytest.mark.parametrize("with_sizes", [True, False], ids=["images and image_lengths", "images alone"])
def test_captured_tower_train_step_with_image_groups(macx, dev, with_sizes):
    net = make_net(macx, dev, stemDropout=1.0)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, H=H, W=W, imageInDim=CIN, seed=1234, images=G, image_lengths=with_sizes,
                                       check_every=1)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert opt.t == 0 and (step.image_lengths is not None) == with_sizes
    ref = make_net(macx, dev, stemDropout=1.0)            # identically initialised
    rbucket = macx.dp.TowerBuckets(ref)                   # per-tensor copy_ gather
    ropt = macx.optim.FlatAdamEMA(rbucket.tensors(), lr=1e-3)
    assert bits_equal(ropt.flat, opt.flat)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    losses = []
    for it, (index, sizes) in enumerate(zip(INDEX, IMAGE_SIZES)):
        images, q, lengths, ans = inputs(dev, 20 + it, images=G)
        index, sizes = i32(index, dev), i32(sizes, dev)
        groups = dict(image_index=index, **({"image_lengths": sizes} if with_sizes else {}))
        step.load(images, q, lengths, ans, **groups)
        step.replay(iteration=it)                         # (check_every=1: ends in a check())
        w = macx.graph.mix32(it)
        word.fill_(w - (1 << 32) if w >= (1 << 31) else w)
        for t in ref.tensors():
            t.grad = None
        logits = ref(images, q, lengths, train=True, seed=1234, check_ids=False, mask_word=word, **groups)
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
        assert any(float(t.grad.abs().max()) > 0 for t in net.stem.tensors())        # the gather's backward reached the stem
        losses.append(float(loss))
    assert step.status() == (0, -1)
    if with_sizes:
        with pytest.raises(TypeError, match="image_lengths"):
            step.load(images, q, lengths, ans, image_index=index)
    else:
        with pytest.raises(TypeError, match="image_lengths"):
            step.load(images, q, lengths, ans, image_index=index, image_lengths=sizes)
    with pytest.raises(ValueError, match="image_index"):
        step.load(images, q, lengths, ans, **{k: v for k, v in groups.items() if k != "image_index"})
