"""-m gpu: image features resident in device memory.  macx_features_pack and macx_features_gather on their own (every comparison is
an equality of bits with torch's CPU conversion and indexing), macx.FeatureStore on top of them, and the tower fed from a store:
MACNet.forward(store, image_ids=) and the captured classes built with features=.

Shapes (n, C, HW) of the pack: (1, 4, 1) one quad; (3, 36, 196) C off the 8-element store vector and off the tile; (2, 128, 49) HW
off the 16-byte load and the tile, two channel tiles; (5, 8, 9) the file fixture's; (2, 72, 68) both vector paths with a tile edge
on both axes (the workload's route: C % 8 == 0, HW % 4 == 0).  Gather: images whose unit count lies before, on and behind the 1 024
units of a workgroup's pass, for 16-byte loads (C*HW % 8 == 0), 8-byte loads and the fp32 copy."""
import os

import numpy as np
import pytest
import torch

from abi_kit import bits_equal, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = os.path.join(ROOT, "tests", "golden", "h5", "features_like_reference.h5")
DTYPES = {"fp16": torch.float16, "fp32": torch.float32}
CODE = {torch.float32: 0, torch.float16: 1}
PACK_SHAPES = [(1, 4, 1), (3, 36, 196), (2, 128, 49), (5, 8, 9), (2, 72, 68)]
# +-0, fp16 subnormals (the smallest is 2^-24 = 5.96e-8: 3e-8 lies just above the tie to zero), exact ties to even in both
# directions, the largest fp16 and the largest value that still rounds to it
SPECIAL = [0.0, -0.0, 1e-7, 6e-8, 3e-8, -1e-7, -6e-8, -3e-8, 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65504.0,
           65519.99, -65504.0, -65519.99, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25]
SENTINEL = 7.0
UNITS = 1024                        # FT_CHUNK / KBG_CHUNK: units (quads) per workgroup and pass


def source(n, C_, HW, seed):
    """[n, C, HW] fp32 on the CPU: values over fp16's normal and subnormal range, the special values at the head of every image,
    at its tail and at random places"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C_ * HW, generator=g) * torch.pow(10.0, torch.randint(-8, 5, (n, C_ * HW), generator=g).float())
    sp = torch.tensor(SPECIAL)
    k = min(len(sp), C_ * HW)
    x[:, :k] = sp[:k]
    x[:, -k:] = sp[:k].flip(0)
    where = torch.randint(0, C_ * HW, (n, 4 * len(sp)), generator=g)
    x.scatter_(1, where, sp.repeat(4)[None].expand(n, -1))
    assert float(x.abs().max()) < 65520
    return x.reshape(n, C_, HW)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_is_torchs_conversion_bit_for_bit(macx, dev, shape, dtype, layout):
    n, C_, HW = shape
    dt = DTYPES[dtype]
    src = source(n, C_, HW, seed=n + C_ + HW)
    want = src.permute(0, 2, 1).contiguous().to(dt)                         # [n, HW, C] on the CPU
    given = src if layout == 0 else src.permute(0, 2, 1).contiguous()
    rows, row0 = n + 3, 2
    table = torch.full((rows, HW, C_), SENTINEL, dtype=dt, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = macx._lib.lib().macx_features_pack(ptr(given.to(dev)), layout, n, C_, HW, ptr(table), CODE[dt], row0, rows, ptr(word), None)
    torch.cuda.synchronize()
    assert rc == 0
    got = table.cpu()
    assert bits_equal(got[row0:row0 + n], want)
    assert bool((got[:row0] == SENTINEL).all()) and bool((got[row0 + n:] == SENTINEL).all())       # the rows on either side
    assert int(word) == 0


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("bad", [65520.0, -65520.0, float("inf"), float("nan"), 1e38])
def test_overflow_word(macx, dev, bad, layout):
    H, W, C_ = 3, 3, 8
    chunk = torch.rand(2, C_, H, W) if layout == 0 else torch.rand(2, H * W, C_)
    store = macx.FeatureStore(4, H, W, C_, dtype=torch.float16, device=dev)
    store.write(0, chunk)
    assert int(store.overflow) == 0 and store.check() is store              # a clean chunk leaves it 0
    chunk.view(-1)[77] = bad
    store.write(2, chunk)
    assert int(store.overflow) == 1
    with pytest.raises(ValueError, match="float16"):
        store.check()
    store.write(0, torch.rand_like(chunk))                                  # the kernel never clears it
    assert int(store.overflow) == 1
    assert not torch.isfinite(store.table[2:].float()).all()                # the value is stored anyway
    # an fp32 store never sets it for finite input; NaN and the infinities do
    f32 = macx.FeatureStore(4, H, W, C_, dtype=torch.float32, device=dev).write(2, chunk)
    finite = bool(np.isfinite(bad))
    assert int(f32.overflow) == (0 if finite else 1)
    if finite:
        f32.check()
    else:
        with pytest.raises(ValueError, match="float32"):
            f32.check()


# ---- gather ------------------------------------------------------------------------------------------------------------------------
# (C, HW): unit counts before, on and behind one pass and two passes of a workgroup.  16-byte loads: a unit is 8 elements;
# 8-byte loads (C*HW % 8 == 4, so the quad count is odd and cannot lie ON the edge): a unit is 4; fp32: a quad is 4.
GATHER_SHAPES = {"fp16": [(8, UNITS - 1), (8, UNITS), (8, UNITS + 1), (8, 2 * UNITS + 1), (4, UNITS - 1), (4, UNITS + 1), (4, 2 * UNITS - 1),
                          (4, 2 * UNITS + 1), (4, 1), (36, 196)],
                 "fp32": [(4, UNITS - 1), (4, UNITS), (4, UNITS + 1), (4, 2 * UNITS + 1), (4, 1), (36, 196)]}
ROWS = 6
IDS = [5, 0, 2, -1, 5, ROWS, 0, 3]          # repeats, row 0 and the last row, and both ends out of range next to good neighbours


@pytest.mark.parametrize("dtype,shape", [(d, s) for d in DTYPES for s in GATHER_SHAPES[d]], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_gather_is_indexing_bit_for_bit(macx, dev, dtype, shape):
    C_, HW = shape
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(C_ + HW)
    table = (torch.randn(ROWS, HW, C_, generator=g) * torch.pow(10.0, torch.randint(-8, 5, (ROWS, HW, C_), generator=g).float())).to(dt)
    table.view(-1)[:4] = torch.tensor([0.0, -0.0, 6e-8, 65504.0]).to(dt)
    ids = torch.tensor(IDS, dtype=torch.int32)
    G, image = len(IDS), HW * C_
    want = torch.full((G, HW, C_), float("nan"))
    ok = (ids >= 0) & (ids < ROWS)
    want[ok] = table[ids[ok].long()].float()
    buf = torch.full((G * image + 64,), SENTINEL, device=dev)               # a sentinel behind `out`
    L = macx._lib.lib()
    dtab, dids = table.to(dev), ids.to(dev)
    rc = L.macx_features_gather(ptr(dtab), CODE[dt], ROWS, ptr(dids), G, C_, HW, ptr(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    got = buf[:G * image].view(G, HW, C_).cpu()
    assert bits_equal(got[ok], want[ok])                                    # neighbours of a bad id are exact
    bad = got[~ok].view(torch.int32)
    assert bad.numel() == 2 * image and bool((bad == 0x7FC00000).all())     # the whole block quiet NaN
    assert bool((buf[G * image:] == SENTINEL).all())
    if dt == torch.float32:                                                 # the same launch as macx_kb_gather: the copy, bit for bit
        other = torch.full_like(buf, SENTINEL)
        assert L.macx_kb_gather(ptr(dtab), ptr(dids), ROWS, G, HW, C_, ptr(other), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), other.view(torch.int32))
    # the store's method: the same call, any integer dtype of ids
    store = macx.FeatureStore(ROWS, 1, HW, C_, dtype=dt, device=dev)
    store.table.copy_(dtab)
    out = store.gather(ids.long().to(dev))
    assert out.dtype == torch.float32 and not out.requires_grad and bits_equal(out.cpu(), got)


def test_offsets_are_64_bit(macx, dev):
    """an fp16 table just over 4 GiB, allocated and never filled: row 0, one in the middle (behind 2^31 BYTES) and the last (behind
    2^31 ELEMENTS and 2^32 bytes) are packed and gathered back"""
    rows, H, W, C_ = 132000, 4, 4, 1024
    image = H * W * C_
    assert 66000 * image * 2 > 1 << 31 and (rows - 1) * image > 1 << 31 and (rows - 1) * image * 2 > 1 << 32
    table = torch.empty(rows, H * W, C_, dtype=torch.float16, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    L = macx._lib.lib()
    pick = [0, 66000, rows - 1]
    g = torch.Generator().manual_seed(8)
    for round_, layout in enumerate((0, 1)):                                # the tile kernel and the flat one
        src = torch.randn(len(pick), C_, H * W, generator=g) if layout == 0 else torch.randn(len(pick), H * W, C_, generator=g)
        want = (src.permute(0, 2, 1) if layout == 0 else src).contiguous().to(torch.float16).float()
        dsrc = src.to(dev)
        for i, r in enumerate(pick):
            assert L.macx_features_pack(ptr(dsrc[i]), layout, 1, C_, H * W, ptr(table), 1, r, rows, ptr(word), None) == 0
        ids = torch.tensor(pick[::-1] + [pick[1]], dtype=torch.int32, device=dev)
        out = torch.empty(4, H * W, C_, device=dev)
        assert L.macx_features_gather(ptr(table), 1, rows, ptr(ids), 4, C_, H * W, ptr(out), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[[2, 1, 0, 1]]), (round_, layout)
        assert torch.equal(table[rows - 1].cpu().float(), want[2]) and torch.equal(table[66000].cpu().float(), want[1])
    assert int(word) == 0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_from_h5_is_the_files_array_transposed_and_rounded(macx, dev, dtype):
    dt = DTYPES[dtype]
    store = macx.FeatureStore.from_h5(H5, dtype=dt, device=dev, chunk_rows=3)
    with macx.h5.File(H5) as f:
        arr = torch.from_numpy(np.asarray(f["features"]).copy())                   # [7, 8, 3, 3]
    assert (store.rows, store.C, store.H, store.W, store.dtype) == (7, 8, 3, 3, dt) and store.nbytes == 7 * 72 * (2 if dt == torch.float16 else 4)
    want = arr.permute(0, 2, 3, 1).reshape(7, 9, 8).contiguous().to(dt)
    assert bits_equal(store.table.cpu(), want)
    ids = torch.tensor([6, 0, 3, 3], device=dev)
    assert bits_equal(store.gather(ids).cpu(), want[ids.cpu()].float())


# ---- the tower ---------------------------------------------------------------------------------------------------------------------
B, H, W, CIN, D, P, S, A, V, E, IMAGES = 3, 4, 3, 128, 256, 2, 6, 7, 12, 20, 5          # test_full_tower_ids_to_logits_gradients' shape


def make_net(macx, dev, **over):
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D, encDim=D, wrdEmbDim=E, outClassifierDims=[32],
                                        answerWordsNum=A)
    cfg.stemDim = 128
    for k, v in over.items():
        setattr(cfg, k, v)
    return macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=CIN, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)


def make_store(macx, dev, dtype=torch.float16):
    g = torch.Generator().manual_seed(6)
    store = macx.FeatureStore(IMAGES, H, W, CIN, dtype=dtype, device=dev)
    return store.write(0, torch.relu(torch.randn(IMAGES, CIN, H, W, generator=g))).check()


def questions(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.tensor([S, 2, 4], dtype=torch.int32)
    q = torch.randint(1, V + 1, (B, S), generator=g, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    return q.to(dev), lengths.to(dev), torch.tensor([1, 5, 2], dtype=torch.int32, device=dev)


def run(net, images, q, lengths, ans, train, **kw):
    """(logits, gradients of every parameter) of one eager call"""
    for t in net.tensors():
        t.grad = None
    if not train:
        with torch.no_grad():
            return net(images, q, lengths, train=False, **kw).clone(), []
    logits = net(images, q, lengths, train=True, seed=21, **kw)
    net.loss_and_pred(logits, ans)[0].backward()
    torch.cuda.synchronize()
    return logits.detach().clone(), [t.grad.clone() for t in net.tensors()]


def same(x, y):
    return bits_equal(x[0], y[0]) and len(x[1]) == len(y[1]) and all(bits_equal(a, b) for a, b in zip(x[1], y[1]))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shared", [False, True], ids=["one image per question", "image_index"])
def test_forward_from_a_store_is_forward_on_its_gather(macx, dev, dtype, shared):
    net = make_net(macx, dev, **({"stemDropout": 1.0} if shared else {}))
    store = make_store(macx, dev, DTYPES[dtype])
    q, lengths, ans = questions(dev)
    if shared:
        ids, kw = torch.tensor([4, 1], device=dev), {"image_index": torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)}
    else:
        ids, kw = torch.tensor([4, 0, 4], device=dev), {}
    for train in (False, True):
        got = run(net, store, q, lengths, ans, train, image_ids=ids, **kw)
        want = run(net, store.gather(ids), q, lengths, ans, train, **kw)
        assert same(got, want), train
        assert not train or (len(got[1]) == len(net.tensors()) and all(bool(torch.isfinite(t).all()) for t in got[1]))
        other = run(net, store, q, lengths, ans, train, image_ids=torch.tensor([2, 3] if shared else [2, 3, 1], device=dev), **kw)
        assert not bits_equal(other[0], got[0])                             # (the ids matter)
    with pytest.raises(IndexError, match="image_ids outside"):
        net(store, q, lengths, image_ids=ids + 1, **kw)                     # check_ids: the range, on the host


def test_captured_forward_from_a_store(macx, dev):
    net, store = make_net(macx, dev), make_store(macx, dev)
    q, lengths, _ = questions(dev)
    fwd = macx.CapturedTowerForward(net, B, S, features=store)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    assert fwd.images is None and fwd.image_ids.dtype == torch.int32 and tuple(fwd.image_ids.shape) == (B,)
    eager = lambda ids: run(net, store.gather(ids), q, lengths, None, False)[0]
    for ids in (torch.tensor([4, 0, 4], device=dev), torch.tensor([1, 2, 3], dtype=torch.int32, device=dev)):
        assert bits_equal(fwd(None, q, lengths, image_ids=ids).clone(), eager(ids))
    fwd.image_ids.copy_(torch.tensor([0, 0, 2]))                            # one graph follows rewritten ids
    assert bits_equal(fwd.replay().clone(), eager(torch.tensor([0, 0, 2], device=dev)))
    with pytest.raises(IndexError, match="image_ids outside"):
        fwd.load(None, q, lengths, image_ids=torch.tensor([0, 5, 2], device=dev))
    with pytest.raises(ValueError, match="captured with features="):
        fwd.load(store.gather(torch.tensor([0, 1, 2], device=dev)), q, lengths)


def test_captured_train_step_from_a_store(macx, dev):
    """two loads with different ids train as the eager step on the gathered images does; a short batch gives the same bits whatever
    id sits in its dead slot"""
    net, store = make_net(macx, dev), make_store(macx, dev)
    q, lengths, ans = questions(dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, seed=1234, features=store, weights=True)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    ref = make_net(macx, dev)
    rbucket = macx.dp.TowerBuckets(ref)
    ropt = macx.optim.FlatAdamEMA(rbucket.tensors(), lr=1e-3)
    assert bits_equal(ropt.flat, opt.flat)
    word, ones = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(B, device=dev)
    for it, ids in enumerate(([4, 0, 4], [1, 2, 3])):
        ids = torch.tensor(ids, device=dev)
        assert step.load(None, q, lengths, ans, image_ids=ids) == B
        step.replay(iteration=it)
        w = macx.graph.mix32(it) & 0xFFFFFFFF
        word.fill_(w - (1 << 32) if w >= 1 << 31 else w)
        for t in ref.tensors():
            t.grad = None
        logits = ref(store.gather(ids), q, lengths, train=True, seed=1234, check_ids=False, mask_word=word)
        loss, pred = ref.loss_and_pred(logits, ans, weights=ones)
        rbucket.begin_step(B, B)
        loss.backward()
        rbucket.allreduce_(B, B)
        norm = ropt.step(flat_grad=rbucket.flat)
        torch.cuda.synchronize()
        pairs = {"loss": (step.loss, loss.detach()), "logits": (step.logits, logits.detach()), "norm": (step.norm, norm),
                 "flat gradient": (bucket.flat, rbucket.flat), "flat parameters": (opt.flat, ropt.flat)}
        for what, (a, b) in pairs.items():
            assert bits_equal(a.reshape(-1), b.reshape(-1)), (it, what)
        assert torch.equal(step.pred, pred)
    # a short batch: whatever id sat in the dead slot, load() puts slot 0's id there (as it does for every per-question tensor,
    # test_gpu_answer_weights.py) and the step gives the same bits
    state, results = step._state(), []
    for stale in (3, 0, 4):
        step._restore(state)
        step.image_ids.fill_(stale)
        assert step.load(None, q[:2], lengths[:2], ans[:2], image_ids=torch.tensor([3, 1], device=dev)) == 2
        assert step.image_ids.tolist() == [3, 1, 3] and step.weights.tolist() == [1.0, 1.0, 0.0]
        step.replay(iteration=7)
        results.append([t.clone() for t in (step.loss, step.logits[:2], bucket.flat, opt.flat)])
    for other in results[1:]:
        assert all(bits_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(results[0], other))
    assert not bits_equal(results[0][3], state[0][0])                       # (the step trained)
