"""-m gpu: the generic stem (GenericStem on macx_conv2d_*) for every stem option of the reference, against the fp64 restatement
tests/stem_variants_ref.py with the masks of oracle/dropout_hash.py; the conv exports on their own (odd shapes, guard bands,
bit-identical repeats, refusals); GenericStem against the fused Stem on the default configuration; the whole tower
(stem -> MAC cell -> classifier) with a variant stem."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import abi_kit
import stem_variants_ref as sv
from helpers import max_abs, rel_err
from oracle import dropout_hash as dh
from oracle import mac_oracle as mo

pytestmark = pytest.mark.gpu

MATRIX = {   # name: (flags, B, H, W, Cin, memDim)
    "one_layer_k1": (dict(stemNumLayers=1, stemKernelSize=1), 3, 6, 6, 32, 16),
    "three_layers_k3": (dict(stemNumLayers=3), 3, 6, 6, 32, 16),
    "k5": (dict(stemKernelSize=5), 3, 7, 6, 24, 20),
    "even_k_stride2": (dict(stemKernelSizes=[2, 4], stemStrideSizes=[2, 2]), 3, 9, 8, 16, 12),
    "strides_2_1": (dict(stemStrideSizes=[2, 1]), 3, 14, 14, 64, 32),
    "h5_w3": (dict(stemKernelSize=3, stemNumLayers=3, stemStrideSizes=[1, 2, 1]), 2, 5, 3, 8, 12),
    "nlvr_8x32": (dict(stemKernelSizes=[3, 1]), 2, 8, 32, 16, 24),
    "stem_dim_64": (dict(stemDim=64, stemKernelSize=2), 3, 6, 5, 32, 128),
    "loc_L": (dict(locationAware=True), 3, 6, 7, 32, 16),
    "loc_PE": (dict(locationAware=True, locationType="PE", locationDim=5), 3, 6, 6, 32, 16),
    "linear": (dict(stemLinear=True), 3, 5, 5, 32, 24),
    "elu": (dict(relu="ELU", stemNumLayers=3, stemKernelSizes=[1, 3, 2]), 2, 6, 6, 16, 16),
}


def make_cfg(flags, memDim, stemDim=24):
    base = dict(memDim=memDim, stemDim=stemDim, stemDropout=0.82, relu="STD")
    base.update(flags)
    return SimpleNamespace(**base)


def layer_inputs(cfg, B, H, W, Cin, memDim):
    linear, loc, layers = sv.plan(cfg, Cin, memDim)
    shapes, hh, ww = [], H, W
    for _, shape, s in layers:
        shapes.append((B, hh, ww, shape[-2]))
        hh, ww = -(-hh // s), -(-ww // s)
    return linear, shapes, (hh, ww)


def run_variant(macx, dev, cfg, B, H, W, Cin, memDim, train, b0=2, seed=13, feed=False):
    stem = macx.Stem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1)).to(dev)
    if not isinstance(stem, macx.GenericStem):
        stem = macx.GenericStem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():               # seeded: the same data on every run
        for f, n in stem.names:
            if n.endswith("bias"):
                b = getattr(stem, f)
                b.copy_((torch.rand(b.shape, generator=g) - 0.5).to(dev))
    img = torch.relu(torch.randn(B, H, W, Cin, generator=g))
    imgd = img.to(dev).requires_grad_(True)
    kb = stem(imgd.reshape(B, H * W, Cin), train=train, seed=seed, b0=b0)
    dkb = torch.randn(kb.shape, generator=g) / B
    (kb * dkb.to(dev)).sum().backward()
    torch.cuda.synchronize()
    linear, shapes, hw = layer_inputs(cfg, B, H, W, Cin, memDim)
    assert stem.out_hw == hw and tuple(kb.shape) == (B, hw[0] * hw[1], memDim)
    masks = None
    if train and not linear:
        masks = [torch.from_numpy(dh.mask_for(seed, 9 if i == 0 else 10, max(i - 1, 0), cfg.stemDropout, sh, b0=b0)).double()
                 for i, sh in enumerate(shapes)]
    prm = {k: v.cpu().double().requires_grad_(True) for k, v in stem.to_reference_dict().items()}
    imgr = img.double().requires_grad_(True)
    ref = sv.stem(cfg, imgr, prm, memDim, keep=cfg.stemDropout, masks=masks)
    (ref * dkb.double()).sum().backward()
    errs = {"kb": rel_err(kb, ref), "images": rel_err(imgd.grad, imgr.grad)}
    for f, n in stem.names:
        errs[n] = rel_err(getattr(stem, f).grad, prm[n].grad)
    return errs


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", sorted(MATRIX))
def test_generic_stem_option_matrix(macx, dev, name, train):
    flags, B, H, W, Cin, memDim = MATRIX[name]
    errs = run_variant(macx, dev, make_cfg(flags, memDim), B, H, W, Cin, memDim, train)
    print(name, train, {k: "%.1e" % v for k, v in errs.items()})
    assert errs["kb"] < 2e-5, errs
    assert all(v < 2e-4 for v in errs.values()), errs


# The two large cases run under ELU (--relu ELU, as configs/args*.txt): its derivative is continuous, so the fp32 / fp64
# comparison is well posed.  Under ReLU, one of the ~10^6 pre-activations landing within fp32 rounding of zero flips its
# derivative and moves a whole column of the bias gradient by one cotangent entry (~1e-2 of that gradient).
def test_generic_stem_clevr_three_layers(macx, dev):
    """CLEVR's features 14 x 14 x 1024 -> 512 -> 512 -> 512 (three layers), B = 8, training mode"""
    cfg = make_cfg(dict(stemNumLayers=3, relu="ELU"), 512, stemDim=512)
    errs = run_variant(macx, dev, cfg, 8, 14, 14, 1024, 512, True, b0=5)
    print("clevr 3 layers", {k: "%.1e" % v for k, v in errs.items()})
    assert errs["kb"] < 2e-5 and all(v < 2e-4 for v in errs.values()), errs


def test_generic_stem_location_1026_channels(macx, dev):
    """locationAware L on 1024 channels: layer 0 reads 1026 (padded to 1028 inside)"""
    cfg = make_cfg(dict(locationAware=True, relu="ELU"), 128, stemDim=128)
    errs = run_variant(macx, dev, cfg, 2, 14, 14, 1024, 128, True)
    assert errs["kb"] < 2e-5 and all(v < 2e-4 for v in errs.values()), errs


def test_generic_stem_matches_fused_stem_on_default(macx, dev):
    """GenericStem on the default configuration against the fused Stem: same weights, same masks"""
    cfg = mo.flag_file_config("args", memDim=128, ctrlDim=128, attDim=128)
    cfg.stemDim = 256
    B, H, W, Cin = 4, 14, 14, 128
    fused = macx.Stem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1)).to(dev)
    gen = macx.GenericStem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1)).to(dev)
    assert type(fused) is macx.Stem
    gb = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for a, b in zip(fused.tensors(), gen.tensors()):
            assert torch.equal(a, b)
            if a.dim() == 1:
                a.copy_((torch.rand(a.shape, generator=gb) - 0.5).to(dev))
                b.copy_(a)
    img = torch.relu(torch.randn(B, H * W, Cin, generator=torch.Generator().manual_seed(2))).to(dev)
    for train in (False, True):
        ka = fused(img, train=train, seed=9, b0=3)
        kb = gen(img, train=train, seed=9, b0=3)
        d = torch.randn(ka.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        (ka * d).sum().backward()
        (kb * d).sum().backward()
        torch.cuda.synchronize()
        assert rel_err(kb, ka) < 2e-5
        for a, b in zip(fused.tensors(), gen.tensors()):
            assert rel_err(b.grad, a.grad) < 2e-4
            a.grad = b.grad = None


def conv_call(macx, which, sh, *bufs, ws=None, n_ws=0):
    L = macx._lib.lib()
    st = abi_kit.stream(None)
    p = [abi_kit.ptr(b) for b in bufs]
    if which == "fwd":
        return L.macx_conv2d_fwd(C.byref(sh), *p, st)
    if which == "bwd":
        return L.macx_conv2d_bwd_data(C.byref(sh), *p, st)
    return L.macx_conv2d_wgrad(C.byref(sh), *p, abi_kit.ptr(ws), n_ws, st)


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s", [(1, 1, 1, 4, 4, 1, 1), (3, 5, 3, 12, 20, 3, 1), (2, 9, 7, 4, 132, 2, 2),
                                                 (2, 13, 11, 260, 8, 4, 3), (5, 14, 14, 36, 8, 5, 2), (1, 3, 17, 8, 12, 6, 1),
                                                 (64, 14, 14, 64, 16, 3, 1)])
def test_conv_exports_odd_shapes_guards_and_repeatability(macx, dev, B, H, W, Cin, Cout, k, s):
    sh = macx._lib.MacxConvShapes(B, H, W, Cin, Cout, k, s)
    Ho, Wo = -(-H // s), -(-W // s)
    g = torch.Generator().manual_seed(B * 100 + k)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(k, k, Cin, Cout, generator=g, dtype=torch.float64) / (k * Cin ** 0.5)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    dy = torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = sv.conv2d_same(xr, wr, s) + b
    yr.backward(dy)
    ny, nx, nw = B * Ho * Wo * Cout, B * H * W * Cin, k * k * Cin * Cout
    gy, gx, gw = abi_kit.Guarded(ny, dev), abi_kit.Guarded(nx, dev), abi_kit.Guarded(nw, dev)
    y, dx, dw = gy.view, gx.view, gw.view
    n_ws = macx._lib.lib().macx_conv2d_ws_floats(C.byref(sh))
    gs = abi_kit.Guarded(max(n_ws, 4), dev)
    ws = gs.view
    xd, wd, bd, dyd = [t.float().contiguous().to(dev) for t in (x, w, b, dy)]
    assert conv_call(macx, "fwd", sh, xd, wd, bd, y) == 0
    assert conv_call(macx, "bwd", sh, dyd, wd, dx) == 0
    assert conv_call(macx, "wgrad", sh, xd, dyd, dw, ws=ws, n_ws=n_ws) == 0
    torch.cuda.synchronize()
    ey, ex, ew = rel_err(y.reshape(yr.shape), yr), rel_err(dx.reshape(x.shape), xr.grad), rel_err(dw.reshape(w.shape), wr.grad)
    print("conv", (B, H, W, Cin, Cout, k, s), "slabs ws", n_ws, "errors %.1e %.1e %.1e" % (ey, ex, ew))
    assert ey < 2e-5 and ex < 2e-5 and ew < 2e-5
    assert gy.intact() and gx.intact() and gw.intact() and gs.intact()
    y1, dx1, dw1 = y.clone(), dx.clone(), dw.clone()
    assert conv_call(macx, "fwd", sh, xd, wd, bd, y) == 0
    assert conv_call(macx, "bwd", sh, dyd, wd, dx) == 0
    assert conv_call(macx, "wgrad", sh, xd, dyd, dw, ws=ws, n_ws=n_ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y1) and torch.equal(dx, dx1) and torch.equal(dw, dw1)


def test_conv_exports_refuse_bad_input(macx, dev):
    L = macx._lib.lib()
    t = torch.zeros(4096, device=dev)
    ok = macx._lib.MacxConvShapes(1, 4, 4, 4, 4, 3, 1)
    assert conv_call(macx, "fwd", ok, t, t, None, t) == 0
    for bad in [(1, 4, 4, 6, 4, 3, 1), (1, 4, 4, 4, 6, 3, 1), (0, 4, 4, 4, 4, 3, 1), (1, 4, 4, 4, 4, 0, 1), (1, 4, 4, 4, 4, 3, 0),
                (1, 0, 4, 4, 4, 3, 1)]:
        sh = macx._lib.MacxConvShapes(*bad)
        assert conv_call(macx, "fwd", sh, t, t, None, t) == macx._lib.MACX_EINVAL
        assert conv_call(macx, "bwd", sh, t, t, t) == macx._lib.MACX_EINVAL
        assert conv_call(macx, "wgrad", sh, t, t, t, ws=t, n_ws=4096) == macx._lib.MACX_EINVAL
    assert conv_call(macx, "fwd", ok, t[1:], t, None, t) == macx._lib.MACX_EINVAL          # 16-byte alignment
    big = macx._lib.MacxConvShapes(64, 14, 14, 1024, 512, 3, 1)
    need = L.macx_conv2d_ws_floats(C.byref(big))
    assert need > 0
    assert conv_call(macx, "wgrad", big, t, t, t, ws=t, n_ws=need - 1) == macx._lib.MACX_EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("flags", [dict(stemStrideSizes=[2, 1]), dict(locationAware=True, locationType="PE", locationDim=8)])
def test_tower_with_variant_stem(macx, dev, flags):
    """images -> GenericStem -> MAC cell x p -> classifier -> CE: logits and every gradient against restatement stem +
    mo.mac_network + mo.output_classifier in fp64, identical dropout masks"""
    B, H, W, Cin, d, p, S, A = 3, 6, 6, 128, 128, 2, 6, 7
    cfg = mo.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d, outClassifierDims=[32], answerWordsNum=A)
    cfg.stemDim = 128
    for k, v in flags.items():
        setattr(cfg, k, v)
    net = macx.MACNetCore(cfg, H=H, W=W, imageInDim=Cin, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)
    assert isinstance(net.stem, macx.GenericStem)
    g = torch.Generator().manual_seed(6)
    img = torch.relu(torch.randn(B, H * W, Cin, generator=g))
    vq, words, lengths, _ = mo.synthetic_inputs(B, S, 1, d, seed=8)
    ans = torch.tensor([1, 5, 2])
    logits = net(img.to(dev), vq.to(dev), words.to(dev), lengths.to(dev), train=True, seed=21)
    loss, pred = net.loss_and_pred(logits, ans.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert net.last_cell.knowledgeBase.shape[1] == net.stem.N
    dt = torch.float64
    prm = {}
    for src in (net.stem.to_reference_dict(), net.cell.to_reference_dict(), net.out.to_reference_dict()):
        prm.update({k: v.cpu().to(dt).requires_grad_(True) for k, v in src.items()})
    vs = mo.VarStore(params=prm, dtype=dt)
    keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout)
    sk, ok = net.stem.keep, net.out.keep
    _, shapes, _ = layer_inputs(cfg, B, H, W, Cin, d)
    smasks = [torch.from_numpy(dh.mask_for(21, 9 if i == 0 else 10, max(i - 1, 0), sk, sh)).to(dt) for i, sh in enumerate(shapes)]
    kb = sv.stem(cfg, img.to(dt).reshape(B, H, W, Cin), prm, d, keep=sk, masks=smasks)
    c, m, _ = mo.mac_network(cfg, vs, vq.to(dt), words.to(dt), words.to(dt), lengths, kb, train=True, mask_fn=mo.hash_mask_fn(21, keeps),
                             keeps=keeps)
    omasks = [torch.from_numpy(dh.mask_for(21, 7, 0, ok, (B, 2 * d))).to(dt), torch.from_numpy(dh.mask_for(21, 8, 0, ok, (B, 32))).to(dt)]
    rl = mo.output_classifier(cfg, vs, m, vq.to(dt), output_keep=ok, masks=omasks)
    rloss, rpred = mo.answer_loss_and_pred(rl, ans)
    rloss.backward()
    assert max_abs(logits, rl) < 5e-5 and torch.equal(pred.cpu(), rpred)
    bad = {}
    for f, n in net.stem.names:
        e = rel_err(getattr(net.stem, f).grad, prm[n].grad)
        if not e < 3e-4:
            bad[n] = e
    for mod, refs in ((net.cell, macx.params.reference_names(cfg, p)), (net.out, {f: [(n, None)] for f, n in macx.output.REF_NAMES.items()})):
        for f, lst in refs.items():
            if not hasattr(mod, f):
                continue
            for refname, idx in lst:
                rg = prm[refname].grad
                got = getattr(mod, f).grad
                got = got if idx is None else got[idx]
                floor = 5e-2 if refname.endswith("linearLayerlogits/biases/bias") else 1e-7
                e = rel_err(got.reshape(rg.shape), rg, floor=floor)
                if not e < 3e-4:
                    bad[refname] = e
    assert not bad, bad
