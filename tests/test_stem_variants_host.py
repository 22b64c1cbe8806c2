"""CPU: GenericStem's host logic (layer plan, SAME padding, dropout masks and sites, location grid, variable names / shapes /
order, dispatch from Stem, the refusals) against the fp64 restatement tests/stem_variants_ref.py, with the kernel calls of
stem.py / generic.py swapped for torch restatements (the pattern of tests/test_generic_host.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from types import SimpleNamespace

import stem_variants_ref as sv
from oracle import dropout_hash as dh

VARIANTS = {
    "default": {},
    "one_layer_k1": dict(stemNumLayers=1, stemKernelSize=1),
    "three_layers": dict(stemNumLayers=3),
    "k5": dict(stemKernelSize=5),
    "even_k_stride2": dict(stemKernelSizes=[2, 4], stemStrideSizes=[2, 2]),
    "strides_2_1": dict(stemStrideSizes=[2, 1]),
    "stem_dim": dict(stemDim=16),
    "loc_L": dict(locationAware=True),
    "loc_PE": dict(locationAware=True, locationType="PE", locationDim=3, locationBias=2.0),
    "linear": dict(stemLinear=True),
    "elu": dict(relu="ELU", stemKernelSize=2),
}


def cfg_of(**kw):
    base = dict(memDim=12, stemDim=8, stemDropout=0.82, relu="STD")
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.fixture
def host_stem(macx, monkeypatch):
    S, G = macx.stem, macx.generic

    def conv_fwd(x, w, b, s):
        return sv.conv2d_same(x, w, s) + b

    def conv_bwd_data(dy, w, x_shape, s):
        with torch.enable_grad():           # (called from inside an autograd backward)
            x = torch.zeros(x_shape, dtype=dy.dtype, requires_grad=True)
            return torch.autograd.grad(sv.conv2d_same(x, w, s), x, dy)[0]

    def conv_wgrad(x, dy, w_shape, s):
        with torch.enable_grad():
            w = torch.zeros(w_shape, dtype=dy.dtype, requires_grad=True)
            return torch.autograd.grad(sv.conv2d_same(x, w, s), w, dy)[0]

    def dropout(x, seed, site, step, keep, first, mask_word=None):
        m = torch.as_tensor(dh.keep_mask(seed, site, step, keep, first, x.numel())).reshape(x.shape)
        return x * np.float32(1.0 / keep) * m

    def act(a, x, alpha):
        return torch.relu(x) if a == 4 else torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))

    def act_bwd(a, x, alpha, g):
        return g * (x > 0).to(g.dtype) if a == 4 else g * torch.where(x > 0, torch.ones_like(x), torch.exp(x)), None

    def reduce(mode, x, outer, mid, inner):
        assert mode == G.R_ROWS
        return x.reshape(outer, inner).sum(0)

    for name, f in dict(k_conv_fwd=conv_fwd, k_conv_bwd_data=conv_bwd_data, k_conv_wgrad=conv_wgrad).items():
        monkeypatch.setattr(S, name, f)
    for name, f in dict(k_dropout=dropout, k_act=act, k_act_bwd=act_bwd, k_reduce=reduce).items():
        monkeypatch.setattr(G, name, f)
    monkeypatch.setattr(G, "_require_device", lambda t, name: None)
    return S


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_generic_stem_host_logic_matches_the_restatement(macx, host_stem, variant, train):
    B, H, W, Cin, b0, seed = 2, 5, 3, 8, 3, 77
    cfg = cfg_of(**VARIANTS[variant])
    stem = macx.Stem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1))
    fused = variant in ("default", "stem_dim")          # the fused stem takes any widths of the 2-layer 3x3 CNN
    assert isinstance(stem, macx.GenericStem) != fused
    if fused:
        stem = macx.GenericStem(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1))
    names = sv.variable_names(cfg, Cin, cfg.memDim)
    ref_vars = stem.to_reference_dict()
    assert [(n, tuple(v.shape)) for n, v in ref_vars.items()] == [(n, tuple(s)) for n, s in names]
    assert len(stem.tensors()) == len(names)
    for (n, s), t in zip(names, [t.detach() for t in stem.tensors()]):
        if n.endswith("bias"):
            assert float(t.abs().max()) == 0.0
        else:
            assert float(t.abs().max()) <= sv.xavier_limit(s) and float(t.abs().max()) > 0.5 * sv.xavier_limit(s)
    linear, loc, layers = sv.plan(cfg, Cin, cfg.memDim)
    hh, ww, shapes = H, W, []
    for _, shape, s in layers:
        shapes.append((B, hh, ww, shape[-2]))
        hh, ww = -(-hh // s), -(-ww // s)
    assert stem.out_hw == (hh, ww)
    g = torch.Generator().manual_seed(4)
    img = torch.randn(B, H * W, Cin, generator=g)
    masks = None
    if train and not linear:
        masks = [torch.as_tensor(dh.mask_for(seed, 9 if i == 0 else 10, max(i - 1, 0), cfg.stemDropout, sh, b0=b0)).double()
                 for i, sh in enumerate(shapes)]
    params = {n: v.double().requires_grad_(True) for n, v in ref_vars.items()}
    imgr = img.double().reshape(B, H, W, Cin).requires_grad_(True)
    want = sv.stem(cfg, imgr, params, cfg.memDim, keep=cfg.stemDropout, masks=masks)
    imgd = img.clone().requires_grad_(True)
    got = stem(imgd, train=train, seed=seed, b0=b0)
    assert got.shape == (B, hh * ww, cfg.memDim)
    assert float((got.detach().double() - want.detach()).abs().max()) <= 1e-5 * float(want.abs().max())
    cot = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (want * cot).sum().backward()
    (got * cot.float()).sum().backward()
    assert float((imgd.grad.double().reshape(imgr.shape) - imgr.grad).abs().max()) <= 1e-4 * float(imgr.grad.abs().max())
    for (n, _), t in zip(names, stem.tensors()):
        r = params[n].grad
        assert float((t.grad.double() - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-30), n


def test_same_padding_and_location_grid(macx):
    S = macx.stem
    for n in range(1, 9):
        for k in range(1, 6):
            for s in range(1, 4):
                assert S.same_pads(n, k, s) == sv.same_pads(n, k, s)
                assert S.out_dim(n, s) == -(-n // s)
    assert S.same_pads(14, 2, 2) == (0, 0) and S.same_pads(14, 4, 2) == (1, 1) and S.same_pads(5, 2, 1) == (0, 1)
    for t, dim in (("L", 32), ("PE", 3), ("PE", 8)):
        for h, w in ((14, 14), (5, 3), (8, 32), (1, 4)):
            got = S.location_grid(t, h, w, dim, 1.5)
            assert torch.allclose(got, sv.location_grid(t, h, w, dim, 1.5), atol=1e-15, rtol=0)
    grid = S.location_grid("L", 2, 3, 32, 1.0)
    assert grid[0, :, 0].tolist() == [-1.0, 0.0, 1.0] and grid[:, 0, 1].tolist() == [-1.0, 1.0]   # channel 0 varies along W


def test_dispatch_and_output_grid(macx):
    assert type(macx.Stem(cfg_of(), H=4, W=4, inDim=8)) is macx.Stem
    st = macx.Stem(cfg_of(stemStrideSizes=[2, 1], memDim=512, stemDim=512), H=14, W=14, inDim=1024)
    assert isinstance(st, macx.GenericStem) and st.out_hw == (7, 7) and st.N == 49
    st = macx.Stem(cfg_of(locationAware=True, memDim=512, stemDim=512), H=14, W=14, inDim=1024)
    assert st.layers[0][2] == 1026 and tuple(st.kernel0.shape) == (3, 3, 1026, 512)
    st = macx.Stem(cfg_of(locationAware=True, locationType="PE", memDim=512), H=14, W=14, inDim=1024)
    assert tuple(st.kernel0.shape) == (3, 3, 1024 + 128, 8)
    st = macx.Stem(cfg_of(stemNumLayers=0), H=4, W=4, inDim=8)
    assert [n for n in st.to_reference_dict()] == ["stem/cnnLayercnn_0/kernels/kernel", "stem/cnnLayercnn_0/biases/bias"]
    # the generic stem and the fused one draw the same weights for the default configuration
    a = macx.Stem(cfg_of(), H=4, W=4, inDim=8, generator=torch.Generator().manual_seed(3)).to_reference_dict()
    b = macx.GenericStem(cfg_of(), H=4, W=4, inDim=8, generator=torch.Generator().manual_seed(3)).to_reference_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_checkpoint_round_trip_and_tower(macx):
    cfg = cfg_of(stemKernelSizes=[1, 5], stemStrideSizes=[2, 1])
    st = macx.Stem(cfg, H=6, W=6, inDim=8, generator=torch.Generator().manual_seed(0))
    other = macx.Stem(cfg, H=6, W=6, inDim=8, generator=torch.Generator().manual_seed(1))
    macx.checkpoint.load_reference(other, macx.checkpoint.reference_state_dict(st))
    assert all(torch.equal(a, b) for a, b in zip(st.tensors(), other.tensors()))
    with pytest.raises(ValueError):
        other.load_reference_dict({"stem/cnnLayercnn_0/kernels/kernel": torch.zeros(3, 3, 8, 8)})
    from oracle import mac_oracle as mo
    tcfg = mo.default_config(netLength=2, memDim=128, ctrlDim=128, attDim=128)
    tcfg.stemStrideSizes = [2, 1]
    net = macx.MACNetCore(tcfg, H=14, W=14, imageInDim=64, answerWordsNum=5, generator=torch.Generator().manual_seed(0))
    assert isinstance(net.stem, macx.GenericStem) and net.stem.N == 49
    assert list(macx.checkpoint.reference_state_dict(net))[:4] == [
        "macModel/stem/cnnLayercnn_0/kernels/kernel:0", "macModel/stem/cnnLayercnn_0/biases/bias:0",
        "macModel/stem/cnnLayercnn_1/kernels/kernel:0", "macModel/stem/cnnLayercnn_1/biases/bias:0"]


@pytest.mark.parametrize("flags,exc", [
    (dict(stemBN=True), KeyError), (dict(stemGridRnn=True), NameError), (dict(stemKernelSizes=[3]), IndexError),
    (dict(stemNumLayers=3, stemStrideSizes=[1, 1]), IndexError), (dict(stemDim=10, stemKernelSize=1), __import__("macx").UnsupportedOptions),
    (dict(memDim=6, stemKernelSize=1), __import__("macx").UnsupportedOptions)])
def test_refusals(macx, flags, exc):
    with pytest.raises(exc):
        macx.Stem(cfg_of(**flags), H=4, W=4, inDim=8)
    with pytest.raises(exc):
        macx.GenericStem(cfg_of(**flags), H=4, W=4, inDim=8)
    with pytest.raises(macx.UnsupportedOptions):
        macx.GenericStem(cfg_of(), H=4, W=4, inDim=6)
