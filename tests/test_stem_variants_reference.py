"""CPU: tests/stem_variants_ref.py (the fp64 restatement of MACnet.stem for every stem option) against the reference's own
model.MACnet.stem / ops.CNNLayer / ops.cnn / ops.addLocation / ops.linear, run unmodified on the TF stand-in of tests/tf1_shim
(tests/ref_exec.py).  The stand-in's conv2d covers odd kernels at stride 1 only; this module installs TF's general SAME
convolution into it for its own tests (monkeypatch), the shim's file is left as it is.

Checked: the knowledge base and every gradient (images and variables) to 1e-12, variable names / shapes / creation order, the
dropout draws (one per layer input), and the exceptions the reference raises (stemBN, stemGridRnn, short per-layer lists).

Where MACX_REFERENCE_DIR is absent the reference's results are replayed from tests/golden/stem_variants/ (recorded by a live
session with MACX_RECORD_REFERENCE=1, as tests/ref_exec.py does for its calls).
"""
import builtins
import os
import sys

import numpy as np
import pytest
import torch

import ref_exec as rx
import stem_variants_ref as sv

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem_variants")
Bs, H, W, C, D, SD = 2, 5, 3, 8, 8, 12

VARIANTS = {
    "default": [],
    "one_layer_k1": ["--stemNumLayers", "1", "--stemKernelSize", "1"],
    "zero_layers": ["--stemNumLayers", "0"],
    "three_layers": ["--stemNumLayers", "3"],
    "k5": ["--stemKernelSize", "5"],
    "even_k_stride2": ["--stemKernelSizes", "2", "4", "--stemStrideSizes", "2", "2"],
    "strides_2_1": ["--stemStrideSizes", "2", "1"],
    "k4_stride3": ["--stemKernelSizes", "4", "1", "--stemStrideSizes", "3", "1"],
    "stem_dim": ["--stemDim", "4"],
    "loc_L": ["--locationAware"],
    "loc_PE": ["--locationAware", "--locationType", "PE", "--locationDim", "3", "--locationBias", "2.0"],
    "linear": ["--stemLinear"],
    "elu": ["--relu", "ELU", "--stemKernelSize", "2"],
}
RAISES = {
    "bn": ["--stemBN"],
    "grid_rnn": ["--stemGridRnn"],
    "short_kernel_list": ["--stemKernelSizes", "3"],
    "short_stride_list": ["--stemNumLayers", "3", "--stemStrideSizes", "1", "1"],
}


def parse(flags):
    """the reference's parser (config.py:95-428) over the command line, without a flag file; a namespace copy of the result"""
    from types import SimpleNamespace
    M = rx.load()
    M["config"].config.__dict__.clear()
    argv = sys.argv
    try:
        sys.argv = ["main.py", "--memDim", str(D), "--stemDim", str(SD)] + flags
        M["config"].parseArgs()
    finally:
        sys.argv = argv
    return M["config"].config, SimpleNamespace(**vars(M["config"].config))


def local_config(flags):
    """the same flags as a plain namespace, for the replay (the parser's types: ints, floats, lists, store_true)"""
    from types import SimpleNamespace
    cfg = SimpleNamespace(memDim=D, stemDim=SD, stemDropout=0.82, relu="STD")
    i = 0
    while i < len(flags):
        name = flags[i][2:]
        vals = []
        i += 1
        while i < len(flags) and not flags[i].startswith("--"):
            vals.append(flags[i])
            i += 1
        conv = lambda v: float(v) if "." in v else (int(v) if v.lstrip("-").isdigit() else v)   # noqa: E731
        if name in ("stemKernelSizes", "stemStrideSizes"):
            setattr(cfg, name, [int(v) for v in vals])
        else:
            setattr(cfg, name, conv(vals[0]) if vals else True)
    return cfg


def images_for(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bs, H, W, C, generator=g, dtype=torch.float64)


def cotangent(shape, seed=9):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def run_live(monkeypatch, flags, train):
    """MACnet.stem on the stand-in: dict(kb, variables, draws, grads) or dict(raise=name)"""
    M = rx.load()
    tf, model = M["tf"], M["model"]
    monkeypatch.setattr(tf.nn, "conv2d", lambda inp, filter=None, strides=None, padding="SAME", name=None:   # noqa: A002
                        sv.conv2d_same(inp, filter, strides[1]))
    cfg, _ = parse(flags)
    keep = cfg.stemDropout if train else 1.0
    tf.shim_reset(dtype=torch.float64, seed=3, require_grad=True)
    img = tf.wrap(images_for().clone()).requires_grad_(True)
    fake = __import__("types").SimpleNamespace(dropouts={"stem": keep}, batchSize=Bs, H=H, W=W,
                                               batchNorm={"decay": cfg.bnDecay, "train": True})   # model.py:96
    try:
        kb = model.MACnet.stem(fake, img, C, cfg.memDim)
    except Exception as e:                      # noqa: BLE001 -- the reference's exception is its result
        return {"raise": type(e).__name__}
    variables = dict(tf.state.variables)
    leaves = [img] + list(variables.values())
    grads = torch.autograd.grad((kb * cotangent(kb.shape)).sum(), leaves)
    return {"kb": kb.detach().clone().as_subclass(torch.Tensor), "names": list(variables),
            "variables": [v.detach().clone().as_subclass(torch.Tensor) for v in variables.values()],
            "draws": [u.clone().as_subclass(torch.Tensor) for _, u in tf.state.draws],
            "grads": [g.clone().as_subclass(torch.Tensor) for g in grads], "keep": keep}


def _fixture(name):
    return os.path.join(FIXTURES, name + ".npz")


def reference(monkeypatch, name, flags, train):
    """the live result (recorded with MACX_RECORD_REFERENCE=1) or the recorded one"""
    key = "%s_%s" % (name, "train" if train else "eval")
    if rx.available():
        res = run_live(monkeypatch, flags, train)
        if rx.RECORD:
            os.makedirs(FIXTURES, exist_ok=True)
            arrs = {"raise": np.array(res.get("raise", ""))}
            if "raise" not in res:
                arrs.update(kb=res["kb"].numpy(), names=np.array(res["names"]), keep=np.array(res["keep"]))
                for i, v in enumerate(res["variables"]):
                    arrs["var_%d" % i] = v.numpy()
                for i, u in enumerate(res["draws"]):
                    arrs["draw_%d" % i] = u.numpy()
                for i, g in enumerate(res["grads"]):
                    arrs["grad_%d" % i] = g.numpy()
            np.savez_compressed(_fixture(key), **arrs)
        return res
    path = _fixture(key)
    if not os.path.exists(path):
        raise AssertionError("no recorded reference run %s (record with MACX_REFERENCE_DIR=<upstream checkout> "
                             "MACX_RECORD_REFERENCE=1)" % path)
    with np.load(path) as z:
        if str(z["raise"]):
            return {"raise": str(z["raise"])}
        t = lambda k: torch.from_numpy(z[k].copy())        # noqa: E731
        n = len(z["names"])
        return {"kb": t("kb"), "names": [str(s) for s in z["names"]], "variables": [t("var_%d" % i) for i in range(n)],
                "draws": [t("draw_%d" % i) for i in range(sum(k.startswith("draw_") for k in z.files))],
                "grads": [t("grad_%d" % i) for i in range(n + 1)], "keep": float(z["keep"])}


def config_for(flags):
    return parse(flags)[1] if rx.available() else local_config(flags)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_restatement_reproduces_the_reference_stem(monkeypatch, name, train):
    flags = VARIANTS[name]
    ref = reference(monkeypatch, name, flags, train)
    assert "raise" not in ref, ref
    cfg = config_for(flags)
    # variables: names, shapes, creation order
    assert [(n, tuple(v.shape)) for n, v in zip(ref["names"], ref["variables"])] == \
        [(n, tuple(s)) for n, s in sv.variable_names(cfg, C, D)]
    linear, loc, layers = sv.plan(cfg, C, D)
    params = {n: v.clone().requires_grad_(True) for n, v in zip(ref["names"], ref["variables"])}
    keep = ref["keep"]
    masks = None
    if train and not linear:             # tf.nn.dropout draws once per layer input, in layer order (ops.cnn, ops.py:400)
        hh, ww = H, W
        shapes = []
        for _, (k, _, cin, _), s in layers:
            shapes.append((Bs, hh, ww, cin))
            hh, ww = -(-hh // s), -(-ww // s)
        assert [tuple(u.shape) for u in ref["draws"]] == shapes
        masks = [torch.floor(keep + u) for u in ref["draws"]]
    else:
        assert ref["draws"] == []
    img = images_for().requires_grad_(True)
    kb = sv.stem(cfg, img, params, D, keep=keep, masks=masks)
    assert tuple(kb.shape) == tuple(ref["kb"].shape)
    assert float((kb.detach() - ref["kb"]).abs().max()) <= 1e-12
    (kb * cotangent(kb.shape)).sum().backward()
    got = [img.grad] + [params[n].grad for n in ref["names"]]
    for n, a, b in zip(["images"] + ref["names"], got, ref["grads"]):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), n


@pytest.mark.parametrize("name", sorted(RAISES))
def test_refused_stems_raise_what_the_reference_raises(monkeypatch, name):
    flags = RAISES[name]
    ref = reference(monkeypatch, name, flags, False)
    assert ref.get("raise") in ("KeyError", "NameError", "IndexError"), ref
    with pytest.raises(getattr(builtins, ref["raise"])):
        sv.plan(config_for(flags), C, D)


@pytest.mark.parametrize("k,s", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (4, 2), (5, 1), (4, 3), (6, 4)])
def test_same_conv_is_tf_same_padding(k, s):
    """the SAME convolution used above, against its definition: out[oy, ox] = sum over taps of x[oy s - pad_top + ky, ..]
    with pad_top = pad_total // 2, zeros outside"""
    g = torch.Generator().manual_seed(k * 10 + s)
    x = torch.randn(2, 7, 5, 3, generator=g, dtype=torch.float64)
    w = torch.randn(k, k, 3, 4, generator=g, dtype=torch.float64)
    Ho, Wo = -(-7 // s), -(-5 // s)
    pt = max((Ho - 1) * s + k - 7, 0) // 2
    pl = max((Wo - 1) * s + k - 5, 0) // 2
    want = torch.zeros(2, Ho, Wo, 4, dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = oy * s - pt + ky, ox * s - pl + kx
                    if 0 <= iy < 7 and 0 <= ix < 5:
                        want[:, oy, ox] += x[:, iy, ix] @ w[ky, kx]
    assert float((sv.conv2d_same(x, w, s) - want).abs().max()) < 1e-12
