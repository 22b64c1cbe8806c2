"""The host side of the whole-tower HIP graph classes (macx.CapturedTowerForward / CapturedTowerTrainStep): the exports they stand
on, the keywords that default to the behaviour of before, the refusals, and the optimizer's host-computed rate.  No GPU."""
import ctypes as C
import inspect
import math

import pytest
import torch

W_EXPORTS = ("macx_encoder_forward_w", "macx_encoder_backward_w", "macx_stem_forward_w", "macx_stem_backward_w",
             "macx_output_forward_w", "macx_output_backward_w")
SMALL = dict(netLength=3, memDim=256, ctrlDim=256, attDim=256, encDim=256, wrdEmbDim=20, outClassifierDims=[128])


def small_net(macx, **over):
    known = vars(macx.configs.default_config())
    cfg = macx.configs.flag_file_config("args", **dict(SMALL, **{k: v for k, v in over.items() if k in known}))
    for k, v in over.items():                 # (flags the modules read with their own defaults, e.g. the stem's)
        setattr(cfg, k, v)
    return macx.MACNet(cfg, vocab=11, H=5, W=5, imageInDim=128, answerWordsNum=28, generator=torch.Generator().manual_seed(0))


def test_new_symbols_are_exported_with_signatures(macx):
    L = macx._lib.lib()
    for n in W_EXPORTS + ("macx_adam_ema_step_p", "macx_gather_flat"):
        assert n in macx._lib.EXPORTS
        f = getattr(L, n)
        assert f.argtypes is not None and f.restype is C.c_int, n
    # a _w entry point is the plain one plus the device word in front of the stream
    for n in W_EXPORTS:
        plain, w = getattr(L, n[:-2]).argtypes, getattr(L, n).argtypes
        assert list(w) == list(plain[:-1]) + [C.c_void_p, plain[-1]], n
    # macx_adam_ema_step_p: lr and step give way to one device pointer
    plain, p = L.macx_adam_ema_step.argtypes, L.macx_adam_ema_step_p.argtypes
    assert len(p) == len(plain) - 1 and p[6] is C.c_void_p and plain[6] is C.c_float and plain[10] is C.c_int
    assert list(L.macx_gather_flat.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert C.sizeof(macx._lib.MacxGatherEntry) == 24          # {const float* src; uint64_t dst_offset; uint64_t count;}
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5


def test_new_keywords_default_to_the_old_behaviour(macx):
    for cls in (macx.QuestionEncoder, macx.Stem, macx.OutputClassifier, macx.MACNetCore, macx.MACNet,
                macx.GenericQuestionEncoder, macx.GenericStem, macx.GenericOutputClassifier):
        assert inspect.signature(cls.forward).parameters["mask_word"].default is None, cls
    assert inspect.signature(macx.optim.FlatAdamEMA.step).parameters["device_lr"].default is False
    assert inspect.signature(macx.optim.FlatAdamEMA.step).parameters["flat_grad"].default is None
    assert inspect.signature(macx.dp.TowerBuckets.__init__).parameters["fused_gather"].default is False
    sig = inspect.signature(macx.CapturedTowerForward.__init__).parameters
    assert [sig[k].default for k in ("H", "W", "imageInDim", "warmup", "verify", "check_every")] == [14, 14, 1024, 2, True, 0]
    sig = inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters
    assert list(sig)[1:9] == ["net", "opt", "bucket", "B", "S", "H", "W", "imageInDim"]
    assert [sig[k].default for k in ("seed", "warmup", "verify", "check_every")] == [0, 2, True, 0]


def test_captured_tower_classes_need_the_device(macx):
    net = small_net(macx)
    assert type(net.enc) is macx.QuestionEncoder and type(net.stem) is macx.Stem and type(net.out) is macx.OutputClassifier
    with pytest.raises(RuntimeError, match="HIP device"):
        macx.CapturedTowerForward(net, 6, 7, H=5, W=5, imageInDim=128)
    with pytest.raises(RuntimeError, match="HIP device"):
        macx.CapturedTowerTrainStep(net, None, None, 6, 7, H=5, W=5, imageInDim=128)


@pytest.mark.parametrize("over, module", [(dict(encBi=False), "enc"), (dict(stemKernelSize=1), "stem"),
                                          (dict(outClassifierDims=[128, 128]), "out")])
def test_captured_tower_classes_refuse_generic_modules(macx, over, module):
    net = small_net(macx, **over)
    assert type(getattr(net, module)).__name__.startswith("Generic")
    with pytest.raises(macx.UnsupportedOptions, match="net." + module):
        macx.CapturedTowerForward(net, 6, 7, H=5, W=5, imageInDim=128)
    with pytest.raises(macx.UnsupportedOptions, match="net." + module):
        macx.CapturedTowerTrainStep(net, None, None, 6, 7, H=5, W=5, imageInDim=128)


def test_generic_modules_refuse_a_mask_word(macx):
    word = torch.zeros(1, dtype=torch.int32)
    enc = small_net(macx, encBi=False).enc
    with pytest.raises(macx.UnsupportedOptions, match="mask word"):
        enc(torch.zeros(2, 3, dtype=torch.int32), torch.ones(2, dtype=torch.int32), mask_word=word)
    stem = small_net(macx, stemKernelSize=1).stem
    with pytest.raises(macx.UnsupportedOptions, match="mask word"):
        stem(torch.zeros(2, 25, 128), mask_word=word)
    out = small_net(macx, outClassifierDims=[128, 128]).out
    with pytest.raises(macx.UnsupportedOptions, match="mask word"):
        out(torch.zeros(2, 256), torch.zeros(2, 256), mask_word=word)
    # the plan cell: the reference's default option set has no fused cell
    cfg = macx.configs.default_config(netLength=2, memDim=128, ctrlDim=128, attDim=128)
    core = macx.MACNetCore(cfg, H=5, W=5, imageInDim=128)
    assert not isinstance(core.cell, macx.MACCellParams)
    with pytest.raises(macx.UnsupportedOptions, match="mask word"):
        core(torch.zeros(2, 25, 128), torch.zeros(2, 128), torch.zeros(2, 3, 128), torch.ones(2, dtype=torch.int32), mask_word=word)


def test_advance_writes_the_bias_corrected_rate(macx):
    """advance(): t += 1 and lr_t = (float)(lr * sqrt(1 - b2^t) / (1 - b1^t)) in double from the CURRENT lr -- lr, b1, b2 as the C
    floats macx_adam_ema_step receives them.  (The optimizer itself needs device parameters; its host half does not.)"""
    opt = object.__new__(macx.optim.FlatAdamEMA)
    opt.lr, opt.beta1, opt.beta2, opt.t = 1e-4, 0.9, 0.999, 0
    opt.lr_t = torch.zeros(1, dtype=torch.float32)
    f32 = lambda x: C.c_float(x).value
    for t in range(1, 6):
        if t == 3:
            opt.lr = 0.5e-4
        assert opt.advance() == t and opt.t == t
        want = f32(opt.lr) * math.sqrt(1.0 - f32(0.999) ** t) / (1.0 - f32(0.9) ** t)
        assert float(opt.lr_t[0]) == f32(want), t
        # ... which is the textbook rate up to the float rounding of beta2 (2^-24 relative) seen through 1 - b2^t >= 1e-3 and the
        # square root: at most 0.5 * 2^-24 * 0.999 / 1e-3 = 3e-5 (beta1's share is 5e-7, the final rounding 6e-8)
        assert abs(float(opt.lr_t[0]) / (opt.lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)) - 1.0) < 3.2e-5
