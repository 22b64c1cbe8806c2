"""CPU half of test_gpu_side_kernels.py: the fused encoder's width limit through the loaded library, the oracle's length-0 rows, and
the proof that the optimizer bounds (test_gpu_side_kernels.opt_bounds) are fair and sharp:

* fair: a numpy fp32 evaluation of the same formulas -- every operation rounded once, the norm summed pairwise by np.sum, another
  order than the kernel's -- stays within HALF of every bound on every size x gradient scale the GPU test runs.  For p and ema
  "half" applies to what the bound holds beyond the result's own last rounding: a correctly rounded fp32 value is up to half an
  ulp off by itself, so the fp32 evaluation reaches 0.9 - 0.998 of the WHOLE p and ema bounds, whose leading term is that half ulp;
* sharp: a copy of that evaluation with ONE element's update scaled by 1 + 2^-10 is rejected on every combination, and one computed
  without eps wherever eps is more than rounding noise (see test_bounds_reject_a_dropped_eps)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mac_oracle as mo
from test_gpu_side_kernels import OPT_KINDS, OPT_SIZES, opt_bounds, opt_case, opt_eval, opt_lr_t, opt_ratios


# ---- the fused encoder's width limit ------------------------------------------------------------------------------------------
def test_encoder_sizing_refuses_widths_past_the_lds(macx):
    L = macx._lib.lib()
    sh = lambda h: C.byref(macx._lib.MacxEncShapes(B=2, S=3, V=9, E=20, h=h, b0=0))
    for h in (128, 256, 384, 512):                        # rnn_step_bwd_lds(512, 4) = 149,760 B <= 163,840 B
        assert L.macx_encoder_saved_floats(sh(h)) > 0 and L.macx_encoder_ws_floats(sh(h)) > 0, h
    for h in (640, 768, 1024):                            # rnn_step_bwd_lds(640, 4) = 182,528 B
        assert L.macx_encoder_saved_floats(sh(h)) == 0 and L.macx_encoder_ws_floats(sh(h)) == 0, h
    for h in (0, 64, 192, 520):                           # not a multiple of 128: refused as before
        assert L.macx_encoder_saved_floats(sh(h)) == 0 and L.macx_encoder_ws_floats(sh(h)) == 0, h
    # forward and backward refuse the width before they look at a pointer (MACX_EUNSUPPORTED, not the null operands' MACX_EINVAL)
    assert L.macx_encoder_forward(sh(640), 1.0, 1.0, 0, None, None, None, None, None, None, 0, None) == macx._lib.MACX_EUNSUPPORTED
    assert L.macx_encoder_backward(sh(640), 1.0, 1.0, 0, None, None, None, None, 0, None, 0, None, None, None,
                                   None) == macx._lib.MACX_EUNSUPPORTED
    assert L.macx_encoder_forward(sh(512), 1.0, 1.0, 0, None, None, None, None, None, None, 0, None) == macx._lib.MACX_EINVAL


def test_encoder_class_by_width(macx):
    wide = lambda d: mo.flag_file_config("args", ctrlDim=d, memDim=d, attDim=d, encDim=d, wrdEmbDim=8)
    assert type(macx.QuestionEncoder(wide(1280), vocab=5)) is macx.GenericQuestionEncoder
    assert type(macx.QuestionEncoder(wide(1024), vocab=5)) is macx.QuestionEncoder
    assert macx.encoder.FUSED_H_MAX == 512
    with pytest.raises(macx.UnsupportedOptions, match="512"):
        macx.encoder._check_fused(wide(1280))
    macx.encoder._check_fused(wide(1024))


def test_oracle_rows_of_a_length_0_question_are_exact_zeros():
    """What the GPU test holds the kernels to: dynamic_rnn emits zeros and copies the ZERO initial state through for a sequence of
    length 0, whatever the biases are -- questionCntxWords rows and the vecQuestions row are exactly 0.0, and nothing flows back."""
    E, h, V, B, S = 6, 8, 9, 4, 5
    cfg = mo.flag_file_config("args", ctrlDim=2 * h, memDim=2 * h, attDim=2 * h, encDim=2 * h, wrdEmbDim=E)
    vs = mo.VarStore(generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    L = torch.tensor([S, 0, 2, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(1)
    q = torch.randint(1, V + 1, (B, S), generator=g) * (torch.arange(S).unsqueeze(0) < L.unsqueeze(1))
    mo.question_encoder(cfg, vs, q, L, V)                                          # (declares the variables)
    for d in ("fw", "bw"):
        vs.params["encoder/birnnLayer/bidirectional_rnn/%s/basic_lstm_cell/bias" % d] = torch.rand(4 * h, generator=g, dtype=torch.float64) - 0.5
    for t in vs.params.values():
        t.requires_grad_(True)
    w, v = mo.question_encoder(cfg, vs, q, L, V)
    wd, vd = w.detach(), v.detach()
    for b in (1, 3):
        assert float(wd[b].abs().max()) == 0.0 and float(vd[b].abs().max()) == 0.0
    assert float(wd[0].abs().min()) > 0.0 and float(vd[2].abs().min()) > 0.0 and float(wd[2, 2:].abs().max()) == 0.0
    # the gradient of the empty questions' outputs reaches no parameter
    (w[1].sum() + w[3].sum() + v[1].sum() + v[3].sum()).backward()
    assert all(t.grad is None or float(t.grad.abs().max()) == 0.0 for t in vs.params.values())


# ---- the optimizer bounds -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opt_runs(macx):
    """{(n, kind): (case, lr_t, fp64 reference, bounds, fp32 evaluation)}, computed once"""
    out = {}
    for n in OPT_SIZES:
        for kind in OPT_KINDS:
            c = opt_case(n, kind)
            lr_t = opt_lr_t(macx, c)
            ref = opt_eval(c, lr_t, np.float64)
            out[n, kind] = (c, lr_t, ref, opt_bounds(c, lr_t, ref), opt_eval(c, lr_t, np.float32))
    return out


def test_cases_are_live(opt_runs):
    """every term of every formula matters: the clip is on one side where named, neither moment swamps its gradient term, the update
    is not lost in p, and the EMA moves"""
    for (n, kind), (c, lr_t, ref, bounds, _) in opt_runs.items():
        norm = float(ref["norm"])
        assert (norm > 8.0) == (kind in ("clip", "off")), (n, kind, norm)
        b1, b2 = float(np.float32(c["beta1"])), float(np.float32(c["beta2"]))
        for grad_term, old_term in (((1 - b1) * np.abs(ref["gs"]), b1 * np.abs(c["m"])), ((1 - b2) * ref["gs"] ** 2, b2 * c["v"])):
            q = np.median(grad_term) / np.median(old_term)
            assert 1e-4 < q < 1e4, (n, kind, q)
        assert np.median(np.abs(ref["upd"])) > 2.0 ** -20 * np.median(np.abs(c["p"])), (n, kind)
        assert (c["decay"] < 0) == (kind == "off")
        if kind != "off":
            assert np.median(np.abs(ref["ema"] - c["ema"])) > 0


def test_bounds_hold_an_fp32_evaluation_within_half(opt_runs):
    bad = {}
    for (n, kind), (c, lr_t, ref, bounds, f32) in opt_runs.items():
        assert set(bounds) == ({"norm", "p", "m", "v", "final"} | ({"ema"} if kind != "off" else set()))
        ratios = opt_ratios(f32, ref, bounds, beyond_final=0.5)
        print("n %7d %-7s " % (n, kind) + ", ".join("%s %.3f" % (k, r) for k, (r, _) in ratios.items()))
        bad.update({(n, kind, k): r for k, (r, _) in ratios.items() if not r <= 1.0})
    assert not bad, bad


def test_bounds_reject_one_update_off_by_2_to_the_minus_10(opt_runs):
    for (n, kind), (c, lr_t, ref, bounds, f32) in opt_runs.items():
        i = int(np.argmax(np.abs(ref["upd"]) / bounds["p"]))               # the element whose update the bound sees best
        mut = dict(f32, p=f32["p"].copy())
        mut["p"][i] = c["p"][i] - f32["upd"][i] * np.float32(1 + 2.0 ** -10)
        r, at = opt_ratios(mut, ref, bounds)["p"]
        print("n %7d %-7s element %d: error / bound %.1f" % (n, kind, i, r))
        assert r > 1.0 and at == i, (n, kind, r)


def test_bounds_reject_a_dropped_eps(opt_runs, macx):
    """eps = 1e-8 against sqrt(v): at the 2^-30 scale sqrt(v) ~ 1e-9, eps IS the denominator; at 0.01 the elements whose sqrt(v) is
    a few 1e-4 move by ~1e-4 of an update that is itself large there.  At scale ~1 (clip at small n, clip off) eps / sqrt(v) is
    below the rounding of the quotient on most draws -- no honest bound can see it, so those rows are printed, not asserted."""
    for (n, kind), (c, lr_t, ref, bounds, f32) in opt_runs.items():
        mut = opt_eval(c, lr_t, np.float32, drop_eps=True)
        r = max(v[0] for v in opt_ratios(mut, ref, bounds).values())
        print("n %7d %-7s worst error / bound without eps: %.2f" % (n, kind, r))
        if kind in ("x0.01", "x2^-30"):
            assert r > 1.0, (n, kind, r)
