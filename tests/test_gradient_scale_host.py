"""No GPU: the inputs of tests/test_gpu_gradient_scale.py are well-conditioned, and its metrics do what they say.

The yardstick for "is this input fair" is the fp32 oracle against the fp64 oracle on the same inputs and parameters: every
per-question input-gradient error and every scaled parameter-gradient error of every case stays within a TENTH of the bound the
HIP kernels are held to.  A case that the plain fp32 restatement cannot do to 2e-5 would test the conditioning of the data, not
the kernels (the read unit's logit weights x 64 are such a case: 1.3e-4, not used)."""
import pytest
import torch

import gradient_scale_cases as gsc

CASES = gsc.cell_cases()


def test_per_question_err_has_no_floor_and_wants_exact_zeros():
    ref = torch.tensor([[1.0, -2.0], [2.0 ** -30, 0.0], [0.0, 0.0]])
    got = ref.clone()
    assert gsc.per_question_err(got, ref) == [0.0, 0.0, 0.0]
    got[1, 0] *= 1.5                       # wrong by half of a question 2^-31 of its neighbour: rel_err would report 2e-10
    got[0, 1] += 2.0 ** -10
    e = gsc.per_question_err(got, ref)
    assert e[0] == 2.0 ** -11 and e[1] == 0.5 and e[2] == 0.0
    got[2, 1] = 1e-30                      # a reference of exact zeros admits exact zeros only
    assert gsc.per_question_err(got, ref)[2] == gsc.INF
    got[2, 1] = -0.0
    assert gsc.per_question_err(got, ref)[2] == 0.0
    got[0, 0] = float("nan")
    assert gsc.per_question_err(got, ref)[0] == gsc.INF


def test_scaled_rel_err_floor_follows_the_unit():
    ref = torch.zeros(3)
    got = torch.tensor([0.0, 1e-13, 0.0])
    assert gsc.scaled_rel_err(got, ref, 1.0) == pytest.approx(1e-7)             # 1e-13 / (1e-6 * 1)
    assert gsc.scaled_rel_err(got, ref, 1e-6) == pytest.approx(1e-1)            # the same junk under 1e-6-scale gradients
    assert gsc.scaled_rel_err(got, ref, 1e-6, floor=5e-2) == pytest.approx(2e-6)
    ref = torch.tensor([4.0, 0.0, 0.0])
    got = torch.tensor([4.0, 1e-3, 0.0])
    assert gsc.scaled_rel_err(got, ref, 1.0) == pytest.approx(2.5e-4)           # above the floor: relative to the largest entry
    assert gsc.scaled_rel_err(torch.tensor([float("inf"), 0.0, 0.0]), ref, 1.0) == gsc.INF
    assert gsc.param_floor("MACnetwork/MACCell/read/inter2att/inter2logits/linearLayerlogits/biases/bias") == 5e-2
    assert gsc.param_floor("MACnetwork/MACCell/read/linearLayermemKbProj/weights/weight") == 1e-6


def test_bounds_are_the_suites_own():
    import test_gpu_cell
    assert (gsc.GRAD_TOL, gsc.FWD_TOL) == (test_gpu_cell.GRAD_TOL, test_gpu_cell.FWD_TOL)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_fp32_oracle_stays_a_tenth_inside_the_bound(macx, cid):
    case = CASES[cid]
    ref, e32 = gsc.cell_reference(macx, case)
    key, frac = gsc.worst(e32)
    print("gradient-scale host %s: fp32 oracle worst err / bound = %.3g (%s, err %.3g)" % (cid, frac, key, e32[key][0]))
    bad = {k: e for k, (e, bound) in e32.items() if k != "memory" and not e <= bound / 10}
    assert not bad, bad
    assert e32["memory"][0] < gsc.FWD_TOL / 5          # (the forward pass has its own tests; 2.2e-6 under 2^+-6 row scales)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    for k in gsc.INPUT_KEYS:                 # a question without a gradient has none in the reference, and only those
        for b in range(case.B):
            is_zero = not bool((ref[k][b] != 0).any())
            if b in case.zero_grad:
                assert is_zero, (k, b)
            elif k == "d_kb":
                assert not is_zero, (k, b)


@pytest.mark.parametrize("shape", ["launch", "chain"])
def test_homogeneity_leaves_out_less_than_a_percent(macx, shape):
    """2^-100 is far below every gradient of the unit-scale case times 2^-40: per tensor, fewer than 1 % of the elements of the
    fp64 reference are left out of the bit comparison (exact zeros -- padded words, dropped columns -- are compared: 0 * 2^k = 0)."""
    ref, _ = gsc.cell_reference(macx, CASES["unit-" + shape])
    for k in gsc.HOMOGENEITY_K:
        for key, t in ref.items():
            if key == "memory":
                continue
            nz = t[t != 0]
            frac = gsc.excluded_fraction(nz, k) * nz.numel() / max(t.numel(), 1)
            assert frac < 0.01, (key, k, frac)
            assert float(t.abs().max()) * 2.0 ** k < 2.0 ** 100, (key, k)        # and nothing near fp32's overflow


def test_stem_inputs_are_fair(macx):
    """The stem cases under the fp32 conv2d restatement: forward per image, kernel gradients with the scaled floor."""
    cfg, stem, img, dout = gsc.stem_case(macx, image_scales=gsc.STEM_FWD_SCALES)
    r64, r32 = [gsc.oracle_stem(cfg, stem, img, dout, dt) for dt in (torch.float64, torch.float32)]
    e = gsc.per_question_err(r32["out"], r64["out"])
    print("gradient-scale host stem forward: fp32 oracle per image", e)
    assert max(e) <= gsc.STEM_FWD_TOL / 5          # (1.1e-6 on image 0, the unit-scale one; the scaled images are below it)
    cfg, stem, img, dout = gsc.stem_case(macx, dout_scales=gsc.STEM_BWD_SCALES)
    r64, r32 = [gsc.oracle_stem(cfg, stem, img, dout, dt) for dt in (torch.float64, torch.float32)]
    e = {k: gsc.scaled_rel_err(r32[k], r64[k], 1.0) for k in r64 if k.startswith("param:")}
    print("gradient-scale host stem backward: fp32 oracle", e)
    assert max(e.values()) <= gsc.GRAD_TOL / 10
    cfg, stem, img, dout = gsc.stem_case(macx, zero_dout=True)
    r64 = gsc.oracle_stem(cfg, stem, img, dout, torch.float64)
    assert all(not bool((r64[k] != 0).any()) for k in r64 if k.startswith("param:"))


def test_tower_inputs_are_fair(macx):
    cfg, net, img, q, lengths, ans = gsc.tower_case(macx)
    r64, r32 = [gsc.oracle_tower(cfg, net, img, q, lengths, ans, dt) for dt in (torch.float64, torch.float32)]
    e = {k: gsc.scaled_rel_err(r32[k], r64[k], 1.0, floor=gsc.tower_floor(k)) for k in r64 if k.startswith("param:")}
    k = max(e, key=e.get)
    print("gradient-scale host tower: fp32 oracle worst", k, e[k])
    assert e[k] <= gsc.TOWER_TOL / 10
