"""-m gpu: the backward pass at the gradient scales training produces (tests/gradient_scale_cases.py has the cases, the metrics and
the reasoning; tests/test_gradient_scale_host.py shows that the inputs are fair).

Cross-entropy hands every question a gradient of its own magnitude, attention hands every knowledge-base row one, padding hands
exact zeros.  The H2 family (two fp16 planes + power-of-two block exponents) is where scale decides: the per-row exponents of
read_att_bwd_h2_kernel and the chain kernels, the row minima of h2_emin_list_kernel / h2_emin_final, the per-question minima of
sb_h2_kernel / sb_h2w_kernel, the fp16 row factor pk_pow2_f16(da + dg) (0 below 2^-24), the clamps H2_E_MIN/MAX and H2_WE_LO/HI,
and the one exponent per tensor of the stem's kb_gemm3h_kernel / wgrad_split_kernel<WgFp16x2>.  Every route with exponent logic of its own runs
here against the fp64 oracle with

  * input gradients (d_kb, d_words, d_vq) PER QUESTION, no absolute floor, exact zeros where the reference has them;
  * parameter gradients with floors that scale with the case's gradients;

at the suite's own GRAD_TOL / FWD_TOL.  Every test prints its largest error / bound and the ratio of that error to the fp32
oracle's on the same entry, and the module ends with the largest of each item (`-s` shows them)."""
import pytest
import torch

import gradient_scale_cases as gsc
import test_gpu_cell

pytestmark = pytest.mark.gpu

CASES = gsc.cell_cases()
FAMILIES = ("h2", "split", "native")
_FIGURES = {}          # item -> {test id: (err / bound, key, err / fp32 oracle's err)}
_BASE = {}             # (shape, family) -> the k = 0 run of the homogeneity tests


@pytest.fixture(scope="module", autouse=True)
def figures():
    assert (gsc.GRAD_TOL, gsc.FWD_TOL) == (test_gpu_cell.GRAD_TOL, test_gpu_cell.FWD_TOL)
    yield
    _BASE.clear()
    for item, v in sorted(_FIGURES.items()):
        frac, key, ratio = max(v.values(), key=lambda t: t[0])
        print("gradient-scale %s: largest err / bound = %.3g (%s), %.3g x the fp32 oracle's" % (item, frac, key, ratio))
    _FIGURES.clear()


def record(item, tid, errs, e32):
    """print and keep the entry closest to its bound, with the fp32 oracle's error on the same entry"""
    key, frac = gsc.worst(errs)
    base = e32.get(key, (0.0, 1.0))[0]
    ratio = errs[key][0] / base if base > 0 else gsc.INF
    print("gradient-scale %s %s: worst err / bound = %.3g (%s, err %.3g), %.3g x the fp32 oracle's" % (item, tid, frac, key, errs[key][0], ratio))
    _FIGURES.setdefault(item, {})[tid] = (frac, key, ratio)


def run_hip(macx, dev, case, gemm, tune=None, k=0):
    """One training-mode run of the cell on the case's inputs with d_memory, d_control times 2^k -> the flat result"""
    params = case.params(macx).to(dev)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (case.vq, case.words, case.kb)]
    cfg = case.cfg
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=case.lengths.to(dev),
                        knowledgeBase=kbd, memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout,
                        writeDropout=cfg.writeDropout, batchSize=case.B, train=True, config=cfg, params=params, seed=case.seed,
                        gemm=gemm, tune=tune)
    state = cell.run()
    f = 2.0 ** k
    ((state.memory * (case.dmem * f).to(dev)).sum() + (state.control * (case.dctl * f).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    res = {"memory": state.memory.detach().cpu(), "d_kb": kbd.grad.cpu(), "d_words": wd.grad.cpu(), "d_vq": vqd.grad.cpu()}
    ref_shapes = params.to_reference_dict()
    for fld, lst in macx.params.reference_names(cfg, case.p).items():
        if fld not in params.fields:
            continue
        g = getattr(params, fld).grad
        assert g is not None, fld
        for refname, idx in lst:
            res["param:" + refname] = (g if idx is None else g[idx]).reshape(ref_shapes[refname].shape).cpu()
    return res


def hold(macx, item, tid, case, got, k=0):
    """got against the fp64 oracle (times 2^k) by the metrics of gradient_scale_cases, at GRAD_TOL / FWD_TOL"""
    ref, e32 = gsc.cell_reference(macx, case)
    assert set(got) == set(ref), set(got) ^ set(ref)
    ref = gsc.scaled(ref, k)
    errs = gsc.errors(got, ref, case.unit * 2.0 ** k)
    record(item, tid, errs, e32)
    per_q = {key: gsc.per_question_err(got[key], ref[key]) for key in gsc.INPUT_KEYS}
    key = max(per_q, key=lambda key: max(per_q[key]))
    print("gradient-scale %s %s: input gradients per question, worst %s %s (fp32 oracle's worst question %.3g)"
          % (item, tid, key, ["%.3g" % e for e in per_q[key]], e32[key][0]))
    bad = {key: e for key, (e, bound) in errs.items() if not e < bound}
    assert not bad, bad


def tune_id(tune):
    return "default" if not tune else ",".join("%s=%d" % kv for kv in sorted(tune.items()))


# ---- 1. per-question gradient scales 2^{0, -10, -20, -30}
ITEM1 = ([("scales-" + shape, "h2", None) for shape in gsc.SHAPES] +
         [("scales-" + shape, fam, None) for shape in ("launch", "chain") for fam in ("split", "native")] +
         [("scales-chain", "h2", {key: v}) for key, v in (("sb_defer", 0), ("sb_wide", 0), ("chain", 0), ("dkb_fill", 0), ("wgrad_pipe", 2))] +
         [("scales-permuted-chain", "h2", None)])


@pytest.mark.parametrize("cid,gemm,tune", ITEM1, ids=["%s-%s-%s" % (c, g, tune_id(t)) for c, g, t in ITEM1])
def test_per_question_gradient_scales(macx, dev, cid, gemm, tune):
    """Questions whose loss gradients are 2^-10, 2^-20 and 2^-30 of their neighbour's keep their own relative accuracy in d_kb,
    d_words and d_vq, on every kernel family and on every route with exponent-minimum or factor code of its own."""
    case = CASES[cid]
    got = run_hip(macx, dev, case, gemm, tune)
    hold(macx, "1-scales", "%s-%s-%s" % (cid, gemm, tune_id(tune)), case, got)


# ---- 2. exactly-zero questions without kb_lengths
ITEM2 = ([("zeros-" + shape, fam, None) for shape in ("launch", "chain") for fam in FAMILIES] +
         [("zeros-chain", "h2", {"sb_defer": 0}), ("zeros-chain", "h2", {"sb_wide": 0})])


@pytest.mark.parametrize("cid,gemm,tune", ITEM2, ids=["%s-%s-%s" % (c, g, tune_id(t)) for c, g, t in ITEM2])
def test_questions_with_exactly_zero_gradient(macx, dev, cid, gemm, tune):
    """d_memory[b] = d_control[b] = 0 for b in {1, 3}, the others at 1e-6: the dead questions' input gradients are exact zeros,
    everything is finite, and the live questions and the parameters are held as everywhere here (unit 1e-6).  An all-zero gradient
    row that took block exponent 0 instead of H2_E_MAX would scale the live rows of its contraction to nothing."""
    case = CASES[cid]
    got = run_hip(macx, dev, case, gemm, tune)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    for key in gsc.INPUT_KEYS:
        for b in gsc.ZERO_QUESTIONS:
            assert not bool((got[key][b] != 0).any()), (key, b)
    hold(macx, "2-zeros", "%s-%s-%s" % (cid, gemm, tune_id(tune)), case, got)


# ---- 3. homogeneity in the loss scale
@pytest.mark.parametrize("k", gsc.HOMOGENEITY_K)
@pytest.mark.parametrize("gemm", ["h2", "native"])
@pytest.mark.parametrize("shape", ["launch", "chain"])
def test_backward_is_homogeneous_in_the_loss_scale(macx, dev, shape, gemm, k):
    """The backward pass is linear in (d_memory, d_control), and a power of two is exact in fp32, in fp16 and in the block
    exponents: the run on d * 2^k is BIT FOR BIT the k = 0 run times 2^k, on every element with |base| * 2^k >= 2^-100 (fewer
    than 1 % of a tensor lie below; exact zeros are compared), and it meets the oracle times 2^k with unit = 2^k."""
    case = CASES["unit-" + shape]
    if (shape, gemm) not in _BASE:
        _BASE[(shape, gemm)] = run_hip(macx, dev, case, gemm)
    base = _BASE[(shape, gemm)]
    got = run_hip(macx, dev, case, gemm, k=k)
    assert torch.equal(got["memory"], base["memory"])
    bad = {}
    for key, t in base.items():
        if key == "memory":
            continue
        keep = (t == 0) | (t.double().abs() * 2.0 ** k >= gsc.HOMOGENEITY_FLOOR)
        assert float((~keep).double().mean()) < 0.01, (key, float((~keep).double().mean()))
        want = t * 2.0 ** k
        if not torch.equal(got[key][keep], want[keep]):
            diff = (got[key][keep] != want[keep])
            rel = ((got[key][keep].double() - want[keep].double()).abs() / want[keep].double().abs().clamp_min(1e-300))[diff]
            bad[key] = (int(diff.sum()), int(keep.sum()), float(rel.max()))
    print("gradient-scale 3-homogeneity %s-%s-k%+d: tensors not bit-identical (differing, compared, worst relative): %s" % (shape, gemm, k, bad))
    hold(macx, "3-homogeneity", "%s-%s-k%+d" % (shape, gemm, k), case, got, k=k)
    assert not bad, bad


# ---- 4. range inside the operands, under the per-question scales of item 1
@pytest.mark.parametrize("gemm", ["h2", "native"])
@pytest.mark.parametrize("shape", ["launch", "chain"])
@pytest.mark.parametrize("kind", ["kbrange", "gain16", "zerokb"])
def test_range_inside_the_operands(macx, dev, kind, shape, gemm):
    """kbrange: knowledge-base rows times 2^u, u in [-6, 6] -- large activation rows meet small-gradient questions and the other
    way round.  gain16: the read unit's logit weights x 16, attentions up to ~0.98 and many gradient rows near zero.  zerokb: one
    question whose knowledge base is exactly zero (block exponent H2_E_MAX on the ACTIVATION side of every contraction) with a
    gradient that is not."""
    case = CASES["%s-%s" % (kind, shape)]
    got = run_hip(macx, dev, case, gemm)
    hold(macx, "4-range", "%s-%s-%s" % (kind, shape, gemm), case, got)


# ---- 5. the stem: one exponent per operand tensor
def run_stem(macx, dev, **kw):
    cfg, stem, img, dout = gsc.stem_case(macx, **kw)
    r64, r32 = [gsc.oracle_stem(cfg, stem, img, dout, dt) for dt in (torch.float64, torch.float32)]
    stem = stem.to(dev)
    out = stem(img.to(dev), train=True, seed=gsc.STEM_SEED)
    (out * dout.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = {"out": out.detach().cpu()}
    for f, name in macx.stem.REF_NAMES.items():
        got["param:" + name] = getattr(stem, f).grad.cpu()
    return got, r64, r32


def test_stem_forward_per_image_scales(macx, dev):
    """Images at 2^{0, -8, -16} of each other share ONE block exponent in kb_gemm3h_kernel: each image's output against fp64,
    relative to that image's own largest entry, at the stem tests' 1e-5.  (macx_gemm3h.hip.h: the smallest image's products keep
    an absolute error of 2^-38 of the tensor's maximum, about 2^-22 of its own -- the measured figure is printed.)"""
    got, r64, r32 = run_stem(macx, dev, image_scales=gsc.STEM_FWD_SCALES)
    e = gsc.per_question_err(got["out"], r64["out"])
    e32 = gsc.per_question_err(r32["out"], r64["out"])
    print("gradient-scale 5-stem forward: per image err %s (log2 %s), fp32 oracle %s" % (e, ["%.1f" % gsc.log2(x) for x in e], e32))
    b = max(range(len(e)), key=lambda i: e[i])
    _FIGURES.setdefault("5-stem", {})["forward"] = (e[b] / gsc.STEM_FWD_TOL, "out[%d]" % b, e[b] / e32[b] if e32[b] > 0 else gsc.INF)
    assert max(e) < gsc.STEM_FWD_TOL, e


def test_stem_backward_per_image_scales(macx, dev):
    """d_out at 2^{0, -10, -20} per image under one exponent per tensor (kb_gemm3h_kernel backward-data, wgrad_split_kernel<WgFp16x2>): the four
    parameter gradients with the scaled floor (unit 1).  The fused stem returns no image gradient (image features are inputs), so
    the per-image figure of the backward-data product cannot be observed from outside; it enters kernel0's gradient."""
    got, r64, r32 = run_stem(macx, dev, dout_scales=gsc.STEM_BWD_SCALES)
    errs = {k: (gsc.scaled_rel_err(got[k], r64[k], 1.0), gsc.GRAD_TOL) for k in r64 if k.startswith("param:")}
    e32 = {k: (gsc.scaled_rel_err(r32[k], r64[k], 1.0), gsc.GRAD_TOL) for k in errs}
    record("5-stem", "backward", errs, e32)
    assert max(gsc.per_question_err(got["out"], r64["out"])) < gsc.STEM_FWD_TOL
    bad = {k: e for k, (e, bound) in errs.items() if not e < bound}
    assert not bad, bad


def test_stem_all_zero_output_gradient(macx, dev):
    """d_out = 0 (h2_exponent(0) on the gradient side of both contractions): every gradient is exactly zero, and finite."""
    got, r64, _ = run_stem(macx, dev, zero_dout=True)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), k
        if k.startswith("param:"):
            assert not bool((t != 0).any()), k


# ---- 6. the tower under a scaled loss
_TOWER = {}


@pytest.mark.parametrize("k", gsc.TOWER_K)
def test_tower_gradients_follow_the_loss_scale(macx, dev, k):
    """MACNet as in test_gpu_encoder.test_full_tower_ids_to_logits_gradients with loss * 2^k: every parameter gradient against the
    oracle's times 2^k, floors times 2^k, at that test's 3e-4 -- an absolute epsilon anywhere between the loss kernel and the
    embedding gradient shows at 2^-24, a saturation at 2^+24."""
    cfg, net, img, q, lengths, ans = gsc.tower_case(macx)
    if not _TOWER:
        r64, r32 = [gsc.oracle_tower(cfg, net, img, q, lengths, ans, dt) for dt in (torch.float64, torch.float32)]
        _TOWER.update(r64=r64, e32={key: (gsc.scaled_rel_err(r32[key], r64[key], 1.0, floor=gsc.tower_floor(key)), gsc.TOWER_TOL)
                                    for key in r64 if key.startswith("param:")})
    r64, e32 = _TOWER["r64"], _TOWER["e32"]
    net = net.to(dev)
    logits = net(img.to(dev), q.to(dev), lengths.to(dev), train=True, seed=gsc.TOWER_SEED)
    loss, pred = net.loss_and_pred(logits, ans.to(dev))
    (loss * 2.0 ** k).backward()
    torch.cuda.synchronize()
    assert float((logits.detach().cpu().double() - r64["logits"]).abs().max()) < 5e-5
    errs = {}
    for mod, refs in gsc.tower_modules(macx, cfg, net):
        for f, lst in refs.items():
            if not hasattr(mod, f):
                continue
            for refname, idx in lst:
                rg = r64["param:" + refname] * 2.0 ** k
                g = getattr(mod, f).grad
                g = g if idx is None else g[idx]
                errs["param:" + refname] = (gsc.scaled_rel_err(g.reshape(rg.shape), rg, 2.0 ** k, floor=gsc.tower_floor(refname)), gsc.TOWER_TOL)
    assert set(errs) == set(e32), set(errs) ^ set(e32)
    record("6-tower", "k%+d" % k, errs, e32)
    bad = {key: e for key, (e, bound) in errs.items() if not e < bound}
    assert not bad, bad
