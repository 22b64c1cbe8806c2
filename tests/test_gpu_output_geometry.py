"""-m gpu: the answer side at real vocabulary and batch sizes -- macx.OutputClassifier on macx_output_forward_w / _backward_w, the generic
classifier, macx_answer_loss and macx_answer_loss_weighted on their own, and the tower with 1845 answers.

Cases, data and metrics: output_geometry_cases.py (the path every row takes is in its table and is held to the launch rules on the CPU by
test_output_geometry_host.py, which also shows that fp32 arithmetic on the same data uses at most a third of every bound):
  * fused unit, every row of the table, training (hashed masks) and at keep = 1 where marked, forward and backward against the plain fp64
    restatement: logits <= 2e-5 absolute; d_memory / d_vecQ PER QUESTION, every weight gradient PER COLUMN AND PER ROW (fc1_W: per
    answer), every bias gradient per element over sum_b |d preactivation| -- all <= GRAD_TOL, an exactly zero reference admitting exactly
    zero; a second forward + backward gives the same bits; both packs of fc1_W hold zeros on the padded part of the answer axis; inputs, outputs, gradients, `saved` and `ws` sit between sentinel bands
    (test_gpu_guards.py's allocator, extended to n-D tensors), which stay intact;
  * generic classifier (no --outQuestion, two hidden layers of 128) at A = 1845 and 17 (padded to 1920 and 128 columns), same metrics;
  * both loss kernels at (B, A) = (65, 1845), (129, 1845), (1000, 17), (3, 3129) against fp64 cross_entropy; first maxima under ties in
    one lane's passes 0 and 28 and across lanes 63 / 0; a label A - 1; the weighted twin bit-equal to the plain kernel in live rows; a row
    of -inf logits: pred = 0 (tf.argmax / torch.argmax), loss row NaN, gradient row NaN, in both kernels;
  * the tower of test_gpu_stem.test_core_graph_stem_cell_classifier_gradients with answerWordsNum = 1845: pred equals the oracle's.
`-s` (and any failure) prints every figure with the worst question, column and row; observed: profiles/output_geometry_errors.txt.
"""
import contextlib
import math

import pytest
import torch

import abi_kit
import answer_weights_ref as awr
import output_geometry_cases as og
from oracle import dropout_hash as dh
from oracle import mac_oracle as mo

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def guarded(dev):
    """abi_kit.guarded_allocations, with n-D fp32 device tensors (torch.empty(B, A, ..), torch.empty_like) carved out of its
    guarded 1-D buffers as well: the unit's logits, the input gradients and the parameter gradients"""
    with abi_kit.guarded_allocations() as seen:
        one_d, real_like = torch.empty, torch.empty_like

        def empty(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else size
            if len(shape) > 1 and kw.get("dtype") is torch.float32 and str(kw.get("device", "cpu")).startswith("cuda"):
                return one_d(math.prod(shape), **kw).view(*shape)
            return one_d(*size, **kw)

        def empty_like(t, **kw):
            if not kw and t.is_cuda and t.dtype is torch.float32 and t.dim() >= 1:
                return empty(*t.shape, dtype=torch.float32, device=t.device)
            return real_like(t, **kw)

        torch.empty, torch.empty_like = empty, empty_like
        try:
            yield seen
        finally:
            torch.empty, torch.empty_like = one_d, real_like


def on_device(t, dev):
    """a copy of host tensor t inside a guarded allocation (call under guarded())"""
    return torch.empty(*t.shape, dtype=torch.float32, device=dev).copy_(t)


# ---- the fused unit ---------------------------------------------------------------------------------------------------------
_REF = {}          # one case's data and fp64 references at a time


def reference(macx, c):
    if _REF.get("id") != c.id:
        _REF.clear()
        _REF.update(id=c.id, data=og.make_case(macx, mo, c))
        for train in c.modes:
            _REF[train] = og.reference(c, *_REF["data"], train)
    return _REF


def pack(w, K, Nout):
    """macx_small.hip.h's format 0 of a [k_src, n_src] matrix zero-padded to [K, Nout]: dst[Q][g][j][e] = w[16 Q + 4 g + e][j]"""
    full = torch.zeros(K, Nout)
    full[: w.shape[0], : w.shape[1]] = w
    return full.view(K // 16, 4, 4, Nout).permute(0, 1, 3, 2).reshape(-1)


def check_packs(unit, c, seen):
    """the two packs of fc1_W on the padded answer axis, read back from `saved` and `ws` (the first two guarded buffers of the size both
    size calls give): the forward pack's columns A .. Ap and the transposed pack's k rows A .. Ap hold zeros, the rest fc1_W's bits"""
    n = og.saved_floats(c.B, c.d, c.H, c.A)
    assert n == og.ws_floats(c.B, c.d, c.H, c.A)
    bufs = [full[abi_kit.ALLOC_GUARD: abi_kit.ALLOC_GUARD + k] for full, k in seen if k == n]
    assert len(bufs) == 2, len(bufs)
    off, Ap, w = og.al4(c.d * c.d) + og.al4(2 * c.d * c.H), og.pad16(c.A), unit.fc1_W.detach().cpu()
    assert torch.equal(bufs[0][off: off + c.H * Ap].cpu(), pack(w, c.H, Ap)), "forward pack of fc1_W"
    assert torch.equal(bufs[1][off: off + c.H * Ap].cpu(), pack(w.t(), Ap, c.H)), "transposed pack of fc1_W"


def run_fused(unit, c, mem, vq, dl, train, dev):
    for p in unit.parameters():
        p.grad = None
    with guarded(dev) as seen:
        memd, vqd, dld = on_device(mem, dev).requires_grad_(True), on_device(vq, dev).requires_grad_(True), on_device(dl, dev)
        word = None if not c.word else torch.tensor([c.word - (1 << 32) if c.word >= (1 << 31) else c.word], dtype=torch.int32, device=dev)
        logits = unit(memd, vqd, train=train, seed=og.SEED, b0=c.b0, mask_word=word)
        (logits * dld).sum().backward()
        torch.cuda.synchronize()
    abi_kit.assert_guards_intact(seen, ("output unit", c.id, train))
    check_packs(unit, c, seen)
    assert len(seen) >= 10                                            # saved, ws; inputs; logits; input and parameter gradients (16 floats and up)
    got = dict(logits=logits.detach().clone(), d_memory=memd.grad.clone(), d_vecQ=vqd.grad.clone())
    got.update({f: getattr(unit, f).grad.detach().clone() for f in og.FIELDS})
    return got


@pytest.mark.parametrize("case", og.CASES, ids=lambda c: c.id)
def test_output_geometry(macx, dev, case):
    ref = reference(macx, case)
    cfg, host, mem, vq, answers = ref["data"]
    unit = macx.OutputClassifier(cfg, generator=torch.Generator().manual_seed(1))
    unit.load_state_dict(host.state_dict())
    unit = unit.to(dev)
    tol, bad = og.tolerances(), []
    for train in case.modes:
        first = run_fused(unit, case, mem, vq, ref[train]["dl"], train, dev)
        second = run_fused(unit, case, mem, vq, ref[train]["dl"], train, dev)
        for k in og.METRICS:
            assert torch.isfinite(first[k]).all(), (k, train)
            if not torch.equal(first[k], second[k]):
                bad.append("%s differs between two runs (%s)" % (k, "train" if train else "keep1"))
        e = og.errors(first, ref[train])
        og.log(og.line(case, "hip", train, e))
        print("    " + e["where"])
        for k in og.METRICS:
            if not e[k] <= tol[k]:
                bad.append("%s %.3e > %.1e (%s): %s" % (k, e[k], tol[k], "train" if train else "keep1", e["where"]))
    assert not bad, "\n".join([case.reaches, str(og.route(case))] + bad)


# ---- the generic classifier ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, A, padded", og.GENERIC)
def test_generic_classifier_geometry(macx, dev, B, A, padded):
    cfg, prm, mem, answers = og.generic_data(mo, B, A)
    unit = macx.OutputClassifier(cfg, generator=torch.Generator().manual_seed(1))
    assert type(unit) is macx.GenericOutputClassifier and list(unit.params.names) == list(prm) and A + (-A) % 128 == padded
    unit.load_reference_dict(prm)
    unit = unit.to(dev)
    keep = float(unit.keep)
    ref = og.generic_reference(cfg, prm, mem, answers, keep, og.generic_masks(macx.output.fc_site, B, keep, torch.float64))
    runs = []
    for _ in range(2):
        memd = mem.to(dev).requires_grad_(True)
        logits = unit(memd, torch.zeros(B, og.GENERIC_D, device=dev), train=True, seed=og.SEED, b0=og.GENERIC_B0)
        (logits * ref["dl"].to(dev)).sum().backward()
        torch.cuda.synchronize()
        got = dict(logits=logits.detach().clone(), d_memory=memd.grad.clone())
        got.update({k: v.detach().clone() for k, v in unit.params.grads_by_name().items()})
        runs.append(got)
        unit.zero_grad(set_to_none=True)
    first, second = runs
    assert first["logits"].shape == (B, A) and first[og.GENERIC_W[2]].shape == (og.GENERIC_DIMS[1], A) and first[og.GENERIC_B[2]].shape == (A,)
    e = og.generic_errors(first, ref)
    og.log("generic B%d A%d (-> %d columns) train " % (B, A, padded) +
           " ".join("%s %.2f" % (og.generic_label(k), v / (og.LOGIT_TOL if k == "logits" else og.GRAD_TOL)) for k, v in e.items()))
    bad = ["%s %.3e" % (k, v) for k, v in e.items() if not v <= (og.LOGIT_TOL if k == "logits" else og.GRAD_TOL)]
    bad += ["%s differs between two runs" % k for k in first if not torch.equal(first[k], second[k])]
    assert not bad, bad


# ---- both loss kernels on their own --------------------------------------------------------------------------------------------
def launch_plain(macx, dev, logits, answers, scale):
    L, ptr = macx._lib.lib(), macx._lib.ptr
    B, A = logits.shape
    lg, an = logits.to(dev), answers.to(dev)
    rows, pred, dl = torch.full((B,), 7.0, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B, A), 7.0, device=dev)
    macx._lib.check(L.macx_answer_loss(ptr(lg), ptr(an), B, A, ptr(rows), ptr(pred), ptr(dl), scale, None), "macx_answer_loss")
    torch.cuda.synchronize()
    return rows.cpu(), pred.cpu(), dl.cpu()


def launch_weighted(macx, dev, logits, answers, weights, scale):
    L, ptr = macx._lib.lib(), macx._lib.ptr
    B, A = logits.shape
    lg, an, w = logits.to(dev), answers.to(dev), None if weights is None else weights.to(dev)
    rows, pred = torch.full((B,), 7.0, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    dl, out = torch.full((B, A), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    macx._lib.check(L.macx_answer_loss_weighted(ptr(lg), ptr(an), ptr(w), B, A, ptr(rows), ptr(pred), ptr(dl), ptr(out), None, scale, None),
                    "macx_answer_loss_weighted")
    torch.cuda.synchronize()
    return rows.cpu(), pred.cpu(), dl.cpu(), out.cpu()


@pytest.mark.parametrize("B, A", og.LOSS_SHAPES)
def test_answer_loss_at_real_sizes(macx, dev, B, A):
    logits, answers, first_max = og.loss_case(B, A)
    scale = 0.5 / B
    rows, pred, dl = launch_plain(macx, dev, logits, answers, scale)
    ref = logits.double().requires_grad_(True)
    want_rows = torch.nn.functional.cross_entropy(ref, answers.long(), reduction="none")
    (want_rows.sum() * scale).backward()
    err_rows = float((rows.double() - want_rows.detach()).abs().max())
    err_mean = abs(float(rows.mean()) - float(want_rows.mean()))
    ratio = ((dl.double() - ref.grad).abs() / og.dlogits_bound(logits, answers, scale)).max()
    og.log("answer_loss B%d A%d: rows %.2e mean %.2e (bound %.0e), dlogits %.2f of its bound" % (B, A, err_rows, err_mean, og.LOSS_TOL, float(ratio)))
    assert err_rows <= og.LOSS_TOL and err_mean <= og.LOSS_TOL
    assert float(ratio) <= 1.0
    for r, c in first_max.items():
        assert int(pred[r]) == c, (r, int(pred[r]), c)                         # the FIRST maximum
    others = [r for r in range(B) if r not in first_max]
    assert torch.equal(pred.long()[others], logits.argmax(dim=-1)[others])
    assert int(answers[2]) == A - 1 and math.isfinite(float(rows[2])) and float(dl[2, A - 1]) < 0
    # ---- the weighted twin
    import test_gpu_answer_weights as aw
    for pattern in ("zero tail", "fractions"):
        weights = aw.draw_weights(pattern, B, torch.Generator().manual_seed(B + A))
        dead = ~awr.live(weights, B)
        lg2, an2 = logits.clone(), answers.clone()
        lg2[dead] = float("nan")
        an2[dead] = A + 7
        want = awr.reference(lg2, an2, weights, grad_scale=0.5)
        wrows, wpred, wdl, wloss = launch_weighted(macx, dev, lg2, an2, weights, 0.5)
        live = ~dead
        assert abi_kit.bits_equal(wrows[live], rows[live]) and torch.equal(wpred[live], pred[live]), pattern
        assert wpred[dead].tolist() == [-1] * int(dead.sum()) and aw.is_plus_zero(wrows[dead]) and aw.is_plus_zero(wdl[dead])
        err_loss, err_dl = abs(float(wloss[0]) - float(want["loss"])), float((wdl.double() - want["dlogits"]).abs().max())
        og.log("answer_loss_weighted B%d A%d %s: loss %.2e (bound %.0e) dlogits %.2e (bound 1e-06), %d dead" % (B, A, pattern, err_loss, og.LOSS_TOL,
                                                                                                          err_dl, int(dead.sum())))
        assert err_loss <= og.LOSS_TOL and err_dl <= 1e-6
        assert torch.equal(wpred.long(), want["pred"])


@pytest.mark.parametrize("B, A", [(5, 1845), (5, 17)])
def test_a_row_of_minus_infinity(macx, dev, B, A):
    """every logit of row 1 is -inf: tf.argmax and torch.argmax give 0; the loss row is NaN (-inf - -inf) and so is its gradient row"""
    logits, answers, _ = og.loss_case(B, A)
    logits[1] = -math.inf
    assert int(logits.argmax(dim=-1)[1]) == 0
    rows, pred, dl = launch_plain(macx, dev, logits, answers, 1.0 / B)
    wrows, wpred, wdl, wloss = launch_weighted(macx, dev, logits, answers, None, 1.0)
    print("row of -inf, A = %d: pred %d (plain) %d (weighted)" % (A, int(pred[1]), int(wpred[1])))
    for p, r, g in ((pred, rows, dl), (wpred, wrows, wdl)):
        assert int(p[1]) == 0, hex(int(p[1]))
        assert math.isnan(float(r[1])) and bool(torch.isnan(g[1]).all())
        rest = [0, 2, 3, 4]
        assert torch.equal(p.long()[rest], logits.argmax(dim=-1)[rest]) and bool(torch.isfinite(r[rest]).all()) and bool(torch.isfinite(g[rest]).all())
    assert abi_kit.bits_equal(rows[[0, 2, 3, 4]], wrows[[0, 2, 3, 4]]) and torch.equal(pred, wpred) and math.isnan(float(wloss[0]))


# ---- the tower ----------------------------------------------------------------------------------------------------------------
def test_tower_with_the_gqa_vocabulary(macx, dev):
    """test_gpu_stem.test_core_graph_stem_cell_classifier_gradients at its shape with answerWordsNum = 1845: images -> stem -> cell x p ->
    classifier -> loss against the oracle chain under identical masks; logits, loss, pred and every parameter gradient"""
    from helpers import rel_err, max_abs
    B, H, W, Cin, d, p, S, A = 3, 5, 4, 128, 128, 2, 6, 1845
    cfg = mo.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d, outClassifierDims=[32], answerWordsNum=A)
    cfg.stemDim = 128
    net = macx.MACNetCore(cfg, H=H, W=W, imageInDim=Cin, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)
    g = torch.Generator().manual_seed(6)
    img = torch.relu(torch.randn(B, H * W, Cin, generator=g))
    vq, words, lengths, _ = mo.synthetic_inputs(B, S, 1, d, seed=8)
    ans = torch.tensor([1, 1844, 1797])
    logits = net(img.to(dev), vq.to(dev), words.to(dev), lengths.to(dev), train=True, seed=21)
    loss, pred = net.loss_and_pred(logits, ans.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    dt = torch.float64
    prm = {}
    for src in (net.stem.to_reference_dict(), net.cell.to_reference_dict(), net.out.to_reference_dict()):
        prm.update({k: v.cpu().to(dt).requires_grad_(True) for k, v in src.items()})
    vs = mo.VarStore(params=prm, dtype=dt)
    keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout)
    sk, ok = net.stem.keep, net.out.keep
    smasks = [torch.from_numpy(dh.mask_for(21, 9, 0, sk, (B, H * W, Cin))).to(dt), torch.from_numpy(dh.mask_for(21, 10, 0, sk, (B, H * W, 128))).to(dt)]
    kb = mo.stem_cnn(cfg, vs, img.to(dt), H, W, keep=sk, masks=smasks)
    c, m, _ = mo.mac_network(cfg, vs, vq.to(dt), words.to(dt), words.to(dt), lengths, kb, train=True, mask_fn=mo.hash_mask_fn(21, keeps), keeps=keeps)
    omasks = [torch.from_numpy(dh.mask_for(21, 7, 0, ok, (B, 2 * d))).to(dt), torch.from_numpy(dh.mask_for(21, 8, 0, ok, (B, 32))).to(dt)]
    rl = mo.output_classifier(cfg, vs, m, vq.to(dt), output_keep=ok, masks=omasks)
    rloss, rpred = mo.answer_loss_and_pred(rl, ans)
    rloss.backward()
    assert logits.shape == (B, A) and max_abs(logits, rl) < 5e-5 and torch.equal(pred.cpu(), rpred)
    assert abs(float(loss) - float(rloss)) < 1e-5
    bad = {}
    for mod, refs in ((net.stem, {f: [(n, None)] for f, n in macx.stem.REF_NAMES.items()}),
                      (net.cell, macx.params.reference_names(cfg, p)),
                      (net.out, {f: [(n, None)] for f, n in macx.output.REF_NAMES.items()})):
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
    fc1 = og.per_line_err(net.out.fc1_W.grad, prm[macx.output.REF_NAMES["fc1_W"]].grad)[0]
    print("tower, 1845 answers: logits %.2e, fc1_W per answer %.2e" % (max_abs(logits, rl), float(fc1.max())))
