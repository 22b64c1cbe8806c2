"""-m gpu: the attention-loss launch (macx_att_loss) from the kernel up to the captured training steps.

1  the kernel alone against the fp64 reference (tests/att_loss_ref.py), with bounds that follow from fp32 arithmetic:
     rows     |row - ref| <= (n + 16) * 2^-23 * sum_j |term_j|   -- the terms are rounded to fp32 once (2^-24 each) and summed in fp32
              by 64 lanes and six shuffle steps, at most ceil(n / 64) + 6 <= n + 6 additions deep; one more rounding of the product
              with the weight
     d_att    every entry within 2^-20 of its reference, relative to that entry (the kernel evaluates each entry in fp64 and
              rounds once: 2^-24; the weight and eps are the same fp32 values on both sides)
     j >= L   bit for bit +0.0f, with NaN in att and target there
2  bit for bit: NULL weights == ones, a target per step == the shared one repeated, d_att = NULL, repeated calls, row weight 0
3  bad arguments return MACX_EINVAL and launch nothing
4  through the cell: every input and parameter gradient against the fp64 oracle's autograd of the reference loss on ITS maps
   (tests/test_gpu_state_grads.py's tolerance), and state_tensor against the per-step lists
5  CapturedTrainStep / CapturedDPTrainStep / CapturedTowerTrainStep with att_loss= (and aux_loss=): replays == the eager step
"""
import contextlib
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import att_loss_ref as ar
import state_grads_ref as sr
from abi_kit import bits, bits_equal
from helpers import make_case
from kb_lengths_ref import masked_kb_attention
from oracle import mac_oracle as mo
from test_gpu_state_grads import GRAD_TOL, _build, _grad_errors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"ce": 0, "entropy": 1}
EPS, SCALE = 1e-8, 0.37
POISON = 7.0


def call(macx, dev, att, target, lengths, sw, rw, kind, eps=EPS, scale=SCALE, want_d=True, target_steps=None, null_target=False):
    """macx_att_loss through ctypes on poisoned outputs: (return code, rows, d_att | None)"""
    L = macx._lib.lib()
    p, B, n = att.shape
    to = lambda t, dt=torch.float32: None if t is None else t.to(dt).to(dev).contiguous()
    a, t, ln, s, r = to(att), to(target), to(None if lengths is None else torch.as_tensor(lengths), torch.int32), to(sw), to(rw)
    rows = torch.full((p, B), POISON, device=dev)
    d = torch.full((p, B, n), POISON, device=dev) if want_d else None
    if target_steps is None:
        target_steps = int(t is not None and t.dim() == 3)
    ptr = macx._lib.ptr
    rc = L.macx_att_loss(ptr(a), ptr(None if null_target else t), ptr(ln), ptr(s), ptr(r), p, B, n, KIND.get(kind, kind), target_steps,
                         eps, scale, ptr(rows), ptr(d), None)
    torch.cuda.synchronize()
    return rc, rows, d


def length_modes(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    mixed = torch.randint(1, n + 1, (B,), generator=g)
    return {"none": None, "ones": torch.ones(B, dtype=torch.int64), "full": torch.full((B,), n), "random": mixed,
            "zero": torch.zeros(B, dtype=torch.int64), "past": torch.full((B,), n + 5)}


# ================================================= 1 ===============================================================================
@pytest.mark.parametrize("kind", ["ce", "entropy"])
@pytest.mark.parametrize("p,B,n", [(1, 1, 1), (3, 3, 49), (2, 5, 64), (2, 5, 65), (3, 2, 300)])
def test_kernel_against_fp64_reference(macx, dev, p, B, n, kind):
    g = torch.Generator().manual_seed(100 * n + B)
    sw, rw = 0.5 + torch.rand(p, generator=g), 0.5 + torch.rand(B, generator=g)
    for mode, lengths in length_modes(B, n, seed=n).items():
        att, target = ar.draw(p, B, n, lengths, seed=7 + n, nan=True)           # NaN at every j >= L, in both
        for per_step in ((False, True) if kind == "ce" else (False,)):
            t = None if kind != "ce" else (target if per_step else target[0])
            kw = dict(target=t, lengths=lengths, step_weights=sw, row_weights=rw, kind=kind, eps=EPS, scale=SCALE)
            rc, rows, d = call(macx, dev, att, t, lengths, sw, rw, kind)
            assert rc == 0, (mode, rc)
            want_rows, want_d, mag = ar.rows(att, **kw), ar.d_att(att, **kw), ar.abs_term_sums(att, **kw)
            err = (rows.cpu().double() - want_rows).abs()
            bound = (n + 16) * 2.0 ** -23 * mag
            print("ATTLOSS %s p%d B%d n%d %s per_step=%d: worst row error / bound %.3f" % (kind, p, B, n, mode, per_step,
                                                                                          float((err / bound.clamp_min(1e-300)).max())))
            assert bool((err <= bound).all()), (mode, per_step, float((err - bound).max()))
            derr = (d.cpu().double() - want_d).abs()
            assert bool((derr <= 2.0 ** -20 * want_d.abs()).all()), (mode, per_step, float((derr / want_d.abs().clamp_min(1e-300)).max()))
            dead = ~ar.live_mask(lengths, B, n)
            assert bool((bits(d)[:, dead] == 0).all()), mode                    # +0.0f, bit for bit
            assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(d).all())
            assert float(want_rows.abs().min()) > 0 or n == 1                   # (not a comparison of zeros)


# ================================================= 2 ===============================================================================
@pytest.mark.parametrize("kind", ["ce", "entropy"])
@pytest.mark.parametrize("p,B,n", [(3, 3, 49), (2, 5, 65)])
def test_kernel_exactness(macx, dev, p, B, n, kind):
    g = torch.Generator().manual_seed(n)
    lengths = length_modes(B, n, seed=3)["random"]
    att, target = ar.draw(p, B, n, lengths, seed=11, nan=True)
    t = target[0] if kind == "ce" else None
    sw, rw = 0.5 + torch.rand(p, generator=g), 0.5 + torch.rand(B, generator=g)
    # NULL weights == weights of ones
    rc, rows, d = call(macx, dev, att, t, lengths, None, None, kind)
    rc1, rows1, d1 = call(macx, dev, att, t, lengths, torch.ones(p), torch.ones(B), kind)
    assert rc == rc1 == 0 and bits_equal(rows, rows1) and bits_equal(d, d1)
    # two calls give the same bits; d_att = NULL gives the same rows
    rc, rows, d = call(macx, dev, att, t, lengths, sw, rw, kind)
    rc1, rows1, d1 = call(macx, dev, att, t, lengths, sw, rw, kind)
    rc2, rows2, _ = call(macx, dev, att, t, lengths, sw, rw, kind, want_d=False)
    assert rc == rc1 == rc2 == 0 and bits_equal(rows, rows1) and bits_equal(d, d1) and bits_equal(rows, rows2)
    if kind == "ce":                                          # one target for every step == the same target repeated per step
        where_live = ar.live_mask(lengths, B, n)
        rep = target[0].unsqueeze(0).expand(p, B, n).clone()
        assert bool(torch.isnan(rep[:, ~where_live]).all())
        rc3, rows3, d3 = call(macx, dev, att, rep, lengths, sw, rw, kind)
        assert rc3 == 0 and bits_equal(rows, rows3) and bits_equal(d, d3)
    # a row weight of 0: an exactly zero row and +0.0f gradient row, even where att holds 0 under a positive target (and NaN elsewhere)
    rw0 = rw.clone()
    rw0[1] = 0.0
    hard = att.clone()
    hard[:, 1, 0] = 0.0
    hard[:, 1, 1:] = float("nan")
    ht = None
    if kind == "ce":
        ht = target[0].clone()
        ht[1, 0] = 1.0
    rc4, rows4, d4 = call(macx, dev, hard, ht, lengths, sw, rw0, kind)
    assert rc4 == 0 and bool((bits(rows4)[:, 1] == 0).all()) and bool((bits(d4)[:, 1] == 0).all())
    assert bool(torch.isfinite(rows4).all()) and bool(torch.isfinite(d4).all())
    others = [b for b in range(B) if b != 1]
    assert bits_equal(rows4[:, others], rows[:, others]) and bits_equal(d4[:, others], d[:, others])


# ================================================= 3 ===============================================================================
def test_bad_arguments_launch_nothing(macx, dev):
    p, B, n = 2, 3, 17
    att, target = ar.draw(p, B, n, None, seed=1, nan=False)
    EINVAL = macx._lib.MACX_EINVAL
    for what, kw in (("eps = 0", dict(kind="ce", eps=0.0)), ("eps < 0", dict(kind="ce", eps=-1e-8)),
                     ("eps = inf", dict(kind="entropy", eps=float("inf"))), ("eps = nan", dict(kind="entropy", eps=float("nan"))),
                     ("kind 7", dict(kind=7)), ("kind -1", dict(kind=-1)), ("NULL CE target", dict(kind="ce", null_target=True))):
        rc, rows, d = call(macx, dev, att, target, None, None, None, **kw)
        assert rc == EINVAL, what
        assert bool((rows == POISON).all()) and bool((d == POISON).all()), what
    rc, rows, d = call(macx, dev, att, None, None, None, None, "entropy", null_target=True)      # entropy takes no target
    assert rc == 0 and not bool((rows == POISON).any()) and not bool((d == POISON).any())


# ================================================= 4 ===============================================================================
def oracle_att_loss(cfg, ref_params, vq, words, lengths, kb, on, loss_kw, kb_lengths=None, seed=5):
    """state_grads_ref.oracle_aux with the reference loss on the stack of the oracle's own maps"""
    dt = torch.float64
    params = {k: v.detach().cpu().to(dt).clone().requires_grad_(True) for k, v in ref_params.items()}
    vs = mo.VarStore(params=params, dtype=dt)
    vq_, words_, kb_ = [t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (vq, words, kb)]
    keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout)
    masked = masked_kb_attention(kb_lengths, kb.shape[1]) if kb_lengths is not None else contextlib.nullcontext()
    with masked:
        c, m, cell = mo.mac_network(cfg, vs, vq_, words_, words_, lengths.cpu(), kb_, train=True, mask_fn=mo.hash_mask_fn(seed, keeps, b0=0),
                                    keeps=keeps)
    maps = torch.stack(list(cell.attentions[on]), dim=0)
    rows = ar.rows(maps, **loss_kw)
    rows.sum().backward()
    return dict(params=params, inputs=(vq_, words_, kb_), rows=rows.detach(), maps=maps.detach())


@pytest.mark.parametrize("name", ["args", "args1"])
@pytest.mark.parametrize("on,kind,kb_lengths", [("kb", "ce", None), ("kb", "ce", [49, 1, 23]), ("question", "entropy", None)])
def test_through_the_cell_against_the_oracle(macx, dev, name, on, kind, kb_lengths):
    sh = sr.SINGLE_SHAPE
    B, S, N, d, p = sh["B"], sh["S"], sh["N"], sh["d"], sr.steps_of(name)
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    if kb_lengths is not None:
        for b, n in enumerate(kb_lengths):
            kb[b, n:] = 0.0
    n = N if on == "kb" else S
    live = (None if kb_lengths is None else torch.tensor(kb_lengths)) if on == "kb" else lengths
    g = torch.Generator().manual_seed(21)
    _, target = ar.draw(p, B, n, live, seed=5, nan=False)
    sw, rw = 0.5 + torch.rand(p, generator=g), 0.5 + torch.rand(B, generator=g)
    kw = dict(target=target[0] if kind == "ce" else None, lengths=live, step_weights=sw, row_weights=rw, kind=kind, eps=EPS, scale=1.0)
    cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb, kb_lengths=kb_lengths)
    assert type(cell).__name__ == "MACCell"
    cell.run()
    dv = lambda t: None if t is None else t.to(dev)
    rows = macx.losses.attention_loss(cell.state_tensor("att_" + on), dv(kw["target"]), lengths=dv(live), step_weights=dv(sw),
                                      row_weights=dv(rw), kind=kind, eps=EPS, scale=1.0)
    assert rows.shape == (p, B) and rows.requires_grad
    rows.sum().backward()
    torch.cuda.synchronize()
    ref = oracle_att_loss(cfg, params.to_reference_dict(), vq, words, lengths, kb, on, kw, kb_lengths=kb_lengths)
    row_err = float((rows.detach().cpu().double() - ref["rows"]).abs().max() / ref["rows"].abs().max())
    errs = _grad_errors(macx, cfg, p, params, inputs, ref)
    worst = max(errs, key=errs.get)
    print("\nATTLOSS cell %s %s on %s lengths %s: rows %.2e grad %.2e (%s)" % (name, kind, on, kb_lengths, row_err, errs[worst], worst))
    assert row_err < GRAD_TOL
    bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not bad, bad
    for nm, x in zip(("vecQuestions", "words", "knowledgeBase"), ref["inputs"]):          # not a comparison of zeros
        if nm in sr.REACHED["att_" + on]:
            assert float(x.grad.abs().max()) > 1e-4, nm
    assert cell.status() == (0, -1)


@pytest.mark.parametrize("name", ["args", "args1"])
def test_state_tensor_gradient_is_the_per_step_gradient(macx, dev, name):
    sh = sr.SINGLE_SHAPE
    B, S, N, d, p = sh["B"], sh["S"], sh["N"], sh["d"], sr.steps_of(name)
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    G = torch.randn(p, B, N, generator=torch.Generator().manual_seed(2)).to(dev)
    results = []
    for route in ("stacked", "slices"):
        cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb)
        cell.run()
        stacked = cell.state_tensor("att_kb")
        assert stacked.shape == (p, B, N) and stacked.requires_grad
        assert all(bits_equal(stacked[i], cell.attentions["kb"][i]) for i in range(p))
        assert cell.state_tensor("memories").shape == (p + 1, B, d) and cell.state_tensor("att_question").shape == (p, B, S)
        if route == "stacked":
            loss = (stacked * G).sum()
        else:
            loss = sum((cell.attentions["kb"][i] * G[i]).sum() for i in range(p))
        loss.backward()
        torch.cuda.synchronize()
        assert not cell.state_tensor("att_kb").requires_grad                       # the pass is over: a plain view again
        results.append([t.grad for t in inputs] + [t.grad for t in params.tensors()])
    assert all(bits_equal(a, b) for a, b in zip(*results))
    assert float(results[0][2].abs().max()) > 0
    with pytest.raises(KeyError):
        cell.state_tensor("infos")
    with pytest.raises(KeyError):
        cell.state_tensor("att_gate")                                              # this option set has no gate


# ================================================= 5 ===============================================================================
TB, TS, TN, TD, TP = 4, 8, 49, 128, 3


def _train_inputs(macx, dev, seed, kb_lengths=None):
    vq, words, lengths, kb = macx.configs.synthetic_inputs(TB, TS, TN, TD, seed=seed)
    if kb_lengths is not None:
        for b, n in enumerate(kb_lengths):
            kb[b, n:] = 0.0
    gm = torch.randn(TB, TD, generator=torch.Generator().manual_seed(seed)) / TB
    return [t.to(dev) for t in (vq, words, lengths, kb, gm)]


def _att_inputs(dev, seed, n, live, p=TP, B=TB):
    g = torch.Generator().manual_seed(seed)
    _, target = ar.draw(p, B, n, live, seed=seed, nan=False)
    rw = 0.5 + torch.rand(B, generator=g)
    rw[seed % B] = 0.0
    return target[0].to(dev), rw.to(dev), (0.5 + torch.rand(p, generator=g)).to(dev)


def _replays_equal_eager(step, extra=()):
    """three replays, each bit for bit the eager step on the same static tensors: memory, every gradient, aux_rows (+ extra())"""
    got = None
    for _ in range(3):
        for t in extra:
            t.grad.zero_()
        mem = step.replay().clone()
        got = [mem] + [t.grad.clone() for t in step._leaves()] + [t.grad.clone() for t in extra]
        if step.aux_rows is not None:
            got.append(step.aux_rows.clone())
        for t in extra:
            t.grad.zero_()
        ref_mem, ref = step.eager_reference()
        want = [ref_mem] + ref + [t.grad.clone() for t in extra] + ([] if step.aux_rows is None else [step.aux_rows.clone()])
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(bits_equal(a, b) for a, b in zip(got, want))
    return got


@pytest.mark.parametrize("on,kind,kb_lengths", [("kb", "ce", False), ("kb", "ce", True), ("question", "entropy", False)])
def test_captured_train_step_with_att_loss(macx, dev, on, kind, kb_lengths):
    cfg = macx.configs.flag_file_config("args", netLength=TP, memDim=TD, ctrlDim=TD, attDim=TD)
    params = macx.MACCellParams(cfg, TP, generator=torch.Generator().manual_seed(0)).to(dev)
    step = macx.CapturedTrainStep(cfg, params, TB, TS, TN, seed=77, kb_lengths=kb_lengths, att_loss=dict(on=on, kind=kind, weight=0.5))
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert step.aux_rows.shape == (TP, TB)
    kbl = [49, 1, 23, 40] if kb_lengths else None
    x = _train_inputs(macx, dev, 1, kbl)
    n = TN if on == "kb" else TS
    live = (torch.tensor(kbl) if kbl else None) if on == "kb" else x[2].cpu()
    seen = []
    for seed in (3, 4):                                             # a first and a second target, with new weights
        target, rw, sw = _att_inputs(dev, seed, n, live)
        lens = {"kb_lengths": torch.tensor(kbl)} if kbl else {}
        step.load(*x, att_target=target if kind == "ce" else None, att_row_weights=rw, att_step_weights=sw, **lens)
        got = _replays_equal_eager(step)
        # ... and the rows are the reference's on the step's own maps, summed with weight / (p * B)
        maps = torch.stack([a.detach().cpu() for a in step.cell.attentions[on]], dim=0)
        want = ar.rows(maps, target=target.cpu() if kind == "ce" else None, lengths=live, step_weights=sw.cpu(), row_weights=rw.cpu(),
                       kind=kind, eps=1e-8, scale=0.5 / (TP * TB))
        assert float((step.aux_rows.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
        assert bool((bits(step.aux_rows)[:, seed % TB] == 0).all())
        seen.append(got)
    # the gradients follow the target and the weights (a loss on the question map does not reach the knowledge base: REACHED)
    reached = 4 if on == "kb" else 3
    assert not any(bits_equal(a, b) for a, b in zip(seen[0][1:reached], seen[1][1:reached]))
    step.check()


def test_captured_train_step_att_loss_changes_the_gradients(macx, dev):
    """... against the step without att_loss, on the same inputs; a weight of 0 gives the plain step's bits"""
    cfg = macx.configs.flag_file_config("args", netLength=TP, memDim=TD, ctrlDim=TD, attDim=TD)
    x = _train_inputs(macx, dev, 1)
    target, rw, sw = _att_inputs(dev, 3, TN, None)
    grads = {}
    for weight in (None, 0.0, 0.5):
        params = macx.MACCellParams(cfg, TP, generator=torch.Generator().manual_seed(0)).to(dev)
        att = {} if weight is None else dict(att_loss=dict(on="kb", kind="ce", weight=weight))
        step = macx.CapturedTrainStep(cfg, params, TB, TS, TN, seed=77, **att)
        assert step.captured
        step.load(*x, **({} if weight is None else dict(att_target=target, att_row_weights=rw, att_step_weights=sw)))
        mem = step.replay().clone()
        grads[weight] = [mem] + [t.grad.clone() for t in step._leaves()]
    assert all(bits_equal(a, b) for a, b in zip(grads[None], grads[0.0]))
    assert bits_equal(grads[None][0], grads[0.5][0])                                   # the forward pass is the same
    assert not any(bits_equal(a, b) for a, b in zip(grads[None][1:4], grads[0.5][1:4]))


@pytest.mark.parametrize("kind", ["ce", "entropy"])
def test_self_check_leaves_the_weights_at_ones(macx, dev, kind):
    """verify=True draws a target and weights into the static tensors; a constructed step holds what its documentation says --
    target zeros, weights ones -- so a load() that passes no weights trains on unit weights"""
    cfg = macx.configs.flag_file_config("args", netLength=TP, memDim=TD, ctrlDim=TD, attDim=TD)
    x = _train_inputs(macx, dev, 1)
    target, _, _ = _att_inputs(dev, 3, TN, None)
    tkw = dict(att_target=target) if kind == "ce" else {}
    out = []
    for explicit in (False, True):
        params = macx.MACCellParams(cfg, TP, generator=torch.Generator().manual_seed(0)).to(dev)
        step = macx.CapturedTrainStep(cfg, params, TB, TS, TN, seed=77, verify=True, att_loss=dict(on="kb", kind=kind, weight=0.5))
        assert step.captured
        assert bool((step.att_row_weights == 1).all()) and bool((step.att_step_weights == 1).all()) and bool((step.aux_rows == 0).all())
        assert step.att_target is None or bool((step.att_target == 0).all())
        ones = dict(att_row_weights=torch.ones(TB, device=dev), att_step_weights=torch.ones(TP, device=dev)) if explicit else {}
        step.load(*x, **tkw, **ones)
        mem = step.replay().clone()
        torch.cuda.synchronize()
        out.append([mem, step.aux_rows.clone()] + [t.grad.clone() for t in step._leaves()])
        maps = torch.stack([a.detach().cpu() for a in step.cell.attentions["kb"]], dim=0)
    assert all(bits_equal(a, b) for a, b in zip(*out))
    want = ar.rows(maps, target=target.cpu() if kind == "ce" else None, kind=kind, eps=1e-8, scale=0.5 / (TP * TB))      # unit weights
    assert float(want.abs().min()) > 0
    assert float((out[0][1].cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_captured_train_step_with_aux_loss_callable(macx, dev):
    cfg = macx.configs.flag_file_config("args", netLength=TP, memDim=TD, ctrlDim=TD, attDim=TD)
    params = macx.MACCellParams(cfg, TP, generator=torch.Generator().manual_seed(0)).to(dev)
    head = (torch.randn(TD, generator=torch.Generator().manual_seed(8)) / TD).to(dev).requires_grad_(True)   # allocated BEFORE the step
    step_weight = torch.linspace(0.5, 1.5, TP + 1).to(dev)

    def aux_loss(cell, state):                                       # a linear head on every step's memory
        return ((cell.state_tensor("memories") @ head) * step_weight.unsqueeze(1)).sum() / TB

    step = macx.CapturedTrainStep(cfg, params, TB, TS, TN, seed=77, aux_loss=aux_loss)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert step.aux_rows is None
    x = _train_inputs(macx, dev, 2)
    step.load(*x)
    got = _replays_equal_eager(step, extra=(head,))
    assert float(head.grad.abs().max()) > 0
    plain = macx.CapturedTrainStep(cfg, params, TB, TS, TN, seed=77)
    plain.load(*x)
    plain.replay()
    assert not bits_equal(plain.knowledgeBase.grad, got[3])                            # the head's loss reached the inputs


# ---- two gloo ranks on the one GPU, as tests/test_gpu_dp.py
DP_CASES = [("kb", "ce", False), ("kb", "ce", True), ("question", "entropy", False)]      # (on, kind, kb_lengths)


def _dp_worker(rank, world, port, ret, case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import macx
    import att_loss_ref as ref
    dev = torch.device("cuda:0")
    Bg, S, N, d, p = 6, 8, 49, 128, 3
    cfg = macx.configs.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d)
    vq, words, lengths, kb = macx.configs.synthetic_inputs(Bg, S, N, d, seed=3)
    lo, hi = macx.dp.tower_slice(Bg, rank, world)
    dm_full = torch.randn(Bg, d, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(5)
    on, kind, with_lengths = case
    kbl = torch.tensor([49, 1, 23, 40, 7, 49]) if with_lengths else None        # (the launch reads the cell's own int32 tensors)
    if kbl is not None:
        for b, k in enumerate(kbl.tolist()):
            kb[b, k:] = 0.0
    n = N if on == "kb" else S
    _, target = ref.draw(p, Bg, n, kbl if on == "kb" else lengths, seed=5, nan=False)
    target = target[0] if kind == "ce" else None
    cut = lambda t: None if t is None else t[lo:hi].to(dev)
    whole = lambda t: None if t is None else t.to(dev)
    built = dict(kb_lengths=True) if with_lengths else {}
    rw, sw = 0.5 + torch.rand(Bg, generator=g), 0.5 + torch.rand(p, generator=g)
    rw[1], rw[4] = 0.0, 0.0                                    # one unsupervised question per shard
    att = dict(on=on, kind=kind, weight=0.5)
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(7)).to(dev)
    params.requires_grad_(True)
    bucket = macx.dp.OverlappedBuckets(params)
    x = [t[lo:hi].to(dev) for t in (vq, words, lengths, kb)]
    dm = (dm_full / (hi - lo))[lo:hi].to(dev)                  # d(mean over the shard) / d memory
    res, flats = {}, {}
    for capture in (True, False):
        step = macx.CapturedDPTrainStep(cfg, params, bucket, B=hi - lo, S=S, N=N, global_batch=Bg, seed=11, b0=lo, capture=capture,
                                        att_loss=att, **built)
        step.load(x[0], x[1], x[2], x[3], dm, att_target=cut(target), att_row_weights=cut(rw), att_step_weights=sw.to(dev),
                  **({"kb_lengths": cut(kbl)} if with_lengths else {}))
        for it in range(3):
            mem = step.step()
            torch.cuda.synchronize()
            now = (bucket.flat.detach().cpu().clone(), mem.detach().cpu().clone(), step.aux_rows.detach().cpu().clone())
            if it == 0:
                flats[capture] = now
            res[(capture, it)] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, flats[capture]))
        res[("captured", capture)] = bool(step.captured)
        grads = [t.grad.detach().cpu().clone() for t in params.tensors()]
        for t in params.tensors():
            t.grad = None
        del step
    res["capture == eager"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(flats[True], flats[False]))
    # without the loss the gradient is another one: the launch reached the backward pass
    step = macx.CapturedDPTrainStep(cfg, params, bucket, B=hi - lo, S=S, N=N, global_batch=Bg, seed=11, b0=lo, capture=False, **built)
    step.load(x[0], x[1], x[2], x[3], dm, **({"kb_lengths": cut(kbl)} if with_lengths else {}))
    step.step()
    torch.cuda.synchronize()
    res["loss reaches the gradient"] = not torch.equal(bucket.flat.detach().cpu(), flats[False][0])
    for t in params.tensors():
        t.grad = None
    del step
    if rank == 0:
        # one process, the full batch: CapturedTrainStep on identically initialised parameters
        full_params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(7)).to(dev)
        full = macx.CapturedTrainStep(cfg, full_params, Bg, S, N, seed=11, att_loss=att, **built)
        full.load(vq.to(dev), words.to(dev), lengths.to(dev), kb.to(dev), (dm_full / Bg).to(dev), att_target=whole(target),
                  att_row_weights=rw.to(dev), att_step_weights=sw.to(dev), **({"kb_lengths": whole(kbl)} if with_lengths else {}))
        full.replay()
        torch.cuda.synchronize()
        want = [t.grad.detach().cpu() for t in full_params.tensors()]
        # tests/test_gpu_dp.py's criterion (the biases in front of a softmax: rounding noise on a 1e-2 floor)
        errs = {f: float((a - b).abs().max() / max(float(b.abs().max()), 1e-2)) for f, a, b in zip(params.fields, grads, want)}
        ret["errs"] = {f: e for f, e in errs.items() if e > 2e-5}
        ret["worst"] = max(errs.values())
        ret["full captured"] = bool(full.captured)
        # the shard's rows are the full batch's rows times Bg / shard (the mean is over the shard)
        rows_full = full.aux_rows.detach().cpu()[:, lo:hi] * (Bg / float(hi - lo))
        ret["rows"] = float((flats[True][2] - rows_full).abs().max() / rows_full.abs().max())
        ret["res"] = {str(k): v for k, v in res.items()}
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", DP_CASES, ids=lambda c: "%s-%s-%s" % c)
def test_captured_dp_step_with_att_loss(dev, case):
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 37500 + (os.getpid() % 2000) + 2000 * DP_CASES.index(case)
    mp.spawn(_dp_worker, args=(2, port, ret, case), nprocs=2, join=True)
    res = dict(ret["res"])
    assert res["('captured', True)"] and not res["('captured', False)"] and ret["full captured"]
    bad = [k for k, v in res.items() if not v and not k.startswith("('captured'")]
    assert not bad, bad
    assert ret["worst"] < 2e-5, dict(ret["errs"])
    assert ret["rows"] < 1e-5


# ---- the tower
def _tower_step(macx, dev, **kw):
    import test_gpu_tower_graph as tg
    net = tg.make_net(macx, dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, tg.B, tg.S, H=tg.H, W=tg.W, imageInDim=tg.CIN, seed=1234, **kw)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    return net, bucket, opt, step


def test_captured_tower_train_step_with_att_loss(macx, dev):
    import test_gpu_tower_graph as tg
    net, bucket, opt, step = _tower_step(macx, dev, att_loss=dict(on="kb", kind="ce", weight=0.1))
    N = tg.H * tg.W
    target, rw, sw = _att_inputs(dev, 3, N, None, p=tg.P, B=tg.B)
    step.load(*tg.inputs(dev, 20), att_target=target, att_row_weights=rw, att_step_weights=sw)
    state = step._state()
    runs = []
    for _ in range(3):                                                # every replay from the same restored state
        step._restore(state)
        step.replay(iteration=4)
        torch.cuda.synchronize()
        assert bits_equal((step.ce + step.aux).reshape(1), step.loss.reshape(1))
        assert float(step.aux) > 0 and abs(float(step.aux) - float(step.aux_rows.double().sum())) <= 1e-5 * float(step.aux)
        runs.append([t.clone() for t in [step.loss, step.ce, step.aux, step.aux_rows, step.logits, step.pred] + step._stepped()])
    step._restore(state)
    step.opt.advance()
    want = step._eager_reference()                                    # loss, logits, pred, _stepped(), aux, aux_rows
    eager = [want[0], step._parts[0], want[-2], want[-1], want[1], want[2]] + want[3:-2]
    for r, got in enumerate(runs):
        assert len(got) == len(eager)
        for i, (a, b) in enumerate(zip(got, eager)):
            assert bits_equal(a.reshape(-1), b.reshape(-1)), (r, i)
    step._restore(state)
    step.check()


def test_tower_self_check_leaves_the_weights_at_ones(macx, dev):
    """... and the tower's: load() without weights gives the entropy rows of unit weights on the step's own maps"""
    import test_gpu_tower_graph as tg
    net, bucket, opt, step = _tower_step(macx, dev, att_loss=dict(on="kb", kind="entropy", weight=-0.01))
    assert bool((step.att_row_weights == 1).all()) and bool((step.att_step_weights == 1).all()) and step.att_target is None
    state = step._state()
    step.load(*tg.inputs(dev, 22))
    step.replay(iteration=1)
    torch.cuda.synchronize()
    maps = torch.stack([a.detach().cpu() for a in step.cell.attentions["kb"]], dim=0)
    want = ar.rows(maps, kind="entropy", eps=1e-8, scale=-0.01 / (tg.P * tg.B))
    assert float(want.abs().min()) > 0
    assert float((step.aux_rows.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    step._restore(state)


def test_captured_tower_weight_zero_is_the_step_without_att_loss(macx, dev):
    import test_gpu_tower_graph as tg
    N = tg.H * tg.W
    target, _, sw = _att_inputs(dev, 3, N, None, p=tg.P, B=tg.B)
    data = tg.inputs(dev, 21)
    out = []
    for att in (None, dict(on="kb", kind="ce", weight=0.0)):
        net, bucket, opt, step = _tower_step(macx, dev, **({} if att is None else {"att_loss": att}))
        extra = {} if att is None else dict(att_target=target, att_row_weights=torch.zeros(tg.B, device=dev), att_step_weights=sw)
        step.load(*data, **extra)
        step.replay(iteration=0)
        torch.cuda.synchronize()
        if att is None:
            assert step.aux is None and bits_equal(step.loss.reshape(1), step.ce.reshape(1))
        else:
            assert float(step.aux) == 0.0 and bool((bits(step.aux_rows) == 0).all())
        out.append([t.clone() for t in (step.loss, step.ce, opt.flat, opt.m, opt.v, step.norm, step.logits)])
    for i, (a, b) in enumerate(zip(*out)):
        assert bits_equal(a.reshape(-1), b.reshape(-1)), i
