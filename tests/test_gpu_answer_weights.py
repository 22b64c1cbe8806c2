"""-m gpu: per-question answer weights and partial batches.  The kernel alone (macx_answer_loss_weighted) against the fp64 restatement
of tests/answer_weights_ref.py; its autograd wrapper; and the captured tower classes built with weights=True / score=True: a short
batch against the eager step on those questions alone, dead slots that reach nothing (bit for bit), the self-checks, evaluation totals
read once per epoch, and one step at the workload's shape loaded with 39 of 64 questions.

Tolerances.  Scalar loss 1e-5 and dlogits 1e-6 absolute: the bounds of test_answer_loss_and_pred_kernel (tests/test_gpu_output.py).
All-ones weights (NULL) against macx_answer_loss at grad_scale 1: rows and pred bit for bit; dlogits * B within 2 ulp per entry -- the
new kernel multiplies by fl(1 / B) where the old one multiplies by 1, and the test multiplies by B: three roundings, at most 2.5 ulp
of the result, so two floats at most 2 apart (bit for bit when B is a power of two: asserted for B = 1 and 64).  Totals: 1e-12 relative
to fp64 sums of exact products.  Short batch against the eager short batch: logits 1e-4 absolute with identical argmax, every
parameter gradient within 3e-5 of its tensor's largest entry (GRAD_TOL of tests/test_gpu_configs.py), loss 1e-5.

Tower: B = 6, S = 7, 5 x 5 cells, 128 input channels, d = 256, p = 3 (tests/test_gpu_tower_graph.py's net, stem dropout
included); stemDropout = 1.0 only where it must be: the dead-slot test (the stem's tensor exponent cannot move) and images=2 (a stem
that drops is refused with shared images)."""
import math

import pytest
import torch

import answer_weights_ref as ref
import test_gpu_graph_lengths as gl
from test_gpu_graph_lengths import bits_equal, i32

pytestmark = pytest.mark.gpu

B, S, H, W, CIN, P, ANSWERS, N = gl.B, gl.S, gl.H, gl.W, gl.CIN, gl.P, gl.ANSWERS, gl.N
GRAD_TOL = 3e-5
SHAPES = [(1, 1), (5, 3), (64, 28), (130, 100)]
PATTERNS = ["ones", "fractions", "zero tail", "single", "zeros"]
SEED = 1234


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------------
def draw_weights(pattern, Bq, g):
    if pattern == "ones":
        return torch.ones(Bq)
    if pattern == "fractions":
        return 0.25 + torch.rand(Bq, generator=g)
    if pattern == "zero tail":                                 # every kind of "not live" behind the first half: 0, negative, NaN
        w = torch.ones(Bq)
        for i, b in enumerate(range(max(1, Bq // 2), Bq)):
            w[b] = (0.0, -1.0, float("nan"))[i % 3]
        return w
    w = torch.zeros(Bq)
    if pattern == "single":
        w[Bq // 2] = 0.7
    return w


def draw_case(Bq, A, pattern, seed=0):
    """(logits, answers, weights) on the host: a tie between two maxima in question 0 (and in question 1, inside ONE lane's columns, at
    A = 100); dead rows carry NaN logits and the label A + 7"""
    g = torch.Generator().manual_seed(1000 * Bq + 10 * A + seed)
    logits = torch.randn(Bq, A, generator=g)
    answers = torch.randint(0, A, (Bq,), generator=g, dtype=torch.int32)
    if A > 1:
        top = logits.max(dim=1).values + 1.0
        first, second = (3, 70) if A == 100 else (0, A - 1)   # A = 100: columns of two lanes, the second one in the second pass
        logits[0, first] = logits[0, second] = top[0]
        if A == 100 and Bq > 1:
            logits[1, 5] = logits[1, 69] = top[1]             # lane 5's first and second column
    weights = None if pattern is None else draw_weights(pattern, Bq, g)
    dead = ~ref.live(weights, Bq)
    logits[dead] = float("nan")
    answers[dead] = A + 7
    return logits, answers, weights


def launch(macx, dev, logits, answers, weights, totals=None, grad=True, loss=True, scale=1.0):
    """macx_answer_loss_weighted on device copies; outputs pre-filled with a sentinel.  -> rows, pred, dlogits | None, loss | None (host)"""
    L, ptr = macx._lib.lib(), macx._lib.ptr
    Bq, A = logits.shape
    lg, an = logits.to(dev), answers.to(dev)
    w = None if weights is None else weights.to(dev)
    rows = torch.full((Bq,), 7.0, device=dev)
    pred = torch.full((Bq,), -7, dtype=torch.int32, device=dev)
    dl = torch.full((Bq, A), 7.0, device=dev) if grad else None
    out = torch.full((1,), 7.0, device=dev) if loss else None
    macx._lib.check(L.macx_answer_loss_weighted(ptr(lg), ptr(an), ptr(w), Bq, A, ptr(rows), ptr(pred), ptr(dl), ptr(out), ptr(totals),
                                                scale, None), "macx_answer_loss_weighted")
    torch.cuda.synchronize()
    return rows.cpu(), pred.cpu(), None if dl is None else dl.cpu(), None if out is None else out.cpu()


def is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Bq, A", SHAPES)
def test_kernel_against_the_fp64_reference(macx, dev, Bq, A, pattern):
    logits, answers, weights = draw_case(Bq, A, pattern)
    want = ref.reference(logits, answers, weights, grad_scale=0.5)
    rows, pred, dl, loss = launch(macx, dev, logits, answers, weights, scale=0.5)
    dead = ~ref.live(weights, Bq)
    err_loss = abs(float(loss[0]) - float(want["loss"]))
    err_rows = float((rows.double() - want["rows"]).abs().max())
    err_dl = float((dl.double() - want["dlogits"]).abs().max())
    print("B %d A %d %s: loss err %.2e, rows err %.2e, dlogits err %.2e, %d dead" % (Bq, A, pattern, err_loss, err_rows, err_dl, int(dead.sum())))
    assert err_loss <= 1e-5 and err_rows <= 1e-5
    assert err_dl <= 1e-6
    assert torch.equal(pred.long(), want["pred"])                              # the first maximum; -1 in dead rows
    if A > 1 and not bool(dead[0]):
        assert int(pred[0]) == (3 if A == 100 else 0)
    assert is_plus_zero(rows[dead]) and is_plus_zero(dl[dead])                 # +0.0f by bit pattern, whatever the NaN rows held
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(rows).all()) and math.isfinite(float(loss[0]))
    if pattern == "zeros":
        assert is_plus_zero(loss) and is_plus_zero(dl) and pred.tolist() == [-1] * Bq
    # two identical calls -- the same arguments, every output asked for -- give identical bits
    again = launch(macx, dev, logits, answers, weights, scale=0.5)
    assert all(bits_equal(a, b) for a, b in zip((rows, pred, dl, loss), again))
    # every nullable output on its own: the others do not move
    rows2, pred2, none, loss2 = launch(macx, dev, logits, answers, weights, grad=False, scale=0.5)
    assert none is None and bits_equal(rows, rows2) and torch.equal(pred, pred2) and bits_equal(loss, loss2)
    rows3, pred3, dl3, none = launch(macx, dev, logits, answers, weights, loss=False, scale=0.5)
    assert none is None and bits_equal(rows, rows3) and torch.equal(pred, pred3) and bits_equal(dl, dl3)


@pytest.mark.parametrize("Bq, A", SHAPES)
def test_null_weights_are_macx_answer_loss(macx, dev, Bq, A):
    logits, answers, _ = draw_case(Bq, A, None)
    L, ptr = macx._lib.lib(), macx._lib.ptr
    lg, an = logits.to(dev), answers.to(dev)
    rows0, pred0 = torch.empty(Bq, device=dev), torch.empty(Bq, dtype=torch.int32, device=dev)
    dl0 = torch.empty(Bq, A, device=dev)
    macx._lib.check(L.macx_answer_loss(ptr(lg), ptr(an), Bq, A, ptr(rows0), ptr(pred0), ptr(dl0), 1.0, None), "macx_answer_loss")
    rows, pred, dl, loss = launch(macx, dev, logits, answers, None)
    ones = launch(macx, dev, logits, answers, torch.ones(Bq))
    assert all(bits_equal(a, b) for a, b in zip((rows, pred, dl, loss), ones))             # NULL is all ones
    assert bits_equal(rows, rows0.cpu()) and torch.equal(pred, pred0.cpu())
    a, b = (dl * float(Bq)).view(torch.int32).long(), dl0.cpu().view(torch.int32).long()
    apart = int((a - b).abs().max())
    print("B %d A %d: dlogits * B and macx_answer_loss's dlogits are at most %d ulp apart" % (Bq, A, apart))
    assert apart <= 2
    if Bq & (Bq - 1) == 0:
        assert apart == 0                                                          # a power of two: every scaling is exact
    assert abs(float(loss[0]) - float(rows0.double().mean())) <= 1e-6


def test_out_of_range_label_on_a_live_row(macx, dev):
    logits, answers, weights = draw_case(5, 3, "fractions")
    answers[2] = 3
    rows, pred, dl, loss = launch(macx, dev, logits, answers, weights)
    assert math.isnan(float(rows[2])) and is_plus_zero(dl[2]) and 0 <= int(pred[2]) < 3
    keep = torch.tensor([True, True, False, True, True])
    assert bool(torch.isfinite(rows[keep]).all()) and float(dl[keep].abs().max()) > 0 and math.isnan(float(loss[0]))


def test_invalid_arguments_launch_nothing(macx, dev):
    L, ptr = macx._lib.lib(), macx._lib.ptr
    lg, an = torch.zeros(2, 3, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    rows, pred = torch.full((2,), 7.0, device=dev), torch.full((2,), -7, dtype=torch.int32, device=dev)
    good = [ptr(lg), ptr(an), None, 2, 3, ptr(rows), ptr(pred), None, None, None, 1.0, None]
    for at, bad in ((0, None), (1, None), (5, None), (6, None), (3, 0), (4, 0), (3, -1)):
        args = list(good)
        args[at] = bad
        assert L.macx_answer_loss_weighted(*args) == -1, at                        # MACX_EINVAL
    torch.cuda.synchronize()
    assert rows.tolist() == [7.0, 7.0] and pred.tolist() == [-7, -7]


def test_totals_run_on_across_calls(macx, dev):
    totals = macx.output.AnswerTotals(dev)
    want = [0.0, 0.0, 0.0]
    for k, (shape, pattern) in enumerate((((130, 100), "fractions"), ((5, 3), "zero tail"), ((64, 28), "ones"))):
        logits, answers, weights = draw_case(*shape, pattern, seed=k)
        answers[0] = int(logits[0].argmax())                                       # at least one correct answer
        rows, pred, _, _ = launch(macx, dev, logits, answers, weights, totals=totals.tensor, grad=False)
        for i, x in enumerate(ref.sums_of(rows, pred, answers, weights)):
            want[i] += x
    got = totals.tensor.tolist()
    print("totals", got, "host sums", want)
    assert want[1] > 0 and all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, want))
    launch(macx, dev, logits, answers, weights)                                    # totals = NULL: nothing is touched
    assert totals.tensor.tolist() == got
    seen = totals.read()
    assert seen["weight"] == got[2] and seen["loss"] == got[0] / got[2] and seen["accuracy"] == got[1] / got[2]
    totals.reset()
    assert totals.read() == dict(loss=0.0, accuracy=0.0, weight=0.0)


# ---- 2. autograd ---------------------------------------------------------------------------------------------------------------------
def test_autograd_of_the_weighted_loss(macx, dev):
    logits, answers, weights = draw_case(64, 28, "zero tail")
    want = ref.reference(logits, answers, weights, grad_scale=3.0)
    x = logits.to(dev).requires_grad_(True)
    w = weights.to(dev).requires_grad_(True)                                       # data: no gradient flows to the weights
    totals = macx.output.AnswerTotals(dev)
    loss, pred = macx.output.answer_loss_and_pred(x, answers.to(dev), w, totals=totals)
    assert loss.shape == () and loss.requires_grad and not pred.requires_grad and pred.dtype == torch.int32
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(want["loss"])) <= 1e-5 and torch.equal(pred.cpu().long(), want["pred"])
    assert float((x.grad.cpu().double() - want["dlogits"]).abs().max()) <= 3e-6    # (1e-6 at the incoming gradient 3)
    assert w.grad is None and is_plus_zero(x.grad.cpu()[~ref.live(weights, 64)])
    assert abs(totals.read()["loss"] - float(want["loss"])) <= 1e-5 and totals.read()["weight"] == want["sums"][2]
    loss2, pred2 = macx.MACNetCore.loss_and_pred(x.detach(), answers.to(dev), weights.to(dev))      # the net's route, no gradient wanted
    assert bits_equal(loss2, loss.detach()) and torch.equal(pred2, pred) and not loss2.requires_grad


def test_without_weights_the_call_is_the_one_of_before(macx, dev):
    logits, answers, _ = draw_case(64, 28, None)
    L, ptr = macx._lib.lib(), macx._lib.ptr
    lg, an = logits.to(dev), answers.to(dev)
    rows0, pred0, dl0 = torch.empty(64, device=dev), torch.empty(64, dtype=torch.int32, device=dev), torch.empty(64, 28, device=dev)
    macx._lib.check(L.macx_answer_loss(ptr(lg), ptr(an), 64, 28, ptr(rows0), ptr(pred0), ptr(dl0), 1.0 / 64, None), "macx_answer_loss")
    x = lg.clone().requires_grad_(True)
    loss, pred = macx.output.answer_loss_and_pred(x, an, weights=None, totals=None)
    loss.backward()
    torch.cuda.synchronize()
    assert bits_equal(loss.detach(), rows0.mean()) and torch.equal(pred, pred0) and bits_equal(x.grad, dl0 * 1.0)


# ---- 3 - 5. the captured training step ---------------------------------------------------------------------------------------------------
class Tower:
    """a captured step and the identically initialised eager net beside it; net: option overrides of the default net"""

    def __init__(self, macx, dev, net=None, **kw):
        self.macx, self.dev = macx, dev
        net = net or {}
        self.net = gl.make_net(macx, dev, **net)
        self.bucket = macx.dp.TowerBuckets(self.net, fused_gather=True)
        self.opt = macx.optim.FlatAdamEMA(self.bucket.tensors(), lr=1e-3)
        self.before = [b.clone() for b in (self.opt.flat, self.opt.m, self.opt.v, self.opt.ema)]
        self.step = macx.CapturedTowerTrainStep(self.net, self.opt, self.bucket, B, S, H=H, W=W, imageInDim=CIN, seed=SEED, **kw)
        self.state = self.step._state()
        self.ref = gl.make_net(macx, dev, **net)
        self.rbucket = macx.dp.TowerBuckets(self.ref)                              # per-tensor copy_ gather
        self.word = torch.zeros(1, dtype=torch.int32, device=dev)

    def replay(self, iteration):
        self.step._restore(self.state)
        self.step.replay(iteration=iteration)
        torch.cuda.synchronize()

    def eager(self, iteration, images, q, lengths, ans, **groups):
        """the eager step of `ref` on exactly these questions: (logits, loss, pred, flat gradient)"""
        w = self.macx.graph.mix32(iteration)
        self.word.fill_(w - (1 << 32) if w >= (1 << 31) else w)
        n = q.shape[0]
        for t in self.ref.tensors():
            t.grad = None
        logits = self.ref(images, q, lengths, train=True, seed=SEED, check_ids=False, mask_word=self.word, **groups)
        loss, pred = self.ref.loss_and_pred(logits, ans)
        self.rbucket.begin_step(n, n)
        loss.backward()
        self.rbucket.allreduce_(n, n)
        torch.cuda.synchronize()
        return logits.detach(), loss.detach(), pred, self.rbucket.flat.clone()

    def gradient_errors(self, got, want):
        """per parameter: max |got - want| over max |want| of its slice of the flat gradient"""
        out = []
        for o, k in zip(self.bucket.offsets, self.bucket.sizes):
            a, b = got[o:o + k], want[o:o + k]
            out.append(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30))
        return out


@pytest.fixture(scope="module")
def tower(macx, dev):
    """the default net: every dropout site of the tower draws, the stem's among them"""
    t = Tower(macx, dev, weights=True, totals=True)
    assert t.net.stem.keep < 1.0
    torch.cuda.synchronize()
    t.untouched = [bits_equal(a, b) for a, b in zip(t.before, (t.opt.flat, t.opt.m, t.opt.v, t.opt.ema))] + [t.opt.t == 0]
    t.constructed = (t.step.weights.tolist(), t.step.totals.read(), t.step.n)
    return t


def test_construction_checks_itself_and_leaves_nothing_behind(tower):
    step = tower.step
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert tower.untouched == [True] * 5
    assert tower.constructed == ([1.0] * B, dict(loss=0.0, accuracy=0.0, weight=0.0), B)
    assert step.weights.dtype == torch.float32 and step.weights.shape == (B,) and step.totals.tensor.dtype == torch.float64


def check_short_batch(t, n, iteration, images, q, lengths, ans, **groups):
    step = t.step
    assert step.load(images, q, lengths, ans, **groups) == n and step.n == n
    t.replay(iteration)
    logits, loss, pred, flat = t.eager(iteration, images, q, lengths, ans, **groups)
    err_logits = float((step.logits[:n] - logits).abs().max())
    err_loss = abs(float(step.loss) - float(loss))
    errs = t.gradient_errors(t.bucket.flat, flat)
    print("n = %d: logits err %.2e, loss err %.2e, worst gradient err %.2e (parameter %d)" % (n, err_logits, err_loss, max(errs), errs.index(max(errs))))
    assert err_logits <= 1e-4 and torch.equal(step.logits[:n].argmax(dim=1), logits.argmax(dim=1))
    assert torch.equal(step.pred[:n], pred) and step.pred[n:].tolist() == [-1] * (B - n)
    assert err_loss <= 1e-5 and bits_equal(step.loss, step.ce)
    assert max(errs) <= GRAD_TOL, errs
    assert step.weights.tolist() == [1.0] * n + [0.0] * (B - n)
    step.check()


@pytest.mark.parametrize("n", [1, 4, 6])
def test_short_batch_equals_the_eager_short_batch(dev, tower, n):
    images, q, lengths, ans = gl.inputs(dev, 40 + n)
    try:
        check_short_batch(tower, n, 2, images[:n], q[:n], lengths[:n], ans[:n])
        # the static tensors follow the padding rule
        assert torch.equal(tower.step.questions.cpu(), ref.pad_slots(q[:n].cpu(), n, B))
        assert torch.equal(tower.step.lengths.cpu(), ref.pad_slots(lengths[:n].cpu(), n, B))
        assert torch.equal(tower.step.answers.cpu(), ref.pad_slots(ans[:n].cpu(), n, B))
        assert bits_equal(tower.step.images.cpu(), ref.pad_slots(images[:n].cpu(), n, B))
    finally:
        tower.step._restore(tower.state)
        tower.step.totals.reset()


@pytest.mark.parametrize("n", [1, 4, 6])
def test_short_batch_with_image_groups_and_kb_lengths(macx, dev, n, grouped_tower):
    t = grouped_tower
    assert t.step.captured, "the capture's self-check failed in this process: %r" % (t.step.verify_report,)
    images, q, lengths, ans = gl.inputs(dev, 50 + n, images=2)
    index, sizes = i32([1, 0, 1, 1, 0, 1], dev), i32([N, 1, 9, 17, 25, 4], dev)
    try:
        check_short_batch(t, n, 1, images, q[:n], lengths[:n], ans[:n], image_index=index[:n], kb_lengths=sizes[:n])
        one = gl.inputs(dev, 60 + n, images=1)[0]                                   # fewer images than the capture's two
        zero = index[:n] * 0
        assert t.step.load(one, q[:n], lengths[:n], ans[:n], image_index=zero, kb_lengths=sizes[:n]) == n
        assert bits_equal(t.step.images[1], t.step.images[0]) and bits_equal(t.step.images[0], one[0])
        with pytest.raises(IndexError, match="image_index"):                       # image 1 was not loaded
            t.step.load(one, q[:n], lengths[:n], ans[:n], image_index=zero + 1, kb_lengths=sizes[:n])
    finally:
        t.step._restore(t.state)


@pytest.fixture(scope="module")
def grouped_tower(macx, dev):
    return Tower(macx, dev, net=dict(stemDropout=1.0), weights=True, images=2, kb_lengths=True)     # (shared images: the stem must keep)


@pytest.fixture(scope="module")
def keeping_tower(macx, dev):
    """stemDropout = 1.0: the stem's one exponent per tensor cannot move with what the dead slots hold"""
    return Tower(macx, dev, net=dict(stemDropout=1.0), weights=True, totals=True)


def test_dead_slots_reach_nothing(dev, keeping_tower):
    tower = keeping_tower
    step, n = tower.step, 4
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    images, q, lengths, ans = gl.inputs(dev, 71)
    _, q2, _, ans2 = gl.inputs(dev, 72)

    def run(rewrite):
        step.load(images[:n], q[:n], lengths[:n], ans[:n])
        if rewrite:                                   # other in-range ids, lengths and answers, straight into the dead slots
            step.lengths[n:] = i32([2, 6], dev)
            step.questions[n:] = q2[n:] * (torch.arange(S, device=dev).unsqueeze(0) < step.lengths[n:].unsqueeze(1)).to(torch.int32)
            step.answers[n:] = (ans2[n:] + 1) % ANSWERS
        tower.replay(3)
        return [x.clone() for x in (step.loss, step.logits[:n], tower.bucket.flat, tower.opt.flat, step.pred)]

    try:
        first, second = run(False), run(True)
        assert not torch.equal(step.questions[n:], step.questions[:1].expand(B - n, S))           # the second load was rewritten
        for what, a, b in zip(("loss", "live logits", "flat gradient", "stepped parameters", "pred"), first, second):
            assert bits_equal(a, b), what
        assert second[4][n:].tolist() == [-1, -1] and math.isfinite(float(second[0]))
        # the captured step's own eager fallback on the same static tensors, weights [1, 1, 1, 1, 0, 0]
        assert step.weights.tolist() == [1.0] * n + [0.0] * (B - n)
        step._restore(tower.state)
        step.opt.advance()
        want = step._eager_reference()                # loss, logits, pred, norm, flat gradient, ...
        torch.cuda.synchronize()
        assert bits_equal(want[4], second[2]) and bits_equal(want[0], second[0]) and bits_equal(want[1][:n], second[1])
    finally:
        step._restore(tower.state)
        step.totals.reset()


def test_weights_rescale_the_step_and_totals_follow(dev, tower):
    """per-question weights inside a full batch: the loss is the weighted mean of the eager rows, and the totals add it up"""
    step = tower.step
    images, q, lengths, ans = gl.inputs(dev, 81)
    w = torch.tensor([1.0, 0.5, 0.0, 2.0, 1.0, 0.25])
    try:
        step.totals.reset()
        step.load(images, q, lengths, ans, weights=w)
        tower.replay(4)
        logits = tower.eager(4, images, q, lengths, ans)[0]
        want = ref.reference(logits.cpu(), ans.cpu(), w)
        assert abs(float(step.loss) - float(want["loss"])) <= 1e-5 and int(step.pred[2]) == -1
        seen = step.totals.read()
        assert abs(seen["loss"] - float(want["loss"])) <= 1e-5 and seen["weight"] == 4.75
        assert abs(seen["accuracy"] - want["sums"][1] / 4.75) <= 1e-12
        step.load(images, q, lengths, ans)                                         # weights=None: ones again
        assert step.weights.tolist() == [1.0] * B
    finally:
        step._restore(tower.state)
        step.totals.reset()


def test_self_check_with_an_attention_loss(macx, dev):
    t = Tower(macx, dev, weights=True, att_loss=dict(on="kb", kind="entropy", weight=0.1))
    step = t.step
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert step.att_row_weights.tolist() == [1.0] * B and step.weights.tolist() == [1.0] * B
    images, q, lengths, ans = gl.inputs(dev, 91)
    step.load(images[:4], q[:4], lengths[:4], ans[:4])
    assert step.att_row_weights.tolist() == [1.0] * 4 + [0.0] * 2                  # the dead slots are unsupervised as well
    t.replay(0)
    assert math.isfinite(float(step.loss)) and is_plus_zero(step.aux_rows[:, 4:].cpu()) and float(step.aux_rows[:, :4].abs().min()) > 0
    step.load(images, q, lengths, ans)                                             # a full batch afterwards: ones, not the zeros of before
    assert step.att_row_weights.tolist() == [1.0] * B


def test_a_class_built_without_weights_is_the_step_of_before(macx, dev):
    t = Tower(macx, dev)
    step = t.step
    assert step.captured and step.weights is None and step.totals is None
    ropt = macx.optim.FlatAdamEMA(t.rbucket.tensors(), lr=1e-3)
    images, q, lengths, ans = gl.inputs(dev, 20)
    step.load(images, q, lengths, ans)
    step.replay(iteration=0)
    logits, loss, pred, flat = t.eager(0, images, q, lengths, ans)
    norm = ropt.step(flat_grad=t.rbucket.flat)
    torch.cuda.synchronize()
    pairs = {"loss": (step.loss, loss), "logits": (step.logits, logits), "pred": (step.pred, pred), "norm": (step.norm, norm),
             "flat gradient": (t.bucket.flat, flat), "m": (t.opt.m, ropt.m), "v": (t.opt.v, ropt.v), "flat parameters": (t.opt.flat, ropt.flat)}
    for what, (a, b) in pairs.items():
        assert bits_equal(a.reshape(-1), b.reshape(-1)), what
    with pytest.raises(ValueError, match="weights=True"):
        step.load(images[:4], q[:4], lengths[:4], ans[:4])
    with pytest.raises(ValueError, match="weights=True"):                          # n = 1 used to be broadcast into every slot
        step.load(images[:1], q[:1], lengths[:1], ans[:1])


# ---- 6. evaluation totals ------------------------------------------------------------------------------------------------------------
def test_evaluation_totals_over_an_epoch(macx, dev):
    net = gl.make_net(macx, dev)
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN, score=True)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    assert fwd.totals.read() == dict(loss=0.0, accuracy=0.0, weight=0.0) and fwd.weights.tolist() == [1.0] * B
    batches = []
    for seed, n in ((1, 6), (2, 6), (3, 3)):
        images, q, lengths, ans = gl.inputs(dev, seed)
        batches.append((images[:n], q[:n], lengths[:n], ans[:n]))
    rows, hits = [], 0
    with torch.no_grad():
        for images, q, lengths, ans in batches:
            logits = net(images, q, lengths, train=False).cpu().double()
            rows.append(-torch.log_softmax(logits, dim=1).gather(1, ans.cpu().long().unsqueeze(1)).squeeze(1))
            hits += int((logits.argmax(dim=1) == ans.cpu().long()).sum())
    want_loss = float(torch.cat(rows).mean())
    for epoch in range(2):
        fwd.totals.reset()
        for images, q, lengths, ans in batches:
            n = q.shape[0]
            out = fwd(images, q, lengths, answers=ans)
            assert out.shape == (n, ANSWERS) and fwd.n == n and fwd.pred[n:].tolist() == [-1] * (B - n)
        seen = fwd.totals.read()                                                   # the epoch's one synchronisation
        print("epoch %d: %r; host loss %.9f, hits %d / 15" % (epoch, seen, want_loss, hits))
        assert seen["weight"] == 15.0 and seen["accuracy"] == hits / 15.0 and abs(seen["loss"] - want_loss) <= 1e-5
    with torch.no_grad():
        assert float((out - net(*batches[-1][:3], train=False)).abs().max()) <= 1e-4    # the live logits are the eager ones (logits criterion)
    with pytest.raises(TypeError, match="needs answers"):
        fwd(*batches[0][:3])
    fwd.check()


# ---- 7. the workload's shape ---------------------------------------------------------------------------------------------------------
def test_short_batch_at_the_workload_shape(macx, dev):
    import test_gpu_tower_graph as tg
    b, s, hw, cin, d, p, vocab, n = 64, 50, 14, 1024, 512, 12, 90, 39
    cfg = macx.configs.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d)
    net = macx.MACNet(cfg, vocab=vocab, generator=torch.Generator().manual_seed(0)).to(dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, b, s, H=hw, W=hw, imageInDim=cin, seed=7, verify=True, weights=True)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(3, s + 1, (n,), generator=g, dtype=torch.int32).tolist()
    assert step.load(*tg.inputs(dev, 3, b=n, s=s, lengths=lengths, hw=hw * hw, cin=cin, vocab=vocab)) == n
    loss = step.replay(iteration=0)
    step.check()
    assert math.isfinite(float(loss)) and math.isfinite(float(step.norm)) and opt.t == 1
    assert step.pred[n:].tolist() == [-1] * (b - n) and int(step.pred[:n].min()) >= 0
    assert step.weights.tolist() == [1.0] * n + [0.0] * (b - n)
