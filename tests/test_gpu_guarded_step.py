"""-m gpu: the guarded optimizer step (macx_adam_ema_step_g / _pg), from the raw exports to macx.CapturedTowerTrainStep.

The rule (include/macx.h): a step is skipped iff !(norm <= FLT_MAX) || (skip_above > 0 && norm > skip_above); a skipped step writes
no byte of p, m, v, ema; an applied one writes the bits of the unguarded export; guard = [applied, skipped, first, last].  Everything
here is an equality of bits or of integers: the unguarded exports are the reference (tests/test_gpu_side_kernels.py holds THEM to
fp64).  Sizes: 1000 (4 workgroups), 1024 * 256 + 1 (the first element of the grid-stride loop's second pass), 2 * 1024 * 256 + 77."""
import functools
import math

import pytest
import torch

from abi_kit import bits_equal, ptr
from test_gpu_tower_graph import ANSWERS, B, CIN, H, LENGTHS, S, VOCAB, W, make_net

pytestmark = pytest.mark.gpu

PASS = 1024 * 256
SIZES = (1000, PASS + 1, 2 * PASS + 77)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
SLOTS = ("p", "m", "v", "ema")


@functools.lru_cache(maxsize=None)
def host_state(n):
    """ONE random state per size (host tensors, never written): N(0,1) gradient -- its norm, sqrt(n) > 8, makes the clip live --
    moments at the gradient's scale, the shadow a little off the parameters"""
    gen = torch.Generator().manual_seed(777 + n)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float32)
    p = r()
    return dict(p=p, g=r(), m=0.1 * r(), v=(0.1 * r()).square(), ema=p + 0.01 * r())


class Run:
    """device copies of the state of size n, and the four exports on them"""

    def __init__(self, macx, dev, n, clip=8.0, decay=0.999):
        self.macx, self.dev, self.n, self.clip, self.decay = macx, dev, n, clip, decay
        self.t = {k: host_state(n)[k].to(dev) for k in SLOTS}
        self.ws, self.norm = torch.empty(1024, device=dev), torch.full((1,), -1.0, device=dev)
        self.guard = torch.zeros(4, dtype=torch.int32, device=dev)
        self.rate = torch.zeros(1, device=dev)

    def step(self, g, step, guarded, device_rate, skip_above=0.0):
        L, lib, t = self.macx._lib.lib(), self.macx._lib, self.t
        head = (self.n, ptr(t["p"]), ptr(g), ptr(t["m"]), ptr(t["v"]), ptr(t["ema"]))
        tail = (self.clip, self.decay) + ((skip_above, ptr(self.guard)) if guarded else ()) + (ptr(self.ws), ptr(self.norm), None)
        h = HYPER
        if device_rate:
            self.rate.fill_(self.macx.optim.FlatAdamEMA.bias_corrected_lr(h["lr"], h["beta1"], h["beta2"], step))
            f = L.macx_adam_ema_step_pg if guarded else L.macx_adam_ema_step_p
            lib.check(f(*head, ptr(self.rate), h["beta1"], h["beta2"], h["eps"], *tail), "step_p")
        else:
            f = L.macx_adam_ema_step_g if guarded else L.macx_adam_ema_step
            lib.check(f(*head, h["lr"], h["beta1"], h["beta2"], h["eps"], step, *tail), "step")
        torch.cuda.synchronize()
        return self

    def words(self):
        return self.guard.tolist()

    def same_state(self, other):
        return [k for k in SLOTS if not bits_equal(self.t[k], other.t[k] if isinstance(other, Run) else other[k])]


def grad(dev, n, poison=None):
    g = host_state(n)["g"].clone()
    if poison == "nan0":
        g[0] = math.nan
    elif poison == "nan_last":                   # (n > PASS: an element of the second or third pass)
        g[n - 1] = math.nan
    elif poison == "+inf":
        g[n // 2] = math.inf
    elif poison == "-inf":
        g[n // 3] = -math.inf
    elif poison == "3e19":                       # finite, and its square is no fp32: the sum of squares overflows
        g[n // 5] = 3e19
    else:
        assert poison is None
    return g.to(dev)


# ---- 1. an applied step is the unguarded step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.999, -1.0])
@pytest.mark.parametrize("clip", [8.0, 0.0])
@pytest.mark.parametrize("device_rate", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_applied_step_is_the_unguarded_step(macx, dev, n, device_rate, clip, decay):
    g = grad(dev, n)
    plain = Run(macx, dev, n, clip, decay).step(g, 3, False, device_rate)
    guarded = Run(macx, dev, n, clip, decay).step(g, 3, True, device_rate)
    assert guarded.same_state(plain) == [] and bits_equal(guarded.norm, plain.norm)
    assert guarded.words() == [1, 0, 0, 0]
    assert bits_equal(g.cpu(), host_state(n)["g"])                          # the gradient is read only
    changed = plain.same_state(host_state(n))                              # (the reference did step)
    assert changed == (["p", "m", "v", "ema"] if decay >= 0 else ["p", "m", "v"])
    assert math.isfinite(float(plain.norm)) and (float(plain.norm) > 8.0)   # the clip is live where it is on


# ---- 2. a poisoned gradient is skipped ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["nan0", "nan_last", "+inf", "-inf", "3e19"])
@pytest.mark.parametrize("device_rate", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_poisoned_step_is_skipped_and_counted(macx, dev, n, device_rate, poison):
    bad, good = grad(dev, n, poison), grad(dev, n)
    if poison == "3e19":
        assert bool(torch.isfinite(bad).all())
    run = Run(macx, dev, n).step(bad, 3, True, device_rate)
    assert run.same_state(host_state(n)) == []                             # p, m, v, ema bit for bit as before
    assert not math.isfinite(float(run.norm))
    assert run.words() == [0, 1, 1, 1]
    # the same state goes on: attempt 2 is finite and is the unguarded step 4 of that state ...
    run.step(good, 4, True, device_rate)
    plain = Run(macx, dev, n).step(good, 4, False, device_rate)
    assert run.words() == [1, 1, 1, 1]
    assert run.same_state(plain) == [] and bits_equal(run.norm, plain.norm)
    # ... and attempt 3 is poisoned again
    run.step(bad, 5, True, device_rate)
    assert run.words() == [1, 2, 1, 3]
    assert run.same_state(plain) == [] and not math.isfinite(float(run.norm))


# ---- 3. the threshold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_rate", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_skip_above_is_strictly_greater(macx, dev, n, device_rate):
    g = grad(dev, n)
    plain = Run(macx, dev, n).step(g, 3, False, device_rate)
    N = float(plain.norm)                                                   # (an fp32 value: 2 N and N / 2 are exact)
    assert math.isfinite(N) and N > 0
    for threshold in (2 * N, N):                                            # norm > skip_above is false for both: applied
        run = Run(macx, dev, n).step(g, 3, True, device_rate, skip_above=threshold)
        assert run.same_state(plain) == [] and bits_equal(run.norm, plain.norm), threshold
        assert run.words() == [1, 0, 0, 0]
    run = Run(macx, dev, n).step(g, 3, True, device_rate, skip_above=N / 2)
    assert run.same_state(host_state(n)) == [] and float(run.norm) == N
    assert run.words() == [0, 1, 1, 1]
    run.step(grad(dev, n, "nan0"), 4, True, device_rate, skip_above=2 * N)  # (a threshold does not switch the first clause off)
    assert run.same_state(host_state(n)) == [] and run.words() == [0, 2, 1, 2]


# ---- 4. optim.FlatAdamEMA(guard=True) ----------------------------------------------------------------------------------------------------
def flat_optimizer(macx, dev, **kw):
    gen = torch.Generator().manual_seed(31)
    params = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in ((5, 7), (3,), (130, 9), (1,))]
    return macx.optim.FlatAdamEMA(params, lr=1e-3, **kw)


def test_flat_adam_ema_guard(macx, dev):
    opt, twin = flat_optimizer(macx, dev, guard=True), flat_optimizer(macx, dev)
    assert twin.guard is None and opt.guard.dtype == torch.int32 and opt.guard_counts() == (0, 0, 0, 0)
    with pytest.raises(ValueError, match="guard=True"):
        twin.guard_counts()
    before = [b.clone() for b in (opt.flat, opt.m, opt.v, opt.ema)]
    untouched = lambda: all(bits_equal(a, b) for a, b in zip(before, (opt.flat, opt.m, opt.v, opt.ema)))
    nan = torch.zeros_like(opt.flat)
    nan[17] = math.nan
    norm = opt.step(flat_grad=nan)
    assert math.isnan(float(norm)) and untouched() and opt.guard_counts() == (0, 1, 1, 1) and opt.t == 1
    opt.advance()
    opt.step(flat_grad=nan, device_lr=True)
    counts = opt.guard_counts()
    assert untouched() and counts == (0, 2, 1, 2) and (counts.applied, counts.skipped, counts.first, counts.last) == (0, 2, 1, 2)
    assert opt.t == 2                                                       # t counts attempts
    for p in opt.params:                                                    # the gather route: .grad of every parameter, one of them infinite
        p.grad = torch.ones_like(p)
    opt.params[2].grad[4, 4] = math.inf
    opt.step()
    assert untouched() and opt.guard_counts() == (0, 3, 1, 3) and opt.t == 3
    # a finite step applies, with the bits of the unguarded optimizer at the same attempt count
    g = torch.randn(opt.flat.numel(), generator=torch.Generator().manual_seed(5)).to(dev)
    twin.t = 3
    for o in (opt, twin):
        o.advance()
        o.step(flat_grad=g, device_lr=True)
    assert opt.t == twin.t == 4 and opt.guard_counts() == (1, 3, 1, 3) and not untouched()
    assert all(bits_equal(a, b) for a, b in zip((opt.flat, opt.m, opt.v, opt.ema, opt.norm), (twin.flat, twin.m, twin.v, twin.ema, twin.norm)))
    opt.reset_guard()
    assert opt.guard_counts() == (0, 0, 0, 0)
    limited = flat_optimizer(macx, dev, guard=True, skip_above=1e-3)        # the threshold travels
    limited.step(flat_grad=g)
    assert limited.guard_counts() == (0, 1, 1, 1) and bits_equal(limited.flat, before[0])


# ---- 5. the whole path: a poisoned replay costs one skipped update ---------------------------------------------------------------------------
QN, IMAGES = 9, 4


def tower_step(macx, dev):
    """the small tower with its images in a FeatureStore and its questions in a QuestionStore: a question id outside the store names
    image row -1, whose features are gathered as NaN -- the poison reaches every gradient.  (Without a feature store such an id only
    turns the LABEL into -1: a NaN loss and, as in the reference's loss, NO gradient row -- the step's gradient is then the finite
    one of the other questions, and applying it is right.)"""
    gen = torch.Generator().manual_seed(23)
    lengths = torch.tensor(LENGTHS + [4, 6, 2], dtype=torch.int32)
    q = torch.randint(1, VOCAB + 1, (QN, S), generator=gen, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    qs = macx.QuestionStore(q, lengths, answers=torch.randint(0, ANSWERS, (QN,), generator=gen, dtype=torch.int32),
                            image_rows=torch.randint(0, IMAGES, (QN,), generator=gen, dtype=torch.int32), device=dev)
    feats = macx.FeatureStore(IMAGES, H, W, CIN, dtype=torch.float32, device=dev)
    feats.write(0, torch.relu(torch.randn(IMAGES, CIN, H, W, generator=gen))).check()
    net = make_net(macx, dev, seed=0)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3, guard=True)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, seed=1234, features=feats, questions=qs, weights=True)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    return step, opt, qs


def test_poisoned_replay_costs_one_skipped_update(macx, dev):
    clean = torch.tensor([0, 7, 2, 8, 4, 5], dtype=torch.int32, device=dev)
    state = lambda o: [b.clone() for b in (o.flat, o.m, o.v, o.ema)]
    # A: a poisoned batch, then a clean one
    a, opt_a, qs_a = tower_step(macx, dev)
    assert opt_a.guard_counts() == (0, 0, 0, 0) and opt_a.t == 0           # constructed: nothing trained, nothing skipped
    before = state(opt_a)
    poisoned = clean.clone()
    poisoned[3] = QN + 5                                                    # never dereferenced: the question is poisoned, `bad` is set
    a.load_ids(poisoned, check_ids=False)
    loss = a.replay(iteration=0)
    torch.cuda.synchronize()
    assert math.isnan(float(loss)) and math.isnan(float(a.norm))
    assert all(bits_equal(x, y) for x, y in zip(before, state(opt_a)))
    assert all(bits_equal(opt_a.layout.view(before[0], i), p.data) for i, p in enumerate(opt_a.params))     # ... and so is the net
    assert opt_a.guard_counts() == (0, 1, 1, 1) and opt_a.t == 1
    with pytest.raises(ValueError, match="outside"):
        qs_a.check()
    qs_a.reset_bad()
    a.load_ids(clean)
    loss_a = a.replay(iteration=1).clone()
    # B: never saw the poisoned batch; its attempt count is set by hand
    b, opt_b, qs_b = tower_step(macx, dev)
    opt_b.t += 1
    b.load_ids(clean)
    loss_b = b.replay(iteration=1).clone()
    torch.cuda.synchronize()
    assert a.captured and b.captured
    assert math.isfinite(float(loss_a)) and bits_equal(loss_a, loss_b)
    for name, x, y in zip(("params", "m", "v", "ema"), state(opt_a), state(opt_b)):
        assert bits_equal(x, y), name
    assert not bits_equal(before[0], opt_a.flat)                            # (the clean step trained)
    assert opt_a.guard_counts() == (1, 1, 1, 1) and opt_b.guard_counts() == (1, 0, 0, 0) and opt_a.t == opt_b.t == 2
    assert qs_a.check() is qs_a and qs_b.check() is qs_b
