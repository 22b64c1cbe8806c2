"""-m gpu: macx.CapturedDPTowerTrainStep -- the whole tower's data-parallel step replayed as two or three HIP graphs between its
collectives -- on the tower of tests/test_gpu_dp.py::_tower (global batch 5, H=4, W=3, Cin=128, d=256, p=2, S=6, 7 answers, vocab 12:
the smallest shape with unequal shards, a 16-row tile edge inside a shard and a rank that can go all dead).  One process against
CapturedTowerTrainStep; two gloo ranks sharing the one GPU, shards (0,2) and (2,5), against the hand-written eager data-parallel
step (bit for bit) and against the single-process full-batch gradient (the 3e-5 bar of test_two_ranks_whole_tower_matches_the_full_batch).
The references are the existing eager paths, never the class under test.  Every worker counts dist.all_reduce."""
import datetime
import hashlib
import os
import sys
import time
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_dp import _tower

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, H, W, CIN, SEED, LR = 6, 4, 3, 128, 21, 1e-3
BAR = 3e-5                                     # max|a-b| / max(max|b|, 1e-2) per tensor: test_two_ranks_whole_tower_matches_the_full_batch
LOSS_BAR = 2e-4                                # cross-entropy moves by at most twice the largest logit change; 1e-4 is the logits bar
JOIN_SECONDS = 240                             # a rank that leaves lock step ends the test here (the group's own timeout is a minute)


# ---- what both the in-process tests and the workers use ---------------------------------------------------------------------
def bits(t):
    return t.detach().reshape(-1).contiguous().cpu()


def same_bits(a, b):
    a, b = bits(a), bits(b)
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)         # +0 and -0 differ, a NaN equals itself
    return a.shape == b.shape and bool(torch.equal(a, b))


def word_of(macx, dev, iteration):
    w = macx.graph.mix32(iteration)
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w], dtype=torch.int32, device=dev)


def bucket_order(net):
    """the tensors of a net in the order of TowerBuckets' flat buffer"""
    return list(net.out.tensors()) + list(net.cell.tensors()) + list(net.stem.tensors()) + list(net.enc.tensors())


def make_dp_step(macx, dev, lo, hi, Bg, **kw):
    net, data, _ = _tower(macx, dev)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True, exchange=False)
    opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=LR)
    step = macx.CapturedDPTowerTrainStep(net, opt, bucket, B=hi - lo, S=S, H=H, W=W, imageInDim=CIN, global_batch=Bg, b0=lo, seed=SEED, **kw)
    return net, bucket, opt, step, data


def shard(data, lo, hi, dev):
    return [t[lo:hi].to(dev) for t in data]


def stepped(bucket, opt):
    """what a step leaves: the (reduced) flat gradient, its norm, the parameters"""
    torch.cuda.synchronize()
    return dict(flat=bits(bucket.flat).clone(), norm=bits(opt.norm).clone(), params=bits(opt.flat).clone())


def differing(a, b):
    return [k for k in a if not same_bits(a[k], b[k])]


def full_batch_gradient(macx, dev, n, iteration, weights=None):
    """the reference: ONE process, the first n questions of the global batch, eager, on a twin net at its initial parameters;
    returns (loss, the gradients in the flat buffer's order)"""
    net, data, _ = _tower(macx, dev)
    img, q, lengths, ans = shard(data, 0, n, dev)
    logits = net(img, q, lengths, train=True, seed=SEED, b0=0, check_ids=False, mask_word=word_of(macx, dev, iteration))
    kw = {} if weights is None else {"weights": weights[:n].to(dev)}
    loss, _ = net.loss_and_pred(logits, ans, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), [t.grad.detach().reshape(-1).cpu().clone() for t in bucket_order(net)]


def worst_error(bucket, flat, want):
    """max over the tensors of max|a-b| / max(max|b|, 1e-2), a from the flat buffer's segments"""
    errs = []
    for i, b in enumerate(want):
        a = flat[bucket.offsets[i]:bucket.offsets[i] + b.numel()]
        errs.append(float((a - b).abs().max() / max(float(b.abs().max()), 1e-2)))
    return max(errs)


# ---- 1 and 5: one process ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_process(macx, dev):
    """shard = global = 5, b0 = 0, w = 1.0 (no scale launch), and CapturedTowerTrainStep on a twin net and optimizer"""
    net, bucket, opt, step, data = make_dp_step(macx, dev, 0, 5, 5)
    tnet, _, _ = _tower(macx, dev)
    tbucket = macx.dp.TowerBuckets(tnet, fused_gather=True)
    topt = macx.optim.FlatAdamEMA(tbucket.tensors(), lr=LR)
    twin = macx.CapturedTowerTrainStep(tnet, topt, tbucket, 5, S, H=H, W=W, imageInDim=CIN, seed=SEED)
    return (net, bucket, opt, step), (tnet, tbucket, topt, twin), shard(data, 0, 5, dev)


def test_one_process_equals_the_one_graph_step_bit_for_bit(one_process):
    (net, bucket, opt, step), (tnet, tbucket, topt, twin), x = one_process
    assert step.captured, step.verify_report
    assert twin.captured, twin.verify_report
    assert step.shard_weight == 1.0 and step.w_global is None and len(step.graphs) == 2
    states = step._state(), twin._state()
    try:
        step.load(*x)
        twin.load(*x)
        for it in range(3):
            a, b = step.step(iteration=it), twin.replay(iteration=it)
            torch.cuda.synchronize()
            pairs = {"loss": (a, b), "ce": (step.ce, twin.ce), "logits": (step.logits, twin.logits), "pred": (step.pred, twin.pred),
                     "norm": (step.norm, twin.norm), "flat": (bucket.flat, tbucket.flat), "m": (opt.m, topt.m), "v": (opt.v, topt.v),
                     "ema": (opt.ema, topt.ema)}
            bad = [k for k, (p, q) in pairs.items() if not same_bits(p, q)]
            bad += ["parameter %d" % i for i, (p, q) in enumerate(zip(net.tensors(), tnet.tensors())) if not same_bits(p, q)]
            assert not bad, (it, bad)
            assert opt.t == topt.t == it + 1 and float(a) > 0 and float(step.norm) > 0
        step.check()
    finally:
        step._restore(states[0])
        twin._restore(states[1])


def test_the_mask_word_draws_the_steps_masks(one_process):
    (_, bucket, opt, step), _, x = one_process
    state = step._state()
    try:
        step.load(*x)
        seen = []
        for it in (3, 3, 4):
            step._restore(state)
            loss = step.step(iteration=it)
            seen.append(dict(stepped(bucket, opt), loss=bits(loss).clone(), logits=bits(step.logits).clone()))
        assert not differing(seen[0], seen[1])
        assert float(seen[0]["loss"]) != float(seen[2]["loss"]), seen[2]["loss"]
    finally:
        step._restore(state)


# ---- two ranks -----------------------------------------------------------------------------------------------------------------
class CountedAllReduce:
    """dist.all_reduce, counted; keeps a clone of the last buffer of more than one element as it went IN"""

    def __init__(self):
        self.calls, self.went_in, self.real = 0, None, dist.all_reduce
        dist.all_reduce = self

    def __call__(self, t, *a, **kw):
        self.calls += 1
        if t.numel() > 1:
            self.went_in = t.detach().clone()
        return self.real(t, *a, **kw)


def _join(rank, world, port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    import macx
    return macx, torch.device("cuda:0"), CountedAllReduce()


class HandWritten:
    """the eager data-parallel step written out: net, loss_and_pred, TowerBuckets(net) with begin_step / allreduce_, opt.step -- under
    the same mask word.  weights: the step of a weighted global batch (dp.live_weight_sum, one all-reduce of the double,
    dp.shard_factor) through the same bucket, which then exchanges an unscaled buffer."""

    def __init__(self, macx, dev, lo, hi, Bg):
        self.macx, self.dev, self.lo, self.hi, self.Bg = macx, dev, lo, hi, Bg
        self.net, data, _ = _tower(macx, dev)
        self.x = shard(data, lo, hi, dev)
        self.bucket = macx.dp.TowerBuckets(self.net)
        self.opt = macx.optim.FlatAdamEMA(self.bucket.tensors(), lr=LR)

    def step(self, iteration, weights=None):
        macx, net = self.macx, self.net
        img, q, lengths, ans = self.x
        for t in net.tensors():
            t.grad = None
        shard_size, global_size = self.hi - self.lo, self.Bg
        if weights is not None:
            w_local = macx.dp.live_weight_sum(weights, torch.zeros(1, dtype=torch.float64, device=self.dev))
            w_global = w_local.clone()
            dist.all_reduce(w_global)
            shard_size, global_size = 1, 1
        logits = net(img, q, lengths, train=True, seed=SEED, b0=self.lo, check_ids=False, mask_word=word_of(macx, self.dev, iteration))
        if weights is None:
            loss, _ = net.loss_and_pred(logits, ans)
        else:
            ce, _ = net.loss_and_pred(logits, ans, weights=weights)
            loss = ce * macx.dp.shard_factor(w_local, w_global).to(torch.float32).reshape(ce.shape)
        self.bucket.begin_step(shard_size, global_size)
        loss.backward()
        self.bucket.allreduce_(shard_size, global_size)
        self.opt.step(flat_grad=self.bucket.flat)
        return stepped(self.bucket, self.opt)


def digest(t):
    return hashlib.sha256(bits(t).numpy().tobytes()).hexdigest()


def _unweighted_worker(rank, world, port, ret, captures):
    """captures[rank]: the capture= of each CapturedDPTowerTrainStep this rank builds (the ranks build equally many: lock step)"""
    try:
        macx, dev, counted = _join(rank, world, port)
        Bg = 5
        lo, hi = macx.dp.tower_slice(Bg, rank, world)
        out = {"captured": [], "differs": [], "per_step": []}
        steps = [make_dp_step(macx, dev, lo, hi, Bg, capture=c) for c in captures[rank]]
        out["captured"] = [bool(s[3].captured) for s in steps]
        out["during_construction"] = counted.calls
        hand = HandWritten(macx, dev, lo, hi, Bg)
        for s in steps:
            s[3].load(*hand.x)
        first = None
        for it in range(3):
            got = []
            for _, bucket, opt, step, _ in steps:
                calls = counted.calls
                step.step(iteration=it)
                out["per_step"].append(counted.calls - calls)
                got.append(stepped(bucket, opt))
            first = first or got[0]
            want = hand.step(it)
            if it in (0, 2):                                   # after one and after three steps
                out["differs"] += [(it, i, k) for i, g in enumerate(got) for k in differing(g, want)]
        out["params"] = digest(steps[0][2].flat)
        out["finite"] = bool(torch.isfinite(steps[0][2].flat).all())
        if rank == 0:                                          # (no collective in here: rank 1 waits at the barrier)
            _, want = full_batch_gradient(macx, dev, Bg, 0)
            out["worst"] = worst_error(steps[0][1], first["flat"], want)
        ret[rank] = out
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        ret["error of rank %d" % rank] = traceback.format_exc()
        raise


WEIGHTS = {2: [0.5, 1.0], 3: [0.5, 1.0, 1.0]}                  # one fraction and the rest ones; n = 3: live counts 2 and 1; n = 2: 2 and 0


def _weighted_worker(rank, world, port, ret):
    try:
        macx, dev, counted = _join(rank, world, port)
        Bg = 5
        lo, hi = macx.dp.tower_slice(Bg, rank, world)
        net, bucket, opt, step, data = make_dp_step(macx, dev, lo, hi, Bg, weights=True)
        out = {"captured": bool(step.captured), "during_construction": counted.calls, "graphs": len(step.graphs), "short": {}}
        state = step._state()
        x = shard(data, lo, hi, dev)
        reduced = {}
        for n in (2, 3):                                       # n = 2 first: rank 1 is all dead on its very first step
            step._restore(state)
            n_r = macx.dp.shard_count(n, lo, hi)
            if n_r == 0:
                step.load_dead()
            else:
                assert step.load(*[t[:n_r] for t in x], weights=torch.tensor(WEIGHTS[n][lo:lo + n_r])) == n_r
            calls = counted.calls
            loss = step.step(iteration=0)
            torch.cuda.synchronize()
            went_in = bits(counted.went_in)
            out["short"][n] = dict(all_reduces=counted.calls - calls, loss=float(loss), loss_is_plus_zero=same_bits(loss, torch.zeros(1)),
                                   n_r=n_r, step_n=step.n, went_in_zero=not bool(went_in.view(torch.int32).any()),
                                   went_in_finite=bool(torch.isfinite(went_in).all()), w_global=float(step.w_global),
                                   finite=bool(torch.isfinite(bucket.flat).all()))
            reduced[n] = bits(bucket.flat).clone()
        # a full batch through the same graphs, all weights ones, against the hand-written steps
        step._restore(state)
        step.load(*x)
        calls = counted.calls
        step.step(iteration=0)
        got = stepped(bucket, opt)
        out["full_all_reduces"] = counted.calls - calls
        ones = torch.ones(hi - lo, device=dev)
        out["full_differs_from_weighted_eager"] = differing(got, HandWritten(macx, dev, lo, hi, Bg).step(0, weights=ones))
        plain = HandWritten(macx, dev, lo, hi, Bg).step(0)
        out["full_same_bits_as_unweighted"] = not differing(got, plain)
        order = bucket_order(net)
        out["full_worst_against_unweighted"] = worst_error(bucket, got["flat"], [plain["flat"][o:o + t.numel()] for o, t in zip(bucket.offsets, order)])
        if rank == 0:
            for n in (2, 3):
                loss, want = full_batch_gradient(macx, dev, n, 0, weights=torch.tensor(WEIGHTS[n]))
                out["short"][n].update(reference_loss=loss, worst=worst_error(bucket, reduced[n], want))
        ret[rank] = out
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        ret["error of rank %d" % rank] = traceback.format_exc()
        raise


def two_ranks(worker, *args):
    """two spawned ranks, joined with a bound: a rank that fails or leaves lock step ends the test, it does not hang it"""
    ctx = mp.get_context("spawn")
    manager = mp.Manager()
    ret = manager.dict()
    port = 41500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=worker, args=(rank, 2, port, ret) + args) for rank in range(2)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + JOIN_SECONDS
    while any(p.is_alive() for p in procs) and time.monotonic() < deadline and not any(p.exitcode not in (None, 0) for p in procs):
        procs[0].join(0.25)
        procs[1].join(0.25)
    late = [i for i, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(10)
            if p.is_alive():
                p.kill()
                p.join()
    errors = {k: v for k, v in ret.items() if isinstance(k, str)}
    assert not errors, "\n".join("%s:\n%s" % kv for kv in errors.items())
    assert not late and [p.exitcode for p in procs] == [0, 0], ("ranks still running at the bound: %r" % late, [p.exitcode for p in procs])
    return {r: ret[r] for r in (0, 1)}


def check_unweighted(res, captures):
    print("reduced flat buffer against the full-batch gradient, worst tensor: %.3g (bar %.0e)" % (res[0]["worst"], BAR))
    for rank in (0, 1):
        out = res[rank]
        assert out["captured"] == list(captures[rank]), (rank, out["captured"])
        assert out["during_construction"] == 0, "construction issued a collective on rank %d" % rank
        assert out["per_step"] == [1] * (3 * len(captures[rank])), (rank, out["per_step"])
        assert not out["differs"], "rank %d: (step, variant, what) that differ from the hand-written eager step: %r" % (rank, out["differs"])
        assert out["finite"]
    assert res[0]["params"] == res[1]["params"], "the ranks' parameters differ after three steps"
    assert res[0]["worst"] < BAR, res[0]["worst"]


def test_two_ranks_captured_eager_parts_and_hand_written_agree(dev):
    """on each rank the captured step, the capture=False step and the hand-written eager step leave the same reduced flat buffer,
    norm and parameters bit for bit after one and after three steps (two ranks: a sum is commutative, so bucketing changes no bit);
    rank 0's parameters are rank 1's; the reduced buffer is the full-batch gradient; no collective at construction, one per step"""
    captures = ((True, False), (True, False))
    check_unweighted(two_ranks(_unweighted_worker, captures), captures)


def test_a_captured_rank_and_an_eager_parts_rank_stay_in_lock_step(dev):
    """rank 0 captured, rank 1 capture=False: the bits of the test above (each rank against the hand-written eager step)"""
    captures = ((True,), (False,))
    check_unweighted(two_ranks(_unweighted_worker, captures), captures)


def test_weighted_short_batches_and_a_dead_rank(dev):
    """weights=True.  n = 2 (rank 1 all dead through load_dead() on its very first step), n = 3 (live counts 2 and 1): the reduced
    flat buffer against ONE process's eager step over the n questions through net.loss_and_pred(..., weights=) under the 3e-5 bar, the
    ranks' loss terms summing to that step's loss within 2e-4; two all-reduces per step.  Then a full batch, all weights ones, through
    the same graphs: bit for bit the hand-written eager step of the same arithmetic (dp.live_weight_sum, dp.shard_factor, TowerBuckets).
    Against the UNWEIGHTED hand-written step it is held to the 3e-5 bar, not to bits: the weighted step multiplies the loss by the fp32
    factor 2/5 or 3/5 in front of the backward pass (TowerExchangeStep's contract: the buffer is not rescaled), the unweighted step
    multiplies the finished buffer, and the two round differently unless the factor is a power of two.  Whether the bits happened to
    agree, and every measured difference, is printed and is in the failure message.  Measured on an MI355X: worst tensor 0.0 at n = 2
    (rank 0 holds every live question, factor 1) and 5.1e-7 at n = 3; loss sums 2.181150 against 2.181150 and 2.547514 against
    2.547514 (below 3e-7); the full batch differs in bits from the unweighted step, worst tensor 4.8e-7."""
    res = two_ranks(_weighted_worker)
    said = "measured: %r" % {r: {k: v for k, v in res[r].items()} for r in res}
    print(said)
    for rank in (0, 1):
        out = res[rank]
        assert out["captured"] and out["graphs"] == 3 and out["during_construction"] == 0, said
        for n in (2, 3):
            assert out["short"][n]["all_reduces"] == 2 and out["short"][n]["finite"], said
            assert out["short"][n]["step_n"] == out["short"][n]["n_r"], said
            assert out["short"][n]["w_global"] == sum(WEIGHTS[n]), said
        assert out["full_all_reduces"] == 2, said
        assert not out["full_differs_from_weighted_eager"], said
        assert out["full_worst_against_unweighted"] < BAR, said
    dead = res[1]["short"][2]
    assert dead["n_r"] == 0 and dead["went_in_zero"] and dead["went_in_finite"] and dead["loss_is_plus_zero"], said
    assert [res[r]["short"][3]["n_r"] for r in (0, 1)] == [2, 1]
    for n in (2, 3):
        ref = res[0]["short"][n]
        assert ref["worst"] < BAR, said
        assert abs(sum(res[r]["short"][n]["loss"] for r in (0, 1)) - ref["reference_loss"]) < LOSS_BAR, said
