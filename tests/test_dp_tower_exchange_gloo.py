"""CPU, world_size 2 over gloo: macx.dp.TowerExchangeStep -- the host sequence of a whole-tower data-parallel step cut at its
collectives, parts and collectives in order -- driven with stand-in parts (small fp64 tensors), the weighted arithmetic of a global
batch that is short on one rank or dead altogether, and macx.dp.reduce_totals.  In the manner of tests/test_dp_gloo.py."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 9                                           # floats of the stand-in gradient
# per global slot: weights (multiples of 1/8 or not -- fp64 carries both), dealt 3 + 3
CASES = {"full": [1.0, 0.5, 1.0, 0.25, 1.0, 1.0], "short": [1.0, 0.3, 1.0, 0.7, 0.0, 0.0], "rank 1 dead": [1.0, 0.5, 0.125, 0.0, 0.0, 0.0],
         "rank 0 dead": [0.0, -1.0, 0.0, 1.0, 0.5, 0.0], "all dead": [0.0] * 6}


def question_gradients():
    """[6, K] fp64: the gradient of each global question's loss"""
    return torch.randn(6, K, generator=torch.Generator().manual_seed(11), dtype=torch.float64)


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import macx
    lo, hi = macx.dp.tower_slice(6, rank, world)
    g = question_gradients()
    log = []
    real = dist.all_reduce

    def recording(t, *a, **kw):
        log.append("all_reduce[%d]" % t.numel())
        return real(t, *a, **kw)
    macx.dp.dist.all_reduce = recording

    class Parts(macx.dp.TowerExchangeStep):
        """the three "graph replays" as stand-ins: Q sums the live weights, A writes the rank's LOCALLY normalised weighted-mean
        gradient times the factor, B "steps" (it copies the reduced buffer)"""
        weights = None

        def run_part_q(self):
            log.append("Q")
            macx.dp.live_weight_sum(self.weights, self.w_local)
            macx.dp.live_weight_sum(self.weights, self.w_global)

        def run_part_a(self):
            log.append("A")
            w = torch.where(self.weights > 0, self.weights, torch.zeros_like(self.weights)).double()
            local = (w.unsqueeze(1) * g[lo:hi]).sum(0) / w.sum() if float(w.sum()) > 0 else torch.zeros(K, dtype=torch.float64)
            self.flat_grad.copy_(local * self.factor())

        def run_part_b(self):
            log.append("B")
            self.stepped = self.flat_grad.clone()

    flat = torch.zeros(K, dtype=torch.float64)
    step = Parts(flat, None, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    out = {}
    for name, weights in CASES.items():
        del log[:]
        step.weights = torch.tensor(weights[lo:hi], dtype=torch.float32)
        got = step.exchange_step()
        out[name] = dict(order=list(log), flat=got.clone().numpy(), stepped=step.stepped.numpy(), w_local=float(step.w_local),
                         w_global=float(step.w_global), same_buffer=got is flat)
    # an unweighted step: no part Q, one collective
    del log[:]

    class Plain(Parts):
        def run_part_a(self):
            log.append("A")
            self.flat_grad.copy_(g[lo:hi].mean(0) * (float(hi - lo) / 6.0))
    plain = Plain(flat)
    out["unweighted"] = dict(order=None, flat=plain.exchange_step().clone().numpy())
    out["unweighted"]["order"] = list(log)
    # reduce_totals: one all-reduce of the three doubles; the rank's own totals stay
    del log[:]
    totals = macx.output.AnswerTotals("cpu")
    mine = [3.0, 2.0, 4.0] if rank == 0 else [1.5, 0.5, 1.0]
    totals.tensor.copy_(torch.tensor(mine, dtype=torch.float64))
    out["totals"] = dict(job=macx.dp.reduce_totals(totals), own=totals.tensor.tolist(), order=list(log))
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def run_two_ranks():
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 39500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    return {r: ret[r] for r in (0, 1)}


RESULT = {}


def result():
    if not RESULT:
        RESULT.update(run_two_ranks())
    return RESULT


def test_parts_and_collectives_run_in_order():
    for rank, out in result().items():
        for name in CASES:                      # also on a rank whose slots are all dead: every rank issues every collective
            assert out[name]["order"] == ["Q", "all_reduce[1]", "A", "all_reduce[%d]" % K, "B"], (rank, name)
            assert out[name]["same_buffer"]
        assert out["unweighted"]["order"] == ["A", "all_reduce[%d]" % K, "B"], rank


def test_weighted_step_gives_the_full_batch_weighted_mean_gradient():
    g = question_gradients().numpy()
    res = result()
    for name, weights in CASES.items():
        w = np.where(np.asarray(weights, dtype=np.float32) > 0, np.asarray(weights, dtype=np.float32), 0).astype(np.float64)
        W = w.sum()
        want = (w[:, None] * g).sum(0) / W if W > 0 else np.zeros(K)
        for rank in (0, 1):
            out = res[rank][name]
            assert np.all(np.isfinite(out["flat"])), (name, rank)
            assert out["w_global"] == W and out["w_local"] == w[3 * rank:3 * rank + 3].sum(), (name, rank)
            # fp64 rounding: a handful of operations on numbers of order 1
            assert np.max(np.abs(out["flat"] - want)) <= 8 * np.finfo(np.float64).eps * max(1.0, np.max(np.abs(want))), (name, rank)
            assert np.array_equal(out["stepped"], out["flat"])                   # part B saw the reduced buffer
        if W == 0:
            assert not res[0][name]["flat"].any() and not np.signbit(res[0][name]["flat"]).any()      # all +0, no NaN
    assert not np.array_equal(res[0]["short"]["flat"], res[0]["full"]["flat"])


def test_unweighted_step_gives_the_full_batch_mean_gradient():
    want = question_gradients().numpy().mean(0)
    for rank, out in result().items():
        assert np.max(np.abs(out["unweighted"]["flat"] - want)) <= 8 * np.finfo(np.float64).eps, rank


def test_reduce_totals_sums_the_three_doubles():
    for rank, out in result().items():
        t = out["totals"]
        assert t["job"] == dict(loss=4.5 / 5.0, accuracy=2.5 / 5.0, weight=5.0), rank
        assert t["own"] == ([3.0, 2.0, 4.0] if rank == 0 else [1.5, 0.5, 1.0])
        assert t["order"] == ["all_reduce[3]"]
