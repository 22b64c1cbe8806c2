"""The host side of the whole-tower data-parallel step that is cut at its collectives (macx.dp.TowerExchangeStep, whose order of parts
and collectives tests/test_dp_tower_exchange_gloo.py checks over two ranks): the slot-to-rank arithmetic of a short global batch
(macx.dp.shard_count), the device-scalar arithmetic of a weighted step (live_weight_sum, shard_factor), reduce_totals in one process,
and the library's export list and ABI version, which none of this touches.  No GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_signatures(macx):
    assert inspect.signature(macx.dp.reduce_totals).parameters["group"].default is None
    sig = inspect.signature(macx.dp.TowerExchangeStep.__init__).parameters
    assert list(sig)[1:] == ["flat_grad", "group", "w_local", "w_global"] and [sig[k].default for k in list(sig)[2:]] == [None] * 3
    step = macx.dp.TowerExchangeStep(torch.zeros(4))
    for part in (step.run_part_q, step.run_part_a, step.run_part_b):
        with pytest.raises(NotImplementedError):
            part()
    # CapturedTowerTrainStep is what it was: a bucket that spans processes is still refused with weights=True
    assert "global_batch" not in inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters


def test_one_process_runs_the_parts_in_order_without_a_collective(macx):
    log = []

    class Parts(macx.dp.TowerExchangeStep):
        run_part_q = lambda self: log.append("Q")
        run_part_a = lambda self: log.append("A")
        run_part_b = lambda self: log.append("B")
    flat = torch.zeros(4)
    assert Parts(flat).exchange_step() is flat and log == ["A", "B"]
    del log[:]
    sums = [torch.zeros(1, dtype=torch.float64) for _ in range(2)]
    assert Parts(flat, None, *sums).exchange_step() is flat and log == ["Q", "A", "B"]


def test_library_exports_and_abi_are_what_they_were(macx):
    assert len(macx._lib.EXPORTS) == 109 and len(set(macx._lib.EXPORTS)) == 109
    assert macx._lib.ABI_VERSION == 5 and macx._lib.lib().macx_abi_version() == 5
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "macx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(macx_\w+)\s*\(", header))
    assert set(macx._lib.EXPORTS) <= declared
    assert all(hasattr(macx._lib.lib(), n) for n in macx._lib.EXPORTS)


# ---- the slot-to-rank arithmetic of a short global batch ------------------------------------------------------------------------
@pytest.mark.parametrize("global_batch, world", [(5, 2), (7, 3), (6, 2), (10, 4)])
def test_shard_counts_of_a_short_global_batch(macx, global_batch, world):
    slices = [macx.dp.tower_slice(global_batch, r, world) for r in range(world)]
    first = slices[0][1]
    for n in sorted({0, 1, first, first + 1, global_batch - 1, global_batch}):
        counts = [macx.dp.shard_count(n, lo, hi) for lo, hi in slices]
        # global slots 0 .. n-1 are live: slot by slot
        want = [sum(1 for slot in range(lo, hi) if slot < n) for lo, hi in slices]
        assert counts == want, (n, counts, want)
        assert sum(counts) == n and all(0 <= c <= hi - lo for c, (lo, hi) in zip(counts, slices))
    assert [macx.dp.shard_count(global_batch, lo, hi) for lo, hi in slices] == [hi - lo for lo, hi in slices]


def test_shard_counts_named_cases(macx):
    count = macx.dp.shard_count
    assert [macx.dp.tower_slice(5, r, 2) for r in range(2)] == [(0, 2), (2, 5)]
    assert [[count(n, 0, 2), count(n, 2, 5)] for n in (0, 2, 3, 5)] == [[0, 0], [2, 0], [2, 1], [2, 3]]
    assert [macx.dp.tower_slice(7, r, 3) for r in range(3)] == [(0, 2), (2, 4), (4, 7)]
    assert [[count(n, 0, 2), count(n, 2, 4), count(n, 4, 7)] for n in (0, 2, 3, 7)] == [[0, 0, 0], [2, 0, 0], [2, 1, 0], [2, 2, 3]]


# ---- the device-scalar arithmetic, which is plain torch ------------------------------------------------------------------------
def test_live_weight_sum_and_shard_factor(macx):
    out = torch.full((1,), -1.0, dtype=torch.float64)
    w = torch.tensor([1.0, 0.0, -2.0, 0.375, float("nan")])
    assert macx.dp.live_weight_sum(w, out) is out and out.tolist() == [1.375]    # live: w > 0; everything else counts 0
    macx.dp.live_weight_sum(torch.zeros(4), out)
    assert out.tolist() == [0.0]
    f = lambda a, b: macx.dp.shard_factor(torch.tensor([a], dtype=torch.float64), torch.tensor([b], dtype=torch.float64))
    assert f(1.375, 1.375).tolist() == [1.0] and f(0.0, 0.0).tolist() == [0.0] and f(0.0, 2.5).tolist() == [0.0]
    assert f(1.5, 4.0).tolist() == [0.375] and f(1.5, 4.0).dtype == torch.float64
    assert f(1.5, 0.0).tolist() == [0.0]                                         # (cannot arise: W_g >= W_r; still no division by zero)


def test_reduce_totals_of_one_process_is_read(macx):
    totals = macx.output.AnswerTotals("cpu")
    totals.tensor.copy_(torch.tensor([3.0, 2.0, 4.0], dtype=torch.float64))
    assert macx.dp.reduce_totals(totals) == totals.read() == dict(loss=0.75, accuracy=0.5, weight=4.0)
    assert totals.tensor.tolist() == [3.0, 2.0, 4.0]
    totals.reset()
    assert macx.dp.reduce_totals(totals) == dict(loss=0.0, accuracy=0.0, weight=0.0)
