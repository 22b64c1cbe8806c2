"""CPU: the one layout rule of the flat fp32 buffers (macx.params.FlatLayout) and everything built on it -- the cell's gradient
buffer, the dp buckets, the tower's bucket -- and, with world_size 2 over gloo, the early/late exchange that OverlappedBuckets and
TowerBuckets share: which ranges are all-reduced, in which order, asynchronously or not, and that the result is bit for bit one
plain GradBucket all-reduce.  The HIP cell cannot run here: the workers write what its backward pass would (views of the claimed
buffer, the phase-1 hook between the early and the late fields)."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cell_params(macx):
    cfg = macx.configs.flag_file_config("args", netLength=2, memDim=128, ctrlDim=128, attDim=128)
    return macx.MACCellParams(cfg, 2, generator=torch.Generator().manual_seed(7))


class _Module:
    """stand-in for the tower's other modules: a few tiny parameters, odd sizes and a 0-d scalar among them"""

    def __init__(self, shapes):
        self._tensors = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]

    def tensors(self):
        return list(self._tensors)


class _Net:
    def __init__(self, macx):
        self.out = _Module([(5, 3), (3,), ()])
        self.cell = _cell_params(macx)
        self.stem = _Module([(7,), (2, 2)])
        self.enc = _Module([(9,)])


def test_flat_layout_is_the_rule():
    """segments in order, each padded to a multiple of 4 floats; a 0-d scalar is one float"""
    import macx
    FlatLayout = macx.params.FlatLayout
    lay = FlatLayout([1, 3, 4, 5, torch.zeros(()), 2])
    assert lay.sizes == [1, 3, 4, 5, 1, 2]
    assert lay.offsets == [0, 4, 8, 12, 20, 24] and lay.total == 28
    assert [lay.prefix(k) for k in range(7)] == [0, 4, 8, 12, 20, 24, 28]
    tensors = [torch.zeros(1), torch.zeros(3), torch.zeros(2, 2), torch.zeros(5), torch.zeros(()), torch.zeros(2, 1)]
    same = FlatLayout(tensors)
    assert (same.sizes, same.offsets, same.total) == (lay.sizes, lay.offsets, lay.total)
    flat = torch.arange(28.0)
    views = [same.view(flat, i) for i in range(6)]
    assert [tuple(v.shape) for v in views] == [(1,), (3,), (2, 2), (5,), (), (2, 1)]
    assert [float(v.reshape(-1)[0]) for v in views] == [0.0, 4.0, 8.0, 12.0, 20.0, 24.0]
    assert all(same.is_view(flat, i, v) for i, v in enumerate(views))
    assert not same.is_view(flat, 1, views[2]) and not same.is_view(flat, 0, None) and not same.is_view(flat, 2, views[2].clone())
    assert not same.is_view(flat, 2, views[2].t())                  # right address, but not the contiguous segment
    assert FlatLayout([]).total == 0 and FlatLayout([]).prefix(0) == 0


def test_every_flat_consumer_has_the_same_layout():
    """MACCellParams.grad_buffer(), GradBucket, OverlappedBuckets and the cell's range of a TowerBuckets: one set of offsets"""
    import macx
    prm = _cell_params(macx)
    sizes = [t.numel() for t in prm.tensors()]
    assert any(n % 4 for n in sizes)                                # the scalar logit biases: tight packing would differ
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total)
        total += -(-n // 4) * 4
    assert prm.layout.offsets == offsets and prm.layout.sizes == sizes
    assert prm.grad_buffer().numel() == prm.layout.total == total
    one = macx.dp.GradBucket(prm.tensors(), params=prm)
    two = macx.dp.OverlappedBuckets(prm)
    for b in (one, two):
        assert b.offsets == offsets and b.sizes == sizes and b.flat.numel() == total
        assert b.flat.data_ptr() == prm.grad_buffer().data_ptr()
    n_early = sum(f not in macx.params.LATE_FIELDS for f in prm.fields)
    assert 0 < n_early < len(prm.fields) and prm.fields[n_early] in macx.params.LATE_FIELDS
    assert prm.early_floats() == offsets[n_early] == two.early
    net = _Net(macx)
    tower = macx.dp.TowerBuckets(net)
    cell = net.cell
    assert tower.offsets[:3] == [0, 16, 20] and tower.cell_lo == 24
    lo, hi = tower.n_out, tower.n_out + tower.n_cell
    assert (lo, hi - lo) == (3, len(sizes))
    assert [o - tower.cell_lo for o in tower.offsets[lo:hi]] == offsets and tower.sizes[lo:hi] == sizes
    assert tower.cell_hi - tower.cell_lo == total and tower.early == tower.cell_lo + cell.early_floats()
    assert tower.offsets[hi:] == [tower.cell_hi, tower.cell_hi + 8, tower.cell_hi + 12] and tower.flat.numel() == tower.cell_hi + 24
    # the cell's gradient buffer IS its range of the tower's, with the tower as its registered consumer
    buf = cell.grad_buffer()
    assert buf.data_ptr() == tower.flat.data_ptr() + 4 * tower.cell_lo and buf.numel() == total
    assert cell.grad_buffer_state(buf) is True and cell.grad_buffer_state(tower.flat) is None
    assert cell.claim_grad_buffer() is buf and cell.claim_grad_buffer() is None
    # a buffer nobody registered for: its owner is known, and says so
    orphan = _cell_params(macx)
    assert orphan.grad_buffer_state(orphan.grad_buffer()) is False
    assert macx.params.grad_buffer_owner(orphan.grad_buffer()) is orphan and macx.params.grad_buffer_owner(torch.zeros(4)) is None


def _backward_like_the_cell(macx, cell, tensors, values, fire):
    """what one backward pass leaves behind: the cell's gradients as views of its claimed buffer, the phase-1 hook between its early
    and its late fields (fire=False: a pass that was not split), every other module's gradient as a tensor of its own"""
    cell_tensors = cell.tensors()
    first = next(i for i, t in enumerate(tensors) if t is cell_tensors[0])
    n_early = sum(f not in macx.params.LATE_FIELDS for f in cell.fields)
    for t in tensors:
        t.grad = None
    buf = cell.claim_grad_buffer()
    assert buf is not None
    for i, t in enumerate(tensors):                                  # (backward order: classifier, cell phase 1 | 2, stem, encoder)
        k = i - first
        if 0 <= k < len(cell_tensors):
            if k == n_early and fire:
                cell.after_backward_phase1(buf)
            t.grad = cell.layout.view(buf, k)
            t.grad.copy_(values[i])
        else:
            t.grad = values[i].clone()


def _exchange(macx, bucket, cell, tensors, rank, seed, fire):
    """one step of `bucket` and the same gradients through one plain GradBucket -> (bit for bit equal, the collectives issued)"""
    g = torch.Generator().manual_seed(seed + rank)
    values = [torch.randint(-8, 9, tuple(t.shape), generator=g).float() for t in tensors]       # integers, weights 1/2: exact sums
    plain = [torch.zeros_like(t) for t in tensors]
    for t, v in zip(plain, values):
        t.grad = v.clone()
    want = macx.dp.GradBucket(plain).allreduce_(2, 4).clone()
    calls, real = [], dist.all_reduce

    def recorded(t, *args, **kw):
        calls.append(((t.data_ptr() - bucket.flat.data_ptr()) // 4, t.numel(), bool(kw.get("async_op", False))))
        return real(t, *args, **kw)

    dist.all_reduce = recorded
    try:
        bucket.begin_step(2, 4)
        _backward_like_the_cell(macx, cell, tensors, values, fire)
        got = bucket.allreduce_(2, 4)
    finally:
        dist.all_reduce = real
    same = bool(torch.equal(got, want)) and all(bool(torch.equal(t.grad, r.grad)) for t, r in zip(tensors, plain))
    views = all(t.grad.data_ptr() == bucket.flat.data_ptr() + 4 * o for t, o in zip(tensors, bucket.offsets))
    return same and views, calls


def _worker(rank, world, port, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import macx
    net = _Net(macx)
    tower = macx.dp.TowerBuckets(net)
    prm = _cell_params(macx)
    two = macx.dp.OverlappedBuckets(prm)
    out = {}
    for name, bucket, cell, tensors in (("tower", tower, net.cell, tower.tensors()), ("overlapped", two, prm, prm.tensors())):
        for seed, fire in ((100, True), (200, False), (300, True)):
            same, calls = _exchange(macx, bucket, cell, tensors, rank, seed, fire)
            out[(name, seed)] = (same, calls, bucket.overlapped_steps)
        out[(name, "ranges")] = (bucket.early, bucket.flat.numel())
    out["zero_copy"] = two.zero_copy_steps
    if rank == 0:
        ret.update({str(k): v for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 39500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    return dict(ret)


@pytest.mark.parametrize("name", ["tower", "overlapped"])
def test_two_buckets_equal_one_plain_all_reduce_bit_for_bit(two_ranks, name):
    """hook fired, hook suppressed, hook fired again: every step leaves the bits of GradBucket's single all-reduce and the
    gradients as views of the flat buffer; only the steps whose hook fired count as overlapped"""
    steps = [two_ranks[str((name, seed))] for seed in (100, 200, 300)]
    assert [s[0] for s in steps] == [True, True, True]
    assert [s[2] for s in steps] == [1, 1, 2]
    if name == "overlapped":
        assert two_ranks["zero_copy"] == 3                          # fired or not, its gradients were the buffer's own views


@pytest.mark.parametrize("name", ["tower", "overlapped"])
def test_the_collective_sequence(two_ranks, name):
    """(offset in bucket.flat, floats, async_op) of every all-reduce: the early range asynchronously, then the rest; one whole-buffer
    all-reduce when the early bucket did not start"""
    early, total = two_ranks[str((name, "ranges"))]
    assert 0 < early < total
    overlapped = [(0, early, True), (early, total - early, False)]
    fallback = [(0, total, False)]
    assert [list(two_ranks[str((name, seed))][1]) for seed in (100, 200, 300)] == [overlapped, fallback, overlapped]
