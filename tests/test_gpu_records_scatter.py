"""-m gpu: macx_records_scatter on its own, through the raw ABI.  Every comparison is bit for bit: the expected table is
tests/records_ref.py (the header's contract in numpy: slots in ascending order, later ones overwriting, .astype for the conversion)
applied to a table that holds a sentinel everywhere, so rows nobody names must keep the sentinel; every table sits between guard
bands.

Cases (steps, B, n, Q, dtype): the smallest call; the element path (n odd); the 16-byte path; the 8-byte path (n % 4 == 2); the
knowledge-base map of the flagship shape in fp16 (rows of 392 bytes: 8-byte stores on rows that start off 16 bytes); logits; the
widest map (four passes of a wave over a row); and 6000 row units, more than the capped grid's 512 x 4 waves: the stride loop.
ids (records_ref.ids_with_every_kind): -1, Q, Q + 5, -2, INT_MIN, INT_MAX, one id twice and one three times in non-adjacent slots,
as far as B has room (B < 11: the triple, -1, Q, the pair, the rest, in this order)."""
import ctypes as C

import numpy as np
import pytest
import torch

import records_ref
from abi_kit import Guarded, bits_equal, ptr

pytestmark = pytest.mark.gpu

F32, F16 = 0, 1                                       # MACX_FEATURES_F32 / _F16
TORCH = {F32: torch.float32, F16: torch.float16}
NUMPY = {F32: np.float32, F16: np.float16}
FILL = {F32: -7.03125e11, F16: -1234.0}               # the sentinel of a table and its guard bands (exact in the table's dtype)
CASES = [(1, 1, 1, 1, F32), (3, 5, 3, 7, F16), (2, 4, 4, 9, F32), (12, 64, 50, 300, F32), (12, 64, 196, 300, F16), (1, 64, 28, 100, F32),
         (4, 3, 1024, 5, F16), (2, 3000, 4, 4096, F32)]
SPECIALS = [0.0, -0.0, 1e-7, 6e-8, 1.0, 65504.0, 65520.0, float("nan"), float("inf"), float("-inf"), -65520.0, 65519.996, 5.9604645e-8,
            2.9802322e-8, 2.98023224e-8 * 1.0000001]


def source(steps, B, n, seed):
    """[steps, B, n] float32: attention-like values, with the values whose fp16 rounding is delicate sprinkled in where there is room"""
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal((steps, B, n)) * rng.choice([1e-6, 1e-3, 1.0, 300.0], size=(steps, B, 1))).astype(np.float32)
    flat = src.reshape(-1)
    if flat.size >= 4 * len(SPECIALS):
        flat[rng.choice(flat.size, size=len(SPECIALS), replace=False)] = np.array(SPECIALS, dtype=np.float32)
    return src


def call(macx, descs, ids, B, Q):
    arr = (macx._lib.MacxRecordDesc * max(1, len(descs)))()
    for a, (src, table, steps, n, dtype) in zip(arr, descs):
        a.src, a.table, a.steps, a.n, a.dtype = src.data_ptr(), table.data_ptr(), steps, n, dtype
    return macx._lib.lib().macx_records_scatter(arr, len(descs), ptr(ids), B, Q, None)


class Table:
    """a sentinel-filled [Q, steps, n] table between guard bands, `off` elements behind the 16-byte boundary"""

    def __init__(self, Q, steps, n, dtype, dev, off=0):
        self.shape, self.dtype, self.off = (Q, steps, n), dtype, off
        self.guarded = Guarded(Q * steps * n + off, dev, dtype=TORCH[dtype], fill=FILL[dtype])
        self.view = self.guarded.view[off:]

    def initial(self):
        return np.full(self.shape, FILL[self.dtype], dtype=NUMPY[self.dtype])

    def result(self):
        assert self.guarded.intact()
        if self.off:
            assert self.guarded._holds_fill(self.guarded.view[:self.off])
        return self.view.cpu().numpy().reshape(self.shape)


def device_source(src, dev, off=0):
    buf = torch.zeros(src.size + off, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[off:].copy_(torch.from_numpy(src.reshape(-1)))
    return buf[off:]


def run_one(macx, dev, src, ids, Q, dtype, off=0):
    steps, B, n = src.shape
    table = Table(Q, steps, n, dtype, dev, off)
    dsrc, dids = device_source(src, dev, off), torch.from_numpy(ids).to(dev)
    assert call(macx, [(dsrc, table.view, steps, n, dtype)], dids, B, Q) == 0
    torch.cuda.synchronize(dev)
    return table


@pytest.mark.parametrize("steps,B,n,Q,dtype", CASES)
def test_scatter_matches_the_contract_bit_for_bit(macx, dev, steps, B, n, Q, dtype):
    rng = np.random.default_rng(steps * 1000 + B)
    src, ids = source(steps, B, n, seed=n), records_ref.ids_with_every_kind(B, Q, rng)
    if B >= 11:                                                        # (the batch has room for every kind: they are all there)
        assert set(records_ref.dead_kinds(Q)) <= set(ids.tolist())
        counts = np.unique(ids[(ids >= 0) & (ids < Q)], return_counts=True)[1]
        assert (counts >= 3).any() and (counts == 2).any()
    table = run_one(macx, dev, src, ids, Q, dtype)
    want = records_ref.scatter(table.initial(), src, ids)
    got = table.result()
    assert bits_equal(got, want)
    named = np.zeros(Q, dtype=bool)
    named[ids[(ids >= 0) & (ids < Q)]] = True
    assert named.any() and bits_equal(got[~named], table.initial()[~named])          # rows nobody names keep the sentinel
    # the same call with src and table one element off the vector boundary: the narrower path, the same rows
    assert bits_equal(run_one(macx, dev, src, ids, Q, dtype, off=1).result(), want)
    # ... and identical calls give identical bits
    assert bits_equal(run_one(macx, dev, src, ids, Q, dtype).result(), got)


def test_four_descriptors_in_one_call_are_four_calls_of_one(macx, dev):
    B, Q = 64, 90
    ids = records_ref.ids_with_every_kind(B, Q, np.random.default_rng(5))
    dids = torch.from_numpy(ids).to(dev)
    shapes = [(12, 196, F16), (12, 50, F16), (12, 12, F32), (1, 28, F32)]                # kb, question, self, logits
    srcs = [source(steps, B, n, seed=40 + k) for k, (steps, n, _) in enumerate(shapes)]
    dsrcs = [device_source(s, dev) for s in srcs]
    together = [Table(Q, steps, n, dt, dev) for steps, n, dt in shapes]
    assert call(macx, [(d, t.view, steps, n, dt) for d, t, (steps, n, dt) in zip(dsrcs, together, shapes)], dids, B, Q) == 0
    torch.cuda.synchronize(dev)
    for k, (steps, n, dt) in enumerate(shapes):
        alone = Table(Q, steps, n, dt, dev)
        assert call(macx, [(dsrcs[k], alone.view, steps, n, dt)], dids, B, Q) == 0
        torch.cuda.synchronize(dev)
        want = records_ref.scatter(alone.initial(), srcs[k], ids)
        assert bits_equal(alone.result(), want) and bits_equal(together[k].result(), want), k


@pytest.mark.parametrize("n,off", [(len(SPECIALS) + 1, 0), (len(SPECIALS) + 3, 0), (len(SPECIALS) + 2, 0), (len(SPECIALS) + 1, 1)])
def test_fp16_conversion_is_torchs_cpu_conversion(macx, dev, n, off):
    """0, -0.0, subnormals (1e-7, 6e-8, the smallest and half of it: a tie to even and just above it), 1.0, 65504, 65520 (-> inf) and
    the largest float below it (-> 65504), NaN and the infinities -- on the 16-byte (n = 16), the 8-byte (n = 18) and the element
    path (n = 17, and n = 16 one element off the boundary)"""
    assert len(SPECIALS) == 15
    src = np.ones((1, 1, n), dtype=np.float32)
    src[0, 0, :len(SPECIALS)] = np.array(SPECIALS, dtype=np.float32)
    got = run_one(macx, dev, src, np.zeros(1, dtype=np.int32), 1, F16, off=off).result()
    want = torch.from_numpy(src).to(torch.float16).numpy()                             # torch's CPU conversion
    assert bits_equal(got, want)
    assert np.isnan(got[0, 0, 7]) and np.isposinf(got[0, 0, 6]) and got[0, 0, 11] == 65504.0 and np.signbit(got[0, 0, 1])
    assert got[0, 0, 2] != 0 and got[0, 0, 13] == 0 and got[0, 0, 14] != 0             # subnormals kept; the tie goes to even (zero)


def test_a_table_just_over_4_gib(macx, dev):
    """p = 12, n = 196, Q = 920 000 in fp16 is 4.33e9 bytes and 2.16e9 elements: offsets past 2^32 bytes and 2^31 elements.  The
    table is torch.empty; the named rows (the last two and row 0) and their neighbours are compared, the neighbours against a
    sentinel written in front of the call."""
    steps, n, Q, B = 12, 196, 920_000, 5
    assert Q * steps * n > 1 << 31 and Q * steps * n * 2 > 1 << 32
    try:
        table = torch.empty(Q, steps, n, dtype=torch.float16, device=dev)
    except torch.cuda.OutOfMemoryError:
        pytest.fail("4.3 GB of device memory are not available")
    near = [0, 1, 2, Q - 4, Q - 3, Q - 2, Q - 1]
    table[near] = FILL[F16]
    ids = np.array([Q - 1, 0, -1, Q - 2, Q], dtype=np.int32)
    src = source(steps, B, n, seed=3)
    assert call(macx, [(device_source(src, dev), table, steps, n, F16)], torch.from_numpy(ids).to(dev), B, Q) == 0
    torch.cuda.synchronize(dev)
    got = table[near].cpu().numpy()
    want = np.full((len(near), steps, n), FILL[F16], dtype=np.float16)
    with np.errstate(over="ignore"):                                   # (beyond 65504: an infinity, which is the contract)
        for row, slot in ((0, 1), (5, 3), (6, 0)):
            want[row] = src[:, slot, :].astype(np.float16)
    assert bits_equal(got, want)


def test_a_refused_call_leaves_the_table_untouched(macx, dev):
    steps, B, n, Q = 2, 4, 4, 9
    src, ids = device_source(source(steps, B, n, seed=1), dev), torch.arange(B, dtype=torch.int32, device=dev)
    table = Table(Q, steps, n, F32, dev)
    ok = (src, table.view, steps, n, F32)
    EINVAL = macx._lib.MACX_EINVAL
    assert call(macx, [], ids, B, Q) == EINVAL and call(macx, [ok] * 5, ids, B, Q) == EINVAL
    for bad in ((src, table.view, 0, n, F32), (src, table.view, steps, 0, F32), (src, table.view, steps, n, 2),
                (src, table.view, steps, n, -1)):
        assert call(macx, [ok, bad], ids, B, Q) == EINVAL                # a bad descriptor behind a good one: nothing is launched
    assert call(macx, [ok], ids, 0, Q) == EINVAL and call(macx, [ok], ids, B, 0) == EINVAL
    assert macx._lib.lib().macx_records_scatter(None, 1, ptr(ids), B, Q, None) == EINVAL
    torch.cuda.synchronize(dev)
    assert table.guarded.untouched()
    assert call(macx, [ok], ids, B, Q) == 0                              # (the legal call does write)
    torch.cuda.synchronize(dev)
    assert not table.guarded.untouched() and table.guarded.intact()
    assert C.sizeof(macx._lib.MacxRecordDesc) == 32
