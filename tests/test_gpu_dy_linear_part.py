"""-m gpu: the PART form of the small linear alone (macx_linear_part; small_linear_kernel<1, true, NPT>, macx_lin_tile.hip.h) --
the backward recurrence's dy linear, whose input row of question r is the sum of chain_bwd's per-tile partials.

Reference: the plain linear (macx_linear) fed by a host-side fp32 sum of the partials, ((p0 + p1) + p2) + ... over ascending tiles
(dc_reduce_kernel's order).  The PART form promises that sum and, behind it, the plain linear's products and summation order, so both
`part_sum` and the output must be BIT-equal; no tolerance is involved.

Cases: rows 1, 5, 16, 17, 64 (a ragged block of 8 questions, two full ones, full + 1, eight blocks) x every (N, part_shift) of
N in {16, 64, 65, 196} and part_shift in {4, 5, 6} that the layout admits:
  * ((N - 2) >> part_shift) + 2 <= 6 tiles per question: N = 196 runs with 64-row tiles only (the flagship's);
  * a tile holds three slots, so it may reach into at most three questions: 2^part_shift <= 2 N, which leaves N = 16 its 16- and
    32-row tiles.
The combinations outside (N = 196 with 16- / 32-row tiles, N = 16 with 64-row tiles) must be refused, and are checked for that.
Between them a question touches 1 tile (N = 16, 64 aligned), 2 (N = 65 with 64-row tiles) and the launch's maximum (N = 196: always 4, a
question starting a multiple of 4 rows into a tile; N = 65 with 16-row tiles: 5; N = 64 with 16-row tiles: 4), starts on a tile's
first row (N = 64; N = 196, r = 16) and ends on a tile's last (N = 64; N = 196, r = 15).
One more pair, (N = 67, 16-row tiles), reaches the six tiles the kernel is built for at most (r = 5 starts on a tile's last row).
Each case runs three geometries: k = n_out = 512 (the flagship's), k = n_out = 48 (a wave without a k-group, three column tiles)
and k = 528, n_out = 32 (a single k-group in the second pass of the k loop, the odd half of its pair past the end).
Slots no question owns hold NaN: a load from one that reached a sum would show.
"""
import numpy as np
import pytest
import torch

from abi_kit import Guarded, bits_equal, ptr

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 16, 17, 64)
N_SHIFT = [(N, s) for N in (16, 64, 65, 196) for s in (4, 5, 6)] + [(67, 4)]
GEOMETRIES = ((512, 512), (48, 48), (528, 32))
MAX_TILES = 6


def _admitted(N, shift):
    return ((N - 2) >> shift) + 2 <= MAX_TILES and (1 << shift) <= 2 * N


def _tiles_of(r, N, shift):
    first = r * N
    return range(first >> shift, ((first + N - 1) >> shift) + 1)


def _slot(r, t, N, shift):
    return r - ((t << shift) // N)


def _partials(rows, N, shift, k, seed):
    """part[tiles][3][k]: random where a question owns the slot, NaN elsewhere; and the fp32 sums in ascending tile order"""
    ntile = ((rows * N - 1) >> shift) + 1
    rng = np.random.default_rng(seed)
    part = np.full((ntile, 3, k), np.nan, dtype=np.float32)
    x = np.empty((rows, k), dtype=np.float32)
    for r in range(rows):
        for j, t in enumerate(_tiles_of(r, N, shift)):
            sl = _slot(r, t, N, shift)
            assert 0 <= sl < 3
            part[t, sl] = rng.standard_normal(k).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 3))
            x[r] = part[t, sl] if j == 0 else x[r] + part[t, sl]
    return part, x


def test_cases_cover_what_they_claim():
    touched = {(N, s): {len(_tiles_of(r, N, s)) for r in range(64)} for N, s in N_SHIFT if _admitted(N, s)}
    assert sorted(touched) == [(16, 4), (16, 5), (64, 4), (64, 5), (64, 6), (65, 4), (65, 5), (65, 6), (67, 4), (196, 6)]
    assert touched[(16, 4)] == {1} and touched[(64, 6)] == {1} and touched[(65, 6)] == {2}
    assert touched[(196, 6)] == {4}
    assert max(touched[(65, 4)]) == 5 == ((65 - 2) >> 4) + 2 and max(touched[(64, 4)]) == 4
    assert max(touched[(67, 4)]) == 6 == MAX_TILES and len(_tiles_of(5, 67, 4)) == 6
    assert (16 * 196) % 64 == 0 and 17 in ROWS        # N = 196: r = 16 starts on a tile's first row, so r = 15 ends on a tile's last
    assert not _admitted(196, 4) and not _admitted(196, 5) and not _admitted(16, 6)


@pytest.mark.parametrize("N,shift", N_SHIFT)
@pytest.mark.parametrize("rows", ROWS)
def test_part_linear_is_the_plain_linear_of_the_summed_partials(macx, dev, rows, N, shift):
    L = macx._lib.lib()
    act = macx._lib.ACT["TANH"]
    for k, n_out in GEOMETRIES:
        g = torch.Generator().manual_seed(rows * 131 + N * 7 + shift + k)
        W = (torch.randn(k, n_out, generator=g) / k ** 0.5).to(dev)
        b = torch.randn(n_out, generator=g).to(dev)
        wp = torch.empty_like(W)
        macx._lib.check(L.macx_pack_weight(ptr(W), k, n_out, 0, ptr(wp), None), "pack")
        psum = Guarded(rows * k, dev)
        out = Guarded(rows * n_out, dev)
        if not _admitted(N, shift):
            junk = torch.zeros(16 * 3 * k, device=dev)
            rc = L.macx_linear_part(ptr(junk), N, shift, k, rows, ptr(wp), ptr(b), 0.25, n_out, act, ptr(psum.view), ptr(out.view), None)
            torch.cuda.synchronize()
            assert rc != 0 and psum.untouched() and out.untouched(), (N, shift, rc)
            continue
        part, x = _partials(rows, N, shift, k, seed=rows * 1009 + N * 13 + shift)
        partd = Guarded(part.size, dev, fill=float("nan"))
        partd.view.copy_(torch.from_numpy(part).reshape(-1))
        xd = torch.from_numpy(x).to(dev)
        ref = Guarded(rows * n_out, dev)
        macx._lib.check(L.macx_linear(ptr(xd), k, None, 0, rows, ptr(wp), ptr(b), 0.25, n_out, act, ptr(ref.view), None), "linear")
        macx._lib.check(L.macx_linear_part(ptr(partd.view), N, shift, k, rows, ptr(wp), ptr(b), 0.25, n_out, act, ptr(psum.view),
                                           ptr(out.view), None), "linear_part")
        torch.cuda.synchronize()
        what = "rows=%d N=%d shift=%d k=%d n_out=%d" % (rows, N, shift, k, n_out)
        assert psum.intact() and out.intact() and ref.intact(), what
        assert bits_equal(psum.np(rows, k), x), what + ": part_sum differs from the ascending-tile fp32 sum"
        assert np.isfinite(ref.np(rows, n_out)).all(), what
        assert bits_equal(out.np(rows, n_out), ref.np(rows, n_out)), what + ": output differs from the plain linear's"


def test_part_linear_guards(macx, dev):
    L = macx._lib.lib()
    k = n_out = 32
    t, w, ps, o = (torch.zeros(4096, device=dev) for _ in range(4))      # 4 rows of N = 64: 4 tiles x 3 x 32 floats of partials

    def call(**kw):
        return L.macx_linear_part(ptr(kw.get("part", t)), kw.get("N", 64), kw.get("shift", 6), kw.get("k", k), kw.get("rows", 4), ptr(w),
                                  None, 0.0, kw.get("n_out", n_out), 0, ptr(kw.get("psum", ps)), ptr(kw.get("out", o)), None)

    assert call() == 0
    for bad in (dict(rows=0), dict(rows=129), dict(k=24), dict(n_out=24), dict(shift=3), dict(shift=7), dict(N=0), dict(N=400),
                dict(N=16), dict(part=t[1:]), dict(psum=ps[1:]), dict(out=o[1:]), dict(part=None), dict(psum=None), dict(out=None)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
