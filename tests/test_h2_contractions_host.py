"""CPU: what tests/test_gpu_h2_contractions.py rests on (tables, data, reference, restatement, bounds: h2_contraction_cases.py).

  * the case tables take the paths they name under restated launch rules (tile shapes and rings of wgrad_h2_kernel, stages and
    last-stage rows, splits, the S_b kernels' questions per group, the continuous-stream condition), and every restated rule is
    held to the C++ text: whoever edits a rule meets this file;
  * the empty splits the cell's own rule produces: the first M per width, as a recorded fact;
  * the bounds are FAIR: a numpy restatement of the kernels' arithmetic (fp16 planes, fp16 factors multiplied into both G planes
    with fp16 rounding, three terms, fp32 accumulation in the BLAS's order, summation by parts for the wide kernel) stays within
    half of every bound on every case's data, and on family a the factor term is under a tenth of the bound;
  * the bounds are SHARP: planted defects of the restatement each exceed a bound on every case where their path is live (`-s`
    prints the smallest factor per defect);
  * the size calls and every refusal of macx_h2_wgrad / macx_h2_sb (needs the built library, no device: every refused call
    returns before it touches one)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_kit
import h2_contraction_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-network_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _flat(text):
    return re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", text))


def _c_function(path, name):
    m = re.search(r"inline int %s\(.*?\n}\n" % name, _src(path), re.S)
    assert m, name
    return _flat(m.group(0))


# ---- the restated rules are the sources ------------------------------------------------------------------------------------------
def test_the_restated_rules_are_the_sources():
    h = _src("macx_wgrad_h2.hip.h")
    for line in ("inline int wgrad_h2_jw(int Jd) { return (Jd % 256 == 0) ? 2 : 1; }",
                 "inline int wgrad_h2_kw(int Kd) { return (Kd % 256 == 0) ? 2 : 1; }",
                 "inline int wgrad_h2_tiles(int Kd, int Jd) { return (Kd / (wgrad_h2_kw(Kd) * T_TILE)) * (Jd / (wgrad_h2_jw(Jd) * T_TILE)); }",
                 "template <int KW, int JW> constexpr int wh_ring() { return KW + JW == 4 ? 2 : (KW + JW == 3 ? 3 : 4); }",
                 "__host__ __device__ inline size_t wgrad_h2_mpad(size_t M) { return (M + 63) & ~(size_t)31; }",
                 "const int nchunk = (m_end - m_begin + 31) >> 5;",
                 "constexpr int SBH_MAXROWS = %d;" % hc.SBH_MAXROWS, "constexpr int SBH_MAXQ = %d;" % hc.SBH_MAXQ,
                 "constexpr int SBW_MAXQ = %d;" % hc.SBW_MAXQ, "constexpr int SBW_MAXROWS = %d;" % hc.SBW_MAXROWS,
                 "constexpr int SBH_RING = 4;", "constexpr int SBW_RING = 3;",
                 "const bool cont = sb_cont_mode() && p.nsteps > 1 && nchunk >= 3 && p.qpg * nchunk * 32 <= 512;",
                 "inline int sb_cont_mode() { return tune_get(MACX_TUNE_SB_CONT, 1); }",
                 "const float f = k < -30 ? 0.f : h2_pow2(k);"):
        assert line in h, line
    assert _c_function("macx_wgrad_h2.hip.h", "sb_h2_wide_qpg") == (
        "inlineintsb_h2_wide_qpg(intB,intN,intd){constinttiles=(d/128)*(d/256);intgroups=256/tiles;if(groups<1)groups=1;"
        "intqpg=(B+groups-1)/groups;constintrows_q=((N+31)/32)*32;constintcap=min(SBW_MAXQ,(SBW_MAXROWS/2)/rows_q);"
        "if(qpg>cap)qpg=cap;returnqpg<1?1:qpg;}")
    assert _c_function("macx_api.hip", "rows_per_split") == \
        "inlineintrows_per_split(intM,intns){intr=(M+ns-1)/ns;returnh2_mode()?(r+31)&~31:(r+1)&~1;}"
    assert _c_function("macx_api.hip", "wgrad_big_splits") == (
        "inlineintwgrad_big_splits(boolh2,intM,intKd,intJd){if(!h2)returnwgrad_splits(M,Kd,Jd);intns=256/wgrad_h2_tiles(Kd,Jd);"
        "constintmax_by_rows=(M+255)/256;if(ns>max_by_rows)ns=max_by_rows;returnns<1?1:ns;}")
    assert _c_function("macx_api.hip", "sb_qpg") == (
        "inlineintsb_qpg(boolh2,intB,intN){intqpg=(B+15)/16;if(qpg<1)qpg=1;if(h2){constintrows_q=((N+31)/32)*32;"
        "constintcap=SBH_MAXROWS/rows_q;if(qpg>cap)qpg=cap<1?1:cap;if(qpg>SBH_MAXQ)qpg=SBH_MAXQ;}returnqpg;}")
    assert ("ns_w = (wgrad_pipe_mode() >= 3 && wgrad_h2_kw(d) == 2 && wgrad_h2_jw(d) == 2 && R.ns_big >= 2) ? (int)R.ns_big / 2 : "
            "(int)R.ns_big;") in _src("macx_api.hip")
    f = _src("macx_h2.hip.h")
    assert "constexpr int H2_E_MIN = %d, H2_E_MAX = %d;" % (hc.H2_E_MIN, hc.H2_E_MAX) in f and "int e = 141 - be;" in f
    assert "constexpr int H2_PAD_ROWS = %d;" % hc.H2_PAD_ROWS in f


# ---- the tables take the paths they name -------------------------------------------------------------------------------------------
def _stages(c):
    """per non-empty split (stages, live rows of the last stage)"""
    return [((e - b + 31) >> 5, (e - b - 1) % 32 + 1) for b, e in hc.split_rows(c.nt * c.R, c.nsplit) if e > b]


def test_wgrad_table_takes_its_paths():
    form = lambda Kd, Jd: (hc.wgrad_h2_kw(Kd), hc.wgrad_h2_jw(Jd), hc.wh_ring(hc.wgrad_h2_kw(Kd), hc.wgrad_h2_jw(Jd)), hc.wgrad_h2_tiles(Kd, Jd))
    assert [form(*s) for s in hc.SHAPES] == [(1, 1, 4, 1), (2, 1, 3, 1), (1, 2, 3, 1), (2, 2, 2, 1), (1, 1, 4, 9), (2, 2, 2, 2), (2, 2, 2, 2)]
    have = {(c.Kd, c.Jd) for c in hc.WGRAD_CASES}
    assert have == set(hc.SHAPES)
    # rows per split 1 .. 161 on the ring of 4: 1 - 6 stages, last stages of 1, 31 and 32 rows, mpad's rounding on both sides of 32
    single = {c.R: c for c in hc.WGRAD_CASES if (c.Kd, c.Jd, c.nt, c.nsplit) == (128, 128, 1, 1)}
    assert sorted(single) == sorted(hc.ROWS_PER_SPLIT)
    assert [_stages(single[r])[0] for r in hc.ROWS_PER_SPLIT] == [(1, 1), (1, 31), (1, 32), (2, 1), (2, 31), (2, 32), (3, 1), (3, 32), (4, 1), (5, 1), (6, 1)]
    assert [hc.wgrad_h2_mpad(r) for r in hc.ROWS_PER_SPLIT] == [64, 64, 64, 96, 96, 96, 128, 128, 160, 192, 224]
    assert all(hc.wgrad_h2_mpad(m) >= ((m + 31) & ~31) and hc.wgrad_h2_mpad(m) % 32 == 0 for m in range(1, 700))
    for ring, shape in ((3, (256, 128)), (2, (256, 256))):          # fewer, as many and more stages than the ring holds
        n = sorted(_stages(c)[0][0] for c in hc.WGRAD_CASES if (c.Kd, c.Jd) == shape and c.nsplit == 1 and c.nt == 1)
        assert n[0] < ring <= max(n) and ring + 1 in n or ring == 2 and n[0] == 1 and max(n) > ring, (shape, n)
    # tensors: a stage that straddles two tensors (R = 49), shared and per-tensor A
    assert {(c.R, c.a_shared) for c in hc.WGRAD_CASES if c.nt == 3} >= {(32, 0), (32, 1), (49, 0), (49, 1)}
    assert 49 % 32 != 0 and (2 * 49) % 32 != 0
    # splits: ragged last splits, and the one empty split
    sp = {c.id: hc.split_rows(c.nt * c.R, c.nsplit) for c in hc.WGRAD_CASES if c.nsplit > 1}
    assert sp["128x128-nt1-R161-ns2-b"] == [(0, 96), (96, 161)] and sp["128x128-nt1-R161-ns3-d"] == [(0, 64), (64, 128), (128, 161)]
    assert sp["128x128-nt1-R64-ns3-a"] == [(0, 32), (32, 64), (64, 64)] == sp["256x256-nt1-R64-ns3-b"]
    assert (64 - 64 + 31) >> 5 == 0                                    # the kernel's stage count of that split
    assert all(b % 32 == 0 for s in sp.values() for b, _ in s)
    assert max(c.nt * c.R for c in hc.WGRAD_CASES) <= 700 and max(max(c.Kd, c.Jd) for c in hc.WGRAD_CASES) <= 512
    assert {c.fam for c in hc.WGRAD_CASES} == set(hc.FAMILIES)
    assert all(max(c.Kd, c.Jd) >= 256 for c in hc.WGRAD_CASES if c.fam == "c")


def test_empty_splits_of_the_cells_own_rule():
    """wgrad_big_splits + rows_per_split, with mode 3's halving on 256 x 256 tiles: the first M = p B N whose last split starts at or
    behind M.  The export's explicit nsplit = 3 at M = 64 sits inside what the rule produces."""
    def first_empty(d, pipe):
        for M in range(1, 70000):
            ns = hc.cell_splits(M, d, pipe)
            if (ns - 1) * hc.rows_per_split(M, ns) >= M:
                return M, ns, sum(1 for b, e in hc.split_rows(M, ns) if e <= b)
        return None
    assert first_empty(256, 3) == first_empty(512, 3) == (9217, 18, 1)
    assert first_empty(128, 3)[0] == 65537 and first_empty(128, 3)[1:] == (256, 28)
    assert hc.split_rows(9217, 18)[-1] == (17 * 544, 9217) and 17 * 544 > 9217
    # without the halving (MACX_TUNE_WGRAD_PIPE < 3) the 256-wide tiles meet their first empty split later
    assert first_empty(256, 2)[0] > 9217


def test_sb_tables_take_their_paths():
    nar, wid = hc.NARROW_CASES, hc.WIDE_CASES
    assert {c.d for c in nar} == {128, 256, 384} and {c.N for c in nar if c.d == 128} == set(hc.SB_N)
    assert {((c.N + 31) >> 5, (c.N - 1) % 32 + 1) for c in nar if c.d == 128} == {(1, 1), (1, 31), (1, 32), (2, 1), (2, 32), (3, 1), (5, 1)}
    assert {(c.B, c.qpg) for c in nar} >= {(1, 1), (4, 2), (5, 2), (5, 3)}
    assert {(c.dy, c.nsteps) for c in nar} == {(1, 1), (0, 1), (0, 3)} and {"b", "d"} <= {c.fam for c in nar}
    for c in nar:
        assert c.qpg <= hc.SBH_MAXQ and c.qpg * ((c.N + 31) // 32) * 32 <= hc.SBH_MAXROWS
    assert {c.d for c in wid} == {256, 512} and {(c.B, c.qpg) for c in wid} >= {(1, 1), (5, 2), (4, 4), (6, 4)}
    for c in wid:
        assert c.qpg <= hc.SBW_MAXQ and c.qpg * ((c.N + 31) // 32) * 32 <= hc.SBW_MAXROWS // 2 and not c.dy
    cont = [c for c in wid if hc.sb_cont(c.nsteps, c.N, c.qpg, c.cont)]
    per_step = [c for c in wid if not hc.sb_cont(c.nsteps, c.N, c.qpg, c.cont)]
    assert {c.nsteps for c in cont} == {2, 3, 5} and {c.N for c in cont} == {65, 96, 97, 129, 512}
    assert {(c.nsteps, c.N, c.cont) for c in per_step} >= {(1, 65, 1), (3, 33, 1), (3, 97, 0)}
    assert max(c.qpg * ((c.N + 31) // 32) * 32 for c in cont) == 512 and any(c.qpg * ((c.N + 31) // 32) * 32 == 480 for c in cont)
    assert any((c.N, c.qpg, c.B, c.d) == (512, 1, 1, 256) for c in cont)
    # the route plan's own choices stay inside what the exports admit
    for B in (1, 5, 64, 300):
        for N in (1, 33, 196, 512, 4096):
            assert 1 <= hc.sb_qpg(B, N) <= hc.SBH_MAXQ and hc.sb_qpg(B, N) * ((N + 31) // 32) * 32 <= hc.SBH_MAXROWS
            if N <= 512:
                q = hc.sb_h2_wide_qpg(B, N, 512)
                assert 1 <= q <= hc.SBW_MAXQ and q * ((N + 31) // 32) * 32 <= hc.SBW_MAXROWS // 2
    # equal y of two adjacent questions: one fold coefficient is exactly zero
    for c in wid:
        if c.B >= 2:
            y = hc.sb_data(c)[2]
            assert (y[0, 0] == y[0, 1]).all() and (y[0, 0] != y[0, min(2, c.B - 1)]).any() or c.B == 2


# ---- the format restated ------------------------------------------------------------------------------------------------------------
def test_split_and_join_round_trip():
    rng = np.random.RandomState(3)
    x = (rng.standard_normal((70, 256)) * np.exp2(rng.uniform(-30, 10, (70, 1)))).astype(np.float32)
    x[3] = 0
    x[5, :128] = 0
    hi, lo, e = hc.h2_split(x)
    assert e[3].tolist() == [90, 90] and e[5, 0] == 90 and e[5, 1] < 90
    mx = np.abs(x.reshape(70, 2, 128)).max(axis=2)
    scaled = mx[mx > 0] * np.exp2(e[mx > 0].astype(np.float64))
    assert (scaled >= 2.0 ** 14).all() and (scaled < 2.0 ** 15).all()
    back = hc.h2_join(hi, lo, e)
    assert np.abs(back.astype(np.float64) - x).max() <= 2.0 ** -22 * np.abs(x).max() and (back[3] == 0).all()
    h2, l2, e2 = hc.h2_split(back)                                    # the round trip is a fixed point in value: exact in fp32
    assert (hc.h2_join(h2, l2, e2) == back).all() and (e2 == e).all()
    assert hc.pow2_f16(np.array([0, -14, -24, -25, -30, -31, -200])).tolist() == [1.0, 2.0 ** -14, 2.0 ** -24, 0, 0, 0, 0]


# ---- fair and sharp ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _wgrad(c):
    if c.id not in _CACHE:
        o = hc.wgrad_operands(c, *hc.wgrad_data(c))
        _CACHE[c.id] = (o, hc.wgrad_reference(o)) + hc.wgrad_bound(c, o)
    return _CACHE[c.id]


def _sb(c):
    if c.id not in _CACHE:
        X, G, y, W = hc.sb_data(c)
        o = hc.sb_operands(c, X, G)
        _CACHE[c.id] = (o, y, W, hc.sb_reference(c, o, y, W), hc.sb_bound(c, o, y, W))
    return _CACHE[c.id]


@pytest.mark.parametrize("c", hc.WGRAD_CASES, ids=lambda c: c.id)
def test_wgrad_bound_is_fair(c):
    o, ref, bound, part2 = _wgrad(c)
    got = hc.wgrad_restate(c, o).astype(np.float64)
    r = hc.ratio(np.abs(got - ref), bound)
    assert np.isfinite(got).all() and r.max() <= 0.5, "restatement / bound %.3f" % r.max()
    assert (got[bound == 0] == 0).all() and (ref[bound == 0] == 0).all()
    if c.fam == "a":
        assert (part2 <= 0.1 * bound).all()
    if c.fam == "d":
        assert (bound[5] == 0).all() and (bound[:, 7] == 0).all() and (bound > 0).sum() == (c.Kd - 1) * (c.Jd - 1)


@pytest.mark.parametrize("c", hc.NARROW_CASES + hc.WIDE_CASES, ids=lambda c: c.id)
def test_sb_bound_is_fair(c):
    o, y, W, ref, bound = _sb(c)
    got = hc.sb_restate(c, o, y, W)
    for name, g, r, b in zip(("dW1a", "dW1b", "dy"), got, ref, bound):
        if name == "dy" and not c.dy:
            continue
        q = hc.ratio(np.abs(g.astype(np.float64) - r), b)
        assert np.isfinite(g).all() and q.max() <= 0.5, "%s: restatement / bound %.3f" % (name, q.max())
        assert (g[b == 0] == 0).all()
    if c.fam == "a":
        for b, q in zip(bound, hc.sb_bound(c, o, y, W, only_q=True)):
            assert (q <= 0.1 * b).all()
    if c.fam == "d":
        assert (bound[1][5] == 0).all() and (bound[1][:, 7] == 0).all()
        if c.B >= 2 and c.dy:
            assert (ref[2][-1, 1] == 0).all() and (bound[2][-1, 1] == 0).all()         # the all-zero question


def _minima_differ(c):
    """two questions that follow each other in a group differ in a common exponent"""
    o = _sb(c)[0]
    units = lambda s, b: np.concatenate(hc.sb_units(c, o, s, b)).tolist()
    return any(units(*g[i]) != units(*g[i + 1]) for g in hc.sb_groups(c) for i in range(len(g) - 1))


WGRAD_DEFECTS = {
    "factor_next_row": lambda c: c.fam in "bcd" and c.nt * c.R >= 2,
    "block_swap": lambda c: c.fam == "c" and c.Kd == c.Jd and c.Kd >= 256 and c.nt * c.R >= 2,
    "row_past_end": lambda c: (c.nt * c.R) % 32 != 0 and c.fam != "d",
    # (live where the kernel itself gives that row a factor of 2^-8 or more: a row far below the largest is below the bound by design)
    "row_dropped": lambda c: c.fam != "d" and hc.last_stage_weight(_wgrad(c)[0].ea[:, 0] + _wgrad(c)[0].eg[:, 0], c.nt * c.R) >= -8,
    "slab_left_out": lambda c: c.nsplit > 1,
}
SB_DEFECTS = {
    "row_past_end": lambda c: c.N % 32 != 0 and c.fam != "d",
    "row_dropped": lambda c: c.fam != "d" and max(hc.last_stage_weight(_sb(c)[0].ex[s, b][:, 0] + _sb(c)[0].eg[s, b][:, 0], c.N)
                                                   for s in range(c.nsteps) for b in range(c.B)) >= -8,
    "prev_question_min": lambda c: c.fam in "bc" and _minima_differ(c),
    "fold_yk": lambda c: c.wide and c.qpg * c.nsteps >= 2 and c.B + c.nsteps >= 3,
    "step_left_out": lambda c: c.wide and c.nsteps >= 2,
}


def test_wgrad_bound_is_sharp():
    for defect, live in WGRAD_DEFECTS.items():
        worst = []
        for c in hc.WGRAD_CASES:
            if not live(c):
                continue
            o, ref, bound, _ = _wgrad(c)
            r = hc.ratio(np.abs(hc.wgrad_restate(c, o, defect).astype(np.float64) - ref), bound).max()
            assert r > 1.0, "%s slips through on %s (%.3f of the bound)" % (defect, c.id, r)
            worst.append(r)
        assert worst
        print("\nH2X sharp wgrad %-16s live on %2d cases, exceeds a bound by at least %.3g x" % (defect, len(worst), min(worst)))


def test_sb_bound_is_sharp():
    for defect, live in SB_DEFECTS.items():
        worst = []
        for c in hc.NARROW_CASES + hc.WIDE_CASES:
            if not live(c):
                continue
            o, y, W, ref, bound = _sb(c)
            got = hc.sb_restate(c, o, y, W, defect)
            r = max(hc.ratio(np.abs(g.astype(np.float64) - rf), b).max() for g, rf, b in list(zip(got, ref, bound))[:2])
            assert r > 1.0, "%s slips through on %s (%.3f of the bound)" % (defect, c.id, r)
            worst.append(r)
        assert worst
        print("\nH2X sharp sb    %-16s live on %2d cases, exceeds a bound by at least %.3g x" % (defect, len(worst), min(worst)))


def test_a_zero_question_behind_a_live_one_keeps_the_wide_sum_finite():
    """the defect this file's GPU twin exposed: T moved into an all-zero question's unit (a factor of 2^126) went to infinity"""
    c = hc.SB_BY_ID["wide-d256-B5-N65-q2-p1-d"]
    o, y, W, ref, bound = _sb(c)
    EX, EG = hc.sb_units(c, o, 0, 1)
    assert hc.dead(EX[0], EG[0]) and not hc.dead(*[v[0] for v in hc.sb_units(c, o, 0, 0)])
    assert np.float32(2.0 ** 30) * np.float32(2.0 ** 126) == np.inf


# ---- the size calls and every refusal (the built library, no device) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def L(macx):
    return macx._lib.lib()


PTR = C.c_void_p(1 << 20)            # never dereferenced: every call below is refused on the host


def test_wgrad_size_call(macx, L):
    for c in hc.WGRAD_CASES:
        for pair in (0, 1):
            M = c.nt * c.R
            ft = -(-((c.Kd // 128) * (c.Jd // 128) * hc.wgrad_h2_mpad(M) * 2) // 16) * 4
            want = 4 * 64 * 8 + (1 + pair) * (ft + c.nsplit * c.Kd * c.Jd)
            assert L.macx_h2_wgrad_ws_floats(None, c.nt, c.R, c.Kd, c.Jd, c.nsplit, pair) == want, c.id
    # the family is forced: the answer does not depend on the process default or on opts.gemm_family
    o = abi_kit.opts(macx)
    o.gemm_family = 1
    assert L.macx_h2_wgrad_ws_floats(C.byref(o), 1, 161, 128, 128, 3, 0) == L.macx_h2_wgrad_ws_floats(None, 1, 161, 128, 128, 3, 0)
    for bad in ((0, 32, 128, 128, 1), (1, 0, 128, 128, 1), (1, 32, 64, 128, 1), (1, 32, 128, 192, 1), (1, 32, 0, 128, 1),
                (1, 32, 1152, 128, 1), (1, 32, 128, 1152, 1), (1, 32, 128, 128, 0), (1, 32, 128, 128, -1), (1, 32, 128, 128, 4097),
                (1 << 13, 1 << 12, 128, 128, 1)):
        assert L.macx_h2_wgrad_ws_floats(None, *bad, 0) == 0, bad


def _wgrad_call(L, o=None, nt=3, R=49, Kd=256, Jd=128, ns=2, a=PTR, a_stride=None, a_shared=0, g=PTR, g_stride=None, out=PTR,
                a2=None, a2_stride=0, a2_shared=0, g2=None, g2_stride=0, out2=None, ws=PTR, ws_floats=None):
    a_stride = hc.h2_floats(R, Kd) if a_stride is None else a_stride
    g_stride = hc.h2_floats(R, Jd) if g_stride is None else g_stride
    if ws_floats is None:
        ws_floats = L.macx_h2_wgrad_ws_floats(None, nt, R, Kd, Jd, max(ns, 1), int(a2 is not None)) or 1 << 24
    return L.macx_h2_wgrad(o, nt, R, Kd, Jd, ns, a, a_stride, a_shared, g, g_stride, out, a2, a2_stride, a2_shared, g2, g2_stride, out2,
                           ws, ws_floats, None)


def test_wgrad_refusals(macx, L):
    EINVAL, ESMALL = macx._lib.MACX_EINVAL, macx._lib.MACX_ESMALL
    off = C.c_void_p((1 << 20) + 4)
    sa, sg = hc.h2_floats(49, 256), hc.h2_floats(49, 128)
    P2 = C.c_void_p(1 << 21)
    bad = {
        "A NULL": dict(a=None), "G NULL": dict(g=None), "out NULL": dict(out=None), "ws NULL": dict(ws=None),
        "Kd % 128": dict(Kd=192), "Jd % 128": dict(Jd=64), "Kd = 0": dict(Kd=0), "Kd > 1024": dict(Kd=1152), "Jd > 1024": dict(Jd=1152),
        "nsplit = 0": dict(ns=0), "nsplit < 0": dict(ns=-2), "nsplit > 4096": dict(ns=5000), "nt = 0": dict(nt=0), "R = 0": dict(R=0),
        "too many rows": dict(nt=1 << 13, R=1 << 12), "A stride short": dict(a_stride=sa - 4), "G stride short": dict(g_stride=sg - 4),
        "A stride % 4": dict(a_stride=sa + 2), "G stride % 4": dict(g_stride=sg + 1), "a_shared = 2": dict(a_shared=2),
        "A off a 16-byte boundary": dict(a=off), "G off": dict(g=off), "out off": dict(out=off), "ws off": dict(ws=off),
        "half a pair: A2 only": dict(a2=P2), "half a pair: no out2": dict(a2=P2, g2=P2, a2_stride=sa, g2_stride=sg),
        "pair into one output": dict(a2=P2, g2=P2, out2=PTR, a2_stride=sa, g2_stride=sg),
        "pair, A2 stride short": dict(a2=P2, g2=P2, out2=P2, a2_stride=sa - 4, g2_stride=sg),
        "pair, G2 stride short": dict(a2=P2, g2=P2, out2=P2, a2_stride=sa, g2_stride=0),
        "pair, a2_shared = -1": dict(a2=P2, g2=P2, out2=P2, a2_stride=sa, g2_stride=sg, a2_shared=-1),
    }
    for what, kw in bad.items():
        assert _wgrad_call(L, **kw) == EINVAL, what
    need = L.macx_h2_wgrad_ws_floats(None, 3, 49, 256, 128, 2, 0)
    assert _wgrad_call(L, ws_floats=need - 1) == ESMALL
    need2 = L.macx_h2_wgrad_ws_floats(None, 3, 49, 256, 128, 2, 1)
    assert need2 > need and _wgrad_call(L, a2=P2, g2=P2, out2=P2, a2_stride=sa, g2_stride=sg, ws_floats=need2 - 1) == ESMALL
    o = abi_kit.opts(macx)
    o.abi_version = macx._lib.ABI_VERSION + 1
    assert _wgrad_call(L, o=C.byref(o)) == EINVAL and L.macx_h2_wgrad_ws_floats(C.byref(o), 3, 49, 256, 128, 2, 0) == 0
    # a shared A needs no stride; one tensor needs none at all
    assert _wgrad_call(L, a_shared=1, a_stride=0, ws_floats=need - 1) == ESMALL
    assert _wgrad_call(L, nt=1, a_stride=0, g_stride=0, ws_floats=1) == ESMALL


def test_sb_size_call(macx, L):
    for c in hc.NARROW_CASES + hc.WIDE_CASES:
        ng = (c.B + c.qpg - 1) // c.qpg
        assert L.macx_h2_sb_ws_floats(None, c.B, c.N, c.d, c.nsteps, c.qpg, c.wide) == 2 * ng * c.d * c.d, c.id
    # qpg = 0: the route plan's own choice
    for B, N, d in ((5, 33, 256), (64, 196, 512), (300, 1, 128), (1, 4096, 128)):
        q = hc.sb_qpg(B, N)
        assert L.macx_h2_sb_ws_floats(None, B, N, d, 1, 0, 0) == 2 * ((B + q - 1) // q) * d * d
    for B, N, d in ((5, 33, 256), (64, 196, 512), (300, 1, 256), (1, 512, 256), (1000, 100, 512)):
        q = hc.sb_h2_wide_qpg(B, N, d)
        assert L.macx_h2_sb_ws_floats(None, B, N, d, 3, 0, 1) == 2 * ((B + q - 1) // q) * d * d


def _sb_call(L, o=None, B=5, N=33, d=256, nsteps=1, qpg=2, wide=0, x=PTR, x_stride=None, g=PTR, g_stride=None, y=PTR, W=PTR, dA=PTR,
             dB=C.c_void_p(1 << 22), dy=None, ws=PTR, ws_floats=None):
    s = hc.h2_floats(B * N, d) if d % 128 == 0 and d > 0 and B * N > 0 else 0
    x_stride = s if x_stride is None else x_stride
    g_stride = s if g_stride is None else g_stride
    if ws_floats is None:
        ws_floats = 1 << 26
    return L.macx_h2_sb(o, B, N, d, nsteps, qpg, wide, x, x_stride, g, g_stride, y, W, dA, dB, dy, ws, ws_floats, None)


def test_sb_refusals(macx, L):
    EINVAL, ESMALL = macx._lib.MACX_EINVAL, macx._lib.MACX_ESMALL
    off = C.c_void_p((1 << 20) + 8)
    DY = C.c_void_p(1 << 23)
    bad = {
        "X NULL": dict(x=None), "dI1 NULL": dict(g=None), "y NULL": dict(y=None), "dW1a NULL": dict(dA=None), "dW1b NULL": dict(dB=None),
        "ws NULL": dict(ws=None), "dy without W1a": dict(dy=DY, W=None), "one output twice": dict(dB=PTR),
        "d % 128": dict(d=192), "d = 0": dict(d=0), "d > 1024": dict(d=1152), "B = 0": dict(B=0), "N = 0": dict(N=0), "nsteps = 0": dict(nsteps=0),
        "qpg < 0": dict(qpg=-1), "wide = 2": dict(wide=2), "too many rows": dict(B=1 << 13, N=1 << 12),
        "narrow: qpg > SBH_MAXQ": dict(B=40, N=1, qpg=33), "narrow: table rows": dict(B=40, N=129, qpg=26),
        "narrow: one question too long": dict(B=1, N=4097, qpg=1), "nsteps > 1 with dy": dict(nsteps=2, dy=DY),
        "wide: d % 256": dict(wide=1, d=384), "wide: qpg > SBW_MAXQ": dict(wide=1, N=1, qpg=5), "wide: table rows": dict(wide=1, N=129, qpg=4),
        "wide: table rows, N = 97": dict(wide=1, N=97, qpg=5), "wide: N > 512": dict(wide=1, N=513, qpg=1), "wide with dy": dict(wide=1, dy=DY),
        "X stride short": dict(nsteps=3, x_stride=hc.h2_floats(165, 256) - 4), "dI1 stride % 4": dict(nsteps=3, g_stride=hc.h2_floats(165, 256) + 2),
        "X off a 16-byte boundary": dict(x=off), "y off": dict(y=off), "dW1a off": dict(dA=off), "dy off": dict(dy=off), "ws off": dict(ws=off),
    }
    for what, kw in bad.items():
        assert _sb_call(L, **kw) == EINVAL, what
    assert 26 * 160 > hc.SBH_MAXROWS >= 25 * 160 and 4 * 160 > hc.SBW_MAXROWS // 2 >= 3 * 160
    for wide, dy in ((0, None), (0, DY), (1, None)):
        need = L.macx_h2_sb_ws_floats(None, 5, 33, 256, 1, 2, wide)
        assert need == 2 * 3 * 256 * 256 and _sb_call(L, wide=wide, dy=dy, ws_floats=need - 1) == ESMALL
    o = abi_kit.opts(macx, sb_cont=0)
    assert _sb_call(L, o=C.byref(o), ws_floats=1) == ESMALL
    o.abi_version = 4
    assert _sb_call(L, o=C.byref(o)) == EINVAL and L.macx_h2_sb_ws_floats(C.byref(o), 5, 33, 256, 1, 2, 0) == 0
