"""CPU: what tests/test_gpu_stem_geometry.py rests on (cases, data, metrics: stem_geometry_cases.py).

  * every route the case table names -- tile height per launch, chain or not, slabs, rows per slab, empty slabs, JW -- against a Python
    restatement of conv_splits / rows_per_split / kb_gemm_pick_rt; the restatements against the library (conv_splits through
    macx_stem_ws_floats, the other two through the text of the C++ rules), so that an edit which retires an edge fails here;
  * the inputs are fair under the finer metrics (per image, per tap): the oracle in fp32 stays within a third of every tolerance;
  * the magic division of the CONV kernel-gradient kernels: stem_check refuses every batch whose largest flattened row the division
    would not serve, for every N the stem admits."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stem_geometry_cases as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-network_amd", "csrc")


@pytest.fixture(scope="module")
def L(macx):
    return macx._lib.lib()


def shapes(macx, B, H, W, Cin=128, Cmid=128, Cout=128, b0=0):
    return macx._lib.MacxStemShapes(B=B, H=H, W=W, Cin=Cin, Cmid=Cmid, Cout=Cout, b0=b0)


# ---- the table ------------------------------------------------------------------------------------------------------------
ISSUE_PER_IMAGE = [(1, 1, 2), (2, 3, 3), (3, 1, 17), (2, 3, 11), (2, 5, 13), (5, 1, 113), (2, 13, 16), (2, 11, 19), (1, 15, 15), (1, 8, 32),
                   (1, 32, 32), (32, 9, 9), (21, 14, 14)]
ISSUE_CHAIN = [(1, 1, 2), (1, 7, 9), (1, 8, 8), (1, 5, 13), (3, 5, 5), (1, 15, 15), (2, 11, 19)]


def test_table_holds_the_issue_cases():
    key = lambda c: (c.B, c.H, c.W, c.Cin, c.Cmid, c.Cout)
    have = {key(c) for c in sg.CASES}
    for b, h, w in ISSUE_PER_IMAGE:
        ch = (128, 256, 384) if h * w in (208, 209, 225) else (128, 128, 128)
        assert (b, h, w) + ch in have
    for b, h, w in ISSUE_CHAIN:
        assert (b, h, w, 256, 512, 512) in have
    assert (1, 5, 13, 256, 512, 256) in have
    assert max(c.N for c in sg.CASES) == sg.K_MAXN and max(c.M * 9 * c.Cin * c.Cmid for c in sg.PER_IMAGE[:13]) == 4116 * 1152 * 128


@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c.id)
def test_case_takes_the_route_its_row_names(case):
    for family in (2, 1, 0):
        assert sg.route(case, family) == case.expect[family], (case.id, family)


def _c_nchunk(m_begin, m_end):
    """wgrad_split_body (both operand formats): nchunk = (m_end - m_begin + 31) >> 5 (arithmetic shift), nloop = (nchunk + 2) / 3 * 3 (C division)"""
    nchunk = (m_end - m_begin + 31) >> 5
    q = abs(nchunk + 2) // 3 * (1 if nchunk + 2 >= 0 else -1)
    return nchunk, q * 3


def test_the_edges_the_table_was_chosen_for():
    by = sg.BY_ID
    # the two empty slabs of the H2 family, and none in the other two
    c = by["32x9x9-128-128-128"]
    ns, rows, empty, _ = sg.route(c, 2)["wgrad0"]
    assert (c.M, ns, rows, empty) == (2592, 10, 288, 1) and 9 * rows == c.M and _c_nchunk(9 * rows, min(c.M, 10 * rows)) == (0, 0)
    c = by["21x14x14-128-128-128"]
    ns, rows, empty, _ = sg.route(c, 2)["wgrad0"]
    assert (c.M, ns, rows, empty) == (4116, 16, 288, 1) and 15 * rows == 4320
    assert min(c.M, 16 * rows) - 15 * rows == -204 and _c_nchunk(15 * rows, min(c.M, 16 * rows)) == (-6, -3)
    for c in sg.CASES:
        for f in (1, 0):
            assert sg.route(c, f)["wgrad0"][2] == 0 and sg.route(c, f)["wgrad1"][2] == 0
    # two slabs with the cut inside the third image
    c = by["5x1x113-128-128-128"]
    assert sg.route(c, 2)["wgrad0"][:2] == (2, 288) and 288 // c.N == 2 and 288 % c.N != 0 and sg.route(c, 1)["wgrad0"][:2] == (2, 284)
    # both output-tile widths of the kernel gradients at N = 208 / 209 / 225
    for cid in ("2x13x16-128-256-384", "2x11x19-128-256-384", "1x15x15-128-256-384"):
        assert [sg.route(by[cid], f)[k][3] for f in (2, 1) for k in ("wgrad0", "wgrad1")] == [2, 1, 2, 1]
    # every tile height is run, and each above 16 rows with more than one row block per image and a ragged last tile
    seen = {}
    for c in sg.CASES:
        for f in (2, 1, 0):
            for name, _, _ in sg.launches(c):
                rt = sg.route(c, f)[name]
                if rt != "chain":
                    blocks = sg.row_blocks(c.N, rt)
                    seen.setdefault((f, rt), []).append((len(blocks), blocks[-1][1] % 16))
    for f in (2, 1, 0):
        assert {rt for (g, rt) in seen if g == f} == {1, 2, 4, 7, 13}
        for rt in (2, 4, 7, 13):
            assert any(n >= 2 and ragged == 1 for n, ragged in seen[(f, rt)]), (f, rt)
    assert sg.row_blocks(209, 13) == [(0, 112), (112, 97)] and sg.row_blocks(1024, 2)[-1] == (992, 32) and len(sg.row_blocks(1024, 2)) == 32
    # the chain: layer 0 and backward-data of every chain case, layer 1 unless Cout = 256; the row counts around the 64-row tile
    assert [c.M for c in sg.CHAIN] == [2, 63, 64, 65, 65, 75, 225, 418]
    for c in sg.CHAIN:
        r = sg.route(c, 2)
        assert r["fwd0"] == "chain" and r["bwd_data"] == "chain" and (r["fwd1"] == "chain") == (c.Cout == 512)
        assert "chain" not in sg.route(c, 1).values() and "chain" not in sg.route(c, 0).values()
    for c in sg.PER_IMAGE:
        assert "chain" not in sg.route(c, 2).values()
    c = by["3x5x5-256-512-512"]
    assert c.N < sg.CC_ROWS and sg.CC_ROWS // c.N == 2 and sg.CC_ROWS % c.N != 0          # row 64 lies inside the third image
    c = by["2x11x19-256-512-512"]
    assert c.M % sg.CC_ROWS == 34 and c.N // sg.CC_ROWS == 3 and c.N % sg.CC_ROWS != 0


def test_conv_splits_is_the_librarys(macx, L):
    """macx_stem_ws_floats = fixed-size segments + (ns0 9 Cin Cmid + ns1 9 Cmid Cout) slab floats: with conv_splits restated, what is
    left over is ONE constant (the absmax scratch) over the whole table and over a sweep of row counts around every break of the rule"""
    al4 = lambda n: (n + 3) & ~3
    wsize = lambda k, n: k * n * 3 // 2

    def rest(B, H, W, Ci, Cm, Co):
        N, npad, M = H * W, (H + 2) * (W + 2), B * H * W
        ns0, ns1 = sg.conv_splits(9 * Ci // 128 * (Cm // 128), M), sg.conv_splits(9 * Cm // 128 * (Co // 128), M)
        mine = al4(wsize(9 * Co, Cm)) + al4(B * N * Co) + al4(B * npad * Co) + al4(B * N * Cm) + al4(ns0 * 9 * Ci * Cm) + al4(ns1 * 9 * Cm * Co)
        got = L.macx_stem_ws_floats(C.byref(shapes(macx, B, H, W, Ci, Cm, Co)))
        assert got > 0
        return got - mine

    const = {rest(c.B, c.H, c.W, c.Cin, c.Cmid, c.Cout) for c in sg.CASES}
    for ch in ((128, 128, 128), (128, 256, 384), (256, 512, 512)):
        for B in list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257]:
            for H, W in ((1, 2), (3, 3), (7, 7), (9, 9), (14, 14), (8, 32), (32, 32)):
                const.add(rest(B, H, W, *ch))
    assert len(const) == 1 and 8 <= const.pop() < 1 << 16


def _c_function(path, name):
    """the text of an inline C++ function, comments and white space removed"""
    src = open(os.path.join(CSRC, path)).read()
    m = re.search(r"inline int %s\(.*?\n}\n" % name, src, re.S)
    assert m, name
    text = re.sub(r"//[^\n]*", "", m.group(0))
    return re.sub(r"\s+", "", text)


def test_the_restated_rules_are_the_sources():
    """rows_per_split and kb_gemm_pick_rt cannot be asked through the ABI: their C++ text, comments and white space aside, is what
    stem_geometry_cases.py restates.  Whoever edits a rule meets this test, restates it there and re-derives the table's routes."""
    assert _c_function("macx_api.hip", "rows_per_split") == \
        "inlineintrows_per_split(intM,intns){intr=(M+ns-1)/ns;returnh2_mode()?(r+31)&~31:(r+1)&~1;}"
    assert _c_function("macx_gemm.hip.h", "kb_gemm_pick_rt") == (
        "inlineintkb_gemm_pick_rt(intN,intB,intncb=4){staticconstintcand[5]={13,7,4,2,1};if(kb_gemm_force_rt())returnkb_gemm_force_rt();"
        "intk=0;if(N<=16)k=4;elseif(N<=32)k=3;elseif(N<=64)k=2;elseif(N<=112)k=1;"
        "autoblocks=[&](intrt){returnB*ncb*((N+rt*16-1)/(rt*16));};while(k<3&&blocks(cand[k])<200)++k;returncand[k];}")
    assert _c_function("macx_api.hip", "conv_splits") == (
        "inlineintconv_splits(inttiles,intM){intbest=1;doublebeff=0.0;for(intns=1;ns<=16;++ns){if((M+ns-1)/ns<256)break;"
        "constintblocks=tiles*ns;constdoubleeff=(double)blocks/(double)(((blocks+255)/256)*256);"
        "if(eff>beff+0.02){beff=eff;best=ns;}}returnbest;}")
    src = open(os.path.join(CSRC, "macx_gemm3h.hip.h")).read()
    assert "constexpr int CC_ROWS = 64, CC_NOUT = 512, CC_KC = 256" in src
    assert "conv_chain_mode() && p.conv_taps == 9 && p.Nout == CC_NOUT && p.conv_cin % CC_KC == 0" in src
    assert "constexpr int K_MAXN = %d;" % sg.K_MAXN in open(os.path.join(CSRC, "macx_small.hip.h")).read()


# ---- the inputs are fair --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c.id)
def test_fp32_oracle_stays_within_a_third_of_every_tolerance(macx, case):
    """per image / per tap normalisation must not be what fails a correct kernel: plain fp32 arithmetic on the same data, against the
    fp64 oracle under the same metrics, uses at most a third of each bound -- in both modes"""
    cfg, stem, img, dout = sg.make_case(macx, case)
    tol = sg.tolerances(case)
    for train in sg.MODES:
        r64 = sg.oracle(case, cfg, stem, img, dout, train, torch.float64)
        r32 = sg.oracle(case, cfg, stem, img, dout, train, torch.float32)
        e = sg.errors(case, r32, r64)
        print(sg.line(case, "fp32", train, e))
        for k in sg.METRICS:
            assert e[k] <= tol[k] / 3, (k, train, e[k], tol[k], e["where"])


def test_metrics_see_one_image_and_one_tap():
    """an error that one maximum over the tensor hides: a small image's error against ITS maximum, a weak tap's against ITS maximum,
    a non-zero where the reference is exactly zero"""
    ref = torch.ones(3, 4, 8, dtype=torch.float64)
    ref[1] *= 1e-3
    got = ref.clone()
    got[1, 2, 5] += 1e-6
    e, (b, n) = sg.per_image_err(got, ref)
    assert (b, n) == (1, 2) and abs(float(e[1]) - 1e-3) < 1e-9 and float(e[0]) == 0 and float(e[2]) == 0
    k = torch.ones(3, 3, 4, 4, dtype=torch.float64)
    k[0] = 0
    k[2, 1] *= 1e-2
    g = k.clone()
    g[2, 1, 0, 0] += 1e-5
    t = sg.per_tap_err(g, k)
    assert int(t.argmax()) == 7 and abs(float(t[7]) - 1e-3) < 1e-9 and float(t[:3].max()) == 0
    g[0, 1, 2, 2] = 1e-30
    assert float(sg.per_tap_err(g, k)[1]) == float("inf")


# ---- the magic division ----------------------------------------------------------------------------------------------------
def test_refusal_bound_lies_below_the_first_wrong_quotient():
    """for every N the stem admits: the first m at which (m magic) >> 32 != m // N is at or above the smallest row index stem_check
    refuses, and less than one image above it: the rule gives away nothing that matters"""
    for n in range(1, sg.K_MAXN + 1):
        e, wrong, bound = sg.magic_excess(n), sg.first_wrong_row(n), sg.refused_rows(n)
        assert 0 <= e < n
        if e == 0:
            assert wrong is None and bound is None and n & (n - 1) == 0
            continue
        assert bound <= wrong < bound + n, (n, wrong, bound)
        mg = sg.magic(n)
        assert (wrong * mg) >> 32 != wrong // n and ((wrong - 1) * mg) >> 32 == (wrong - 1) // n
        for m in (bound - 1, bound - n, bound // 2, n - 1, n, 0):          # exact below the bound
            assert m < 0 or (m * mg) >> 32 == m // n
    assert sg.first_wrong_row(1023) == 4215782 and sg.first_wrong_row(1000) == 6100999


def test_magic_w_is_exact_for_every_pixel():
    """yy = __umulhi(n, ceil(2^32 / W)) for the pixel n < N <= 1024 of an image W <= 1024 wide"""
    n = np.arange(sg.K_MAXN, dtype=np.uint64)
    for w in range(2, sg.K_MAXN + 1):
        mg = sg.magic(w)
        assert mg < 1 << 32                                    # (W = 1, which stem_check refuses, would not fit the 32-bit field)
        assert np.array_equal((n * np.uint64(mg)) >> np.uint64(32), n // np.uint64(w)), w


def _largest_batch(n, cmax=128):
    """(largest B the division rule serves, largest B the dropout's 32-bit element index serves) at b0 = 0"""
    r = sg.refused_rows(n)
    by_div = None if r is None else r // n                     # (B n - 1) e < 2^32  <=>  B n - 1 < r  <=>  B n <= r
    by_idx = ((1 << 32) - 1) // (n * cmax)
    return by_div, by_idx


@pytest.mark.parametrize("hw", [(31, 33), (25, 40), (14, 14), (16, 32)], ids=lambda hw: "N%d" % (hw[0] * hw[1]))
def test_stem_check_refuses_one_image_past_the_bound(macx, L, hw):
    """N = 1023 and 1000: the division's bound decides (about 4,100 and 6,100 images); N = 196: the element index of the dropout (2^32 /
    128 rows) is reached first, below the division's 39.8 M rows; N = 512: e = 0, the division never refuses"""
    H, W = hw
    n = H * W
    by_div, by_idx = _largest_batch(n)
    sizes = lambda B: (L.macx_stem_saved_floats(C.byref(shapes(macx, B, H, W))), L.macx_stem_ws_floats(C.byref(shapes(macx, B, H, W))))
    if n in (1023, 1000):
        assert by_div < by_idx and (by_div + 1) * n - 1 >= sg.refused_rows(n) > by_div * n - 1
        assert by_div * n - 1 < sg.first_wrong_row(n)
        ok = by_div
    else:
        assert by_div is None or by_div > by_idx
        ok = by_idx
    a, b = sizes(ok)
    assert a > 0 and b > 0
    assert sizes(ok + 1) == (0, 0)
    assert sizes(1) > (0, 0)


def test_a_shape_the_division_refuses_is_refused_like_any_other(macx, L):
    """1 x 1025 (N > K_MAXN) and 4200 images of 31 x 33: both sizes 0, MACX_EINVAL from the forward and the backward call before a
    pointer is looked at, and macx.Stem's ValueError from the autograd node before the device is asked for anything"""
    too_wide, too_many, fine = shapes(macx, 1, 1, 1025), shapes(macx, 4200, 31, 33), shapes(macx, 4100, 31, 33)
    assert L.macx_stem_saved_floats(C.byref(shapes(macx, 1, 1, 1024))) > 0 and L.macx_stem_saved_floats(C.byref(fine)) > 0
    P, G = macx._lib.MacxStemParams(), macx._lib.MacxStemGrads()
    EINVAL = -1
    for sh in (too_wide, too_many):
        assert L.macx_stem_saved_floats(C.byref(sh)) == 0 and L.macx_stem_ws_floats(C.byref(sh)) == 0
        assert L.macx_stem_forward_w(C.byref(sh), 0, 1.0, 0, C.byref(P), None, None, None, 0, None, None) == EINVAL
        assert L.macx_stem_backward_w(C.byref(sh), 0, 1.0, 0, C.byref(P), None, None, 0, None, 0, None, C.byref(G), None, None) == EINVAL
    cfg = sg.mo.flag_file_config("args", memDim=128, ctrlDim=128, attDim=128)
    cfg.stemDim = 128
    for H, W, B in ((1, 1025, 1), (31, 33, 4200)):
        stem = macx.Stem(cfg, H=H, W=W, inDim=128, generator=torch.Generator().manual_seed(1))
        sh = shapes(macx, B, H, W)
        with pytest.raises(ValueError, match="stem"):
            stem._call(sh, (stem.act, 1.0), 0, False, None, torch.zeros(4))
