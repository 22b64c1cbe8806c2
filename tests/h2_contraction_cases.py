"""Tables, data, reference, restatement and bounds for the H2 row contractions on their own: macx_h2_wgrad (wgrad_h2_kernel and
its factor-table kernel) and macx_h2_sb (sb_h2_kernel, sb_h2w_kernel), mac-network_amd/csrc/macx_wgrad_h2.hip.h.
Used by tests/test_h2_contractions_host.py (CPU) and tests/test_gpu_h2_contractions.py (-m gpu).

WHAT THE KERNELS COMPUTE.  An operand row lives as two fp16 planes hi, lo and one exponent e per 128 columns: the stored value is
x' = (hi + lo) 2^-e (h2_split / h2_join below restate macx_h2_from_f32 / macx_h2_to_f32 bit for bit; the GPU file checks that).
A contraction over rows brings the rows of an operand family to the family's smallest exponent E per 128-column block through
ONE fp16 factor per (row m, block of A, block of G),  f_m = fp16(2^k_m),  k_m = (EA - ea_m) + (EG - eg_m) <= 0,  zero for
k_m < -24 (pk_pow2_f16), multiplied into both G planes with fp16 rounding:  gh' = fp16(gh f), gl' = fp16(gl f).  The accumulator
then receives, in fp32,  al gh' + ah gl' + ah gh'  per row, and leaves as  acc 2^-(EA + EG).  In exact arithmetic, with
exact factors 2^k_m, the three terms plus the dropped al gl sum to  sum_m a'_m g'_m: the fp64 product of the round-tripped
operands is the REFERENCE, and conversion error is out of the comparison.

THE BOUND, per element, in the output's unit U = 2^-(EA + EG) (`core` below computes the pieces per block pair in fp64):
  (1) fp32 accumulation.  Every fp16 x fp16 product is exact in fp32 (22 bits).  A sum of n fp32 terms taken in ANY order or tree
      is off by at most (n - 1) 2^-24 sum |terms| (to first order; the matrix pipe is assumed no worse than a chain of fp32
      adds).  n is counted, not fitted: 3 terms per live row of the longest split (3 L), one add per slab of the fixed-order
      slab sum (nsplit), one for the |gh'| <= (1 + 2^-10) |gh f| slack of the rounded planes, one spare:
          k 2^-24 S,   k = 3 L + nsplit + 2,   S = sum_m (|ah| + |al|)(|gh| + |gl|) f_m .
      The dropped term is bounded by ITSELF, from the planes:   D = sum_m |al| |gl| f_m   (<= 2^-22 of S, typically 2^-26).
  (2) the fp16 factor.  gh f is exact (a power of two) unless it lands below fp16's normal range: a non-zero |gh f| < 2^-14 is
      rounded at half the subnormal spacing, 2^-25, and so is gl f; a row with k_m < -24 is dropped whole and loses
      |gh + gl| 2^k_m.  Absolute in the unit U:
          Q = sum_m (|ah| + |al|) q_m,   q_m = 2^-25 [0 < |gh f| < 2^-14] + 2^-25 [0 < |gl f| < 2^-14]   or   |gh + gl| 2^k_m .
      The exponents follow from the data (h2_exponent: 141 - biased exponent of the block maximum, zero block -> H2_E_MAX = 90,
      clamped to [-113, 90]) and the minima from the exponents, so the test computes Q itself.
  wgrad:   |out - ref| <= (k 2^-24 S + D + Q) U                                 (one unit per block pair: E over ALL rows)
  sb_h2 (narrow), per question b with its OWN minima (a stage never crosses a question; unit U_b), N rows, then the folds
      dW1b += S_b,  dW1a += y_b S_b (one fma),  over the qpg questions x nsteps steps of a group and the ngroup slabs:
          e_b = (3 N + 1) 2^-24 S_b^abs + D_b + Q_b                            (error of S_b itself)
          |dW1b - ref| <= sum_b [e_b + (Qn + 2) 2^-24 S_b^abs],   |dW1a - ref| <= sum_b |y_bk| [e_b + (Qn + 2) 2^-24 S_b^abs],
          Qn = qpg nsteps + ngroup;
      dy[b][k] = sum_j W1a[k][j] S_b[k][j]: two fmas per lane, four shuffle adds, the test adds the 4 d / 128 partials in fp64:
          |dy - ref| <= sum_j |W1a_kj| [e_b + 7 2^-24 S_b^abs] .
  (3) sb_h2w (wide): ONE running accumulator T_k = S_1 + .. + S_k over the K = (questions of the group) x nsteps questions in
      processing order -- steps outer, the group's questions inner; both forms of the kernel walk stage g = (step, question,
      chunk) in that order (issue_g / the step loop) -- moved between the questions' units by exact powers of two, and
      dW1b = T_K, dW1a = sum_k (y_k - y_{k+1}) T_k (y_{K+1} = 0).  Every add into T rounds against the RUNNING sum, so
          err(T_k) <= 3 N k 2^-24 Tabs_k + C_k,    Tabs_k = sum_{i <= k} S_i^abs,  C_k = sum_{i <= k} (D_i + Q_i),
      and a fold (y_k - y_{k+1}: one rounding; the fma: one; K + ngroup adds into dW1a) gives
          |dW1a - ref| <= sum_k (|y_k| + |y_{k+1}|) [(3 N k + K + ngroup + 3) 2^-24 Tabs_k + C_k]
          |dW1b - ref| <= (3 N K + ngroup + 1) 2^-24 Tabs_K + C_K                                   summed over the groups.
      The two 128-column blocks of dI1 in a 128 x 256 tile share ONE minimum (the smaller of the two).
A question whose unit 2^-(EX + EG) underflows fp32 (EX + EG >= 150: every value of both operands below 2^-45 of a normal fp32's
range -- in practice an all-zero question) adds nothing in either kernel.
An element with S = 0 (an all-zero column, an all-zero question) has bound 0: only exact zero passes.

DATA (seeded; family per case):  a: N(0,1) against N(0,1) 1e-6;  b: a with every row scaled by 2^U(-20, 0);  c: every (row,
128-column block) scaled by its own 2^U(-12, 0) and the blocks of A by 2^8, 2^-8, .. and of G by 2^-6, 2^6, ..: the (A block,
G block) factor tables all differ;  d: b with a zero row in A, another in G, the last N / 3 rows of one question (tensor) zero in
both, one all-zero question (where there are two) and one all-zero column each.  Family e -- every H2 buffer pre-filled with
0xFF bytes -- is applied to EVERY case by the GPU file.
"""
from collections import namedtuple

import numpy as np

# Each case runs on the FIRST seed on which the restatement stays within half of every bound (the host file asserts that it does).
# D and the loss of a dropped row are not rounding errors but what the arithmetic leaves out by design, the same in the kernel and
# in the restatement: on an element whose live rows all but cancel they are the whole bound, and such a draw says nothing about
# rounding.  Seed 0 wherever no entry stands here.
FIRST_FAIR_SEED = {"128x128-nt1-R32-ns1-d": 1, "128x128-nt1-R64-ns1-d": 1, "256x128-nt1-R33-ns1-b": 13, "256x256-nt1-R64-ns3-b": 10,
                   "wide-d256-B1-N1-q1-p1-b": 1}
U24 = 2.0 ** -24
H2_E_MIN, H2_E_MAX, H2_PAD_ROWS = -113, 90, 64
SBH_MAXROWS, SBH_MAXQ, SBW_MAXROWS, SBW_MAXQ = 4096, 32, 1024, 4
FAMILIES = "abcd"


# ---- the format --------------------------------------------------------------------------------------------------------------
def h2_floats(rows, cols):
    rp = rows + H2_PAD_ROWS
    return ((2 * (cols // 8) * rp * 16 + rp * (cols // 128) + 15) & ~15) // 4


def h2_split(x):
    """fp32 [rows, C] -> (hi, lo) fp16 [rows, C], e int [rows, C / 128]: h2_from_f32_kernel (h2_exponent, h2_split8)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, C = x.shape
    xb = x.reshape(rows, C // 128, 128)
    mx = np.abs(xb).max(axis=2)
    be = ((mx.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    e = np.where(mx == 0, H2_E_MAX, np.clip(141 - be, H2_E_MIN, H2_E_MAX))
    xs = np.ldexp(xb, e[:, :, None]).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi.reshape(rows, C), lo.reshape(rows, C), e


def h2_join(hi, lo, e):
    """(hi + lo) 2^-e in fp32: h2_to_f32_kernel"""
    rows, C = hi.shape
    s = (hi.astype(np.float32) + lo.astype(np.float32)).reshape(rows, C // 128, 128)
    return np.ldexp(s, -e[:, :, None]).astype(np.float32).reshape(rows, C)


def pow2_f16(k):
    """pk_pow2_f16: 2^k as fp16 for k <= 0, 0 below 2^-24 (k < -30 by the test, -30 .. -25 by the conversion)"""
    k = np.asarray(k)
    return np.where(k < -24, 0.0, np.ldexp(1.0, np.maximum(k, -40))).astype(np.float16)


# ---- the pieces of the bound for one (block of A, block of G) ------------------------------------------------------------------
Core = namedtuple("Core", "S D Q")           # [128, 128] fp64 each, in the unit 2^-(EA + EG)


def core(ah, al, ea, gh, gl, eg, EA, EG):
    """planes fp16 [rows, 128], ea / eg int [rows]: S, D, Q of the docstring"""
    k = (EA - ea) + (EG - eg)
    f = pow2_f16(k).astype(np.float64)[:, None]
    aabs = np.abs(ah.astype(np.float64)) + np.abs(al.astype(np.float64))
    ghf, glf = np.abs(gh.astype(np.float64)) * f, np.abs(gl.astype(np.float64)) * f
    S = aabs.T @ (ghf + glf)
    D = np.abs(al.astype(np.float64)).T @ glf
    q = U24 / 2 * ((ghf > 0) & (ghf < 2.0 ** -14)) + U24 / 2 * ((glf > 0) & (glf < 2.0 ** -14))
    lost = np.abs(gh.astype(np.float64) + gl.astype(np.float64)) * np.ldexp(1.0, np.maximum(k, -400))[:, None]
    q = np.where(f == 0, lost, q)
    return Core(S, D, aabs.T @ q)


def emin(e):
    """h2_emin_final / the per-question minima: the smallest exponent of the rows, at most 126"""
    return np.minimum(e.min(axis=0), 126)


# ================================================= macx_h2_wgrad ==============================================================
WCase = namedtuple("WCase", "id Kd Jd nt R a_shared nsplit fam seed")


def _w(Kd, Jd, nt, R, nsplit=1, a_shared=0, fam="b", seed=0):
    cid = "%dx%d-nt%d-R%d%s-ns%d-%s" % (Kd, Jd, nt, R, "-shared" if a_shared else "", nsplit, fam)
    return WCase(cid, Kd, Jd, nt, R, a_shared, nsplit, fam, FIRST_FAIR_SEED.get(cid, seed))


ROWS_PER_SPLIT = (1, 31, 32, 33, 63, 64, 65, 96, 97, 129, 161)
SHAPES = ((128, 128), (256, 128), (128, 256), (256, 256), (384, 384), (512, 256), (256, 512))
WGRAD_CASES = (
    # every tile shape, on 4 stages with a last stage of one row; c where there are two blocks on a side
    [_w(Kd, Jd, 1, 97, fam="c" if max(Kd, Jd) >= 256 else "b") for Kd, Jd in SHAPES]
    # rows per split: 1 - 6 stages against the rings of 4, 3 and 2
    + [_w(128, 128, 1, r, fam="abd"[i % 3]) for i, r in enumerate(ROWS_PER_SPLIT) if r != 97]
    + [_w(256, 128, 1, r, fam="b") for r in (33, 65, 129)]
    + [_w(256, 256, 1, r, fam="c") for r in (1, 33, 65, 161)]
    # tensors: a stage inside one tensor (R = 32) and straddling two (R = 49), A per tensor and shared
    + [_w(Kd, Kd, 3, R, a_shared=s, fam=fam) for Kd in (128, 256) for R, s, fam in ((32, 0, "b"), (49, 0, "d"), (49, 1, "b"), (32, 1, "a"))]
    # splits: ragged last split, an empty one (M = 64, nsplit = 3: the third starts at M)
    + [_w(128, 128, 1, 161, nsplit=2, fam="b"), _w(128, 128, 1, 161, nsplit=3, fam="d"), _w(256, 256, 1, 161, nsplit=3, fam="c"),
       _w(128, 128, 1, 64, nsplit=3, fam="a"), _w(256, 256, 1, 64, nsplit=3, fam="b"), _w(256, 128, 3, 49, nsplit=2, fam="b"),
       _w(384, 384, 3, 49, nsplit=2, a_shared=1, fam="c")])
WGRAD_BY_ID = {c.id: c for c in WGRAD_CASES}
assert len(WGRAD_BY_ID) == len(WGRAD_CASES)


# ---- the launch rules, restated (held to the C++ text by the host file) ----------------------------------------------------------
def wgrad_h2_kw(Kd):
    return 2 if Kd % 256 == 0 else 1


wgrad_h2_jw = wgrad_h2_kw


def wgrad_h2_tiles(Kd, Jd):
    return (Kd // (wgrad_h2_kw(Kd) * 128)) * (Jd // (wgrad_h2_jw(Jd) * 128))


def wh_ring(kw, jw):
    return 2 if kw + jw == 4 else (3 if kw + jw == 3 else 4)


def wgrad_h2_mpad(M):
    return (M + 63) & ~31


def rows_per_split(M, ns):
    return ((M + ns - 1) // ns + 31) & ~31


def wgrad_big_splits(M, Kd, Jd):
    ns = min(256 // wgrad_h2_tiles(Kd, Jd), (M + 255) // 256)
    return max(ns, 1)


def cell_splits(M, d, pipe=3):
    """CellBwd::read_weight_contractions: the splits of the dW2 / dWx contractions (mode 3 halves them on 256 x 256 tiles)"""
    ns = wgrad_big_splits(M, d, d)
    return ns // 2 if (pipe >= 3 and wgrad_h2_kw(d) == 2 and ns >= 2) else ns


def split_rows(M, ns):
    """[(m_begin, m_end)] per split; an empty split has m_end <= m_begin"""
    r = rows_per_split(M, ns)
    return [(s * r, min(M, s * r + r)) for s in range(ns)]


def sb_qpg(B, N):
    qpg = max((B + 15) // 16, 1)
    cap = SBH_MAXROWS // (((N + 31) // 32) * 32)
    if qpg > cap:
        qpg = max(cap, 1)
    return min(qpg, SBH_MAXQ)


def sb_h2_wide_qpg(B, N, d):
    groups = max(256 // ((d // 128) * (d // 256)), 1)
    qpg = (B + groups - 1) // groups
    cap = min(SBW_MAXQ, (SBW_MAXROWS // 2) // (((N + 31) // 32) * 32))
    return max(min(qpg, cap), 1)


def sb_cont(nsteps, N, qpg, sb_cont_mode=1):
    """sb_h2w_launch: the continuous stage stream runs when ..."""
    nchunk = (N + 31) >> 5
    return bool(sb_cont_mode) and nsteps > 1 and nchunk >= 3 and qpg * nchunk * 32 <= 512


# ---- data --------------------------------------------------------------------------------------------------------------------
def _rows(rng, rows, cols, fam, scale, sign):
    """one operand [rows, cols] of family a / b / c (d starts from b); sign: +1 for the A side's block scales, -1 for G's"""
    x = rng.standard_normal((rows, cols)).astype(np.float32) * np.float32(scale)
    if fam in "bd":
        x *= np.exp2(rng.uniform(-20, 0, (rows, 1))).astype(np.float32)
    if fam == "c":
        blk = np.exp2(rng.uniform(-12, 0, (rows, cols // 128)))
        blk *= np.exp2(sign * (8.0 if sign > 0 else 6.0) * (-1.0) ** np.arange(cols // 128))[None, :]
        x *= np.repeat(blk, 128, axis=1).astype(np.float32)
    return x


def wgrad_data(c):
    """A [nt or 1][R][Kd], G [nt][R][Jd] fp32"""
    rng = np.random.RandomState(1000 + c.seed + 7 * c.Kd + 3 * c.Jd + 31 * c.nt * c.R + c.nsplit)
    nta = 1 if c.a_shared else c.nt
    A = _rows(rng, nta * c.R, c.Kd, c.fam, 1.0, +1).reshape(nta, c.R, c.Kd)
    G = _rows(rng, c.nt * c.R, c.Jd, c.fam, 1e-6, -1).reshape(c.nt, c.R, c.Jd)
    if c.fam == "d":
        A[0, c.R // 2] = 0
        G[-1, c.R // 3] = 0
        if c.R >= 3:
            A[0, c.R - c.R // 3:] = 0
            G[0, c.R - c.R // 3:] = 0
        if c.nt >= 2 and not c.a_shared:
            A[1] = 0
            G[1] = 0
        A[:, :, 5] = 0
        G[:, :, 7] = 0
    return A, G


WOps = namedtuple("WOps", "ah al ea gh gl eg A1 G1")     # planes / exponents over all M reduction rows; A1, G1: the round trip


def wgrad_operands(c, A, G):
    """what the kernel multiplies, row m of the reduction = row m % R of tensor m // R (A shared: of the one tensor)"""
    M = c.nt * c.R
    ah, al, ea = h2_split(A.reshape(-1, c.Kd))
    gh, gl, eg = h2_split(G.reshape(-1, c.Jd))
    if c.a_shared:
        idx = np.arange(M) % c.R
        ah, al, ea = ah[idx], al[idx], ea[idx]
    return WOps(ah, al, ea, gh, gl, eg, h2_join(ah, al, ea), h2_join(gh, gl, eg))


def wgrad_reference(o):
    return o.A1.astype(np.float64).T @ o.G1.astype(np.float64)


def _blocks(n):
    return [slice(128 * i, 128 * i + 128) for i in range(n // 128)]


def wgrad_bound(c, o):
    """(bound, part 2 of it) [Kd, Jd] fp64"""
    M = c.nt * c.R
    L = max(max(e - b for b, e in split_rows(M, c.nsplit)), 0)
    k = 3 * L + c.nsplit + 2
    EA, EG = emin(o.ea), emin(o.eg)
    bound, part2 = np.zeros((c.Kd, c.Jd)), np.zeros((c.Kd, c.Jd))
    for kb, ks in enumerate(_blocks(c.Kd)):
        for jb, js in enumerate(_blocks(c.Jd)):
            p = core(o.ah[:, ks], o.al[:, ks], o.ea[:, kb], o.gh[:, js], o.gl[:, js], o.eg[:, jb], EA[kb], EG[jb])
            unit = np.ldexp(1.0, -int(EA[kb] + EG[jb]))
            bound[ks, js] = (k * U24 * p.S + p.D + p.Q) * unit
            part2[ks, js] = p.Q * unit
    return bound, part2


def _terms(ah, al, ghs, gls):
    """the three products of a set of rows, fp32 accumulation in the BLAS's order (not the kernel's)"""
    ah, al, ghs, gls = (t.astype(np.float32) for t in (ah, al, ghs, gls))
    return (al.T @ ghs + ah.T @ gls) + ah.T @ ghs


def _scaled(gh, gl, f):
    """both G planes times the fp16 row factors, fp16 rounding"""
    return gh * f[:, None], gl * f[:, None]


def _largest_row(esum, b, e):
    """the row of [b, e) with the smallest exponent sum (block 0 of both operands): the largest one of a last stage"""
    return b + int(np.argmin(esum[b:e]))


def last_stage_weight(esum, n):
    """log2 of the factor of the largest row of the last stage of n rows (0: it is among the largest rows of all)"""
    return int(esum[:n].min() - esum[(n - 1) & ~31:n].min())


def wgrad_restate(c, o, defect=None):
    """numpy restatement of factors kernel + contraction + slab sum, fp32.  defect: None | 'factor_next_row' | 'block_swap' |
    'row_past_end' (row M, the re-read last row, with factor 1) | 'row_dropped' (the largest row of the last stage) | 'slab_left_out'"""
    M = c.nt * c.R
    EA, EG = emin(o.ea), emin(o.eg)
    out = np.zeros((c.Kd, c.Jd), np.float32)
    splits = split_rows(M, c.nsplit)
    for kb, ks in enumerate(_blocks(c.Kd)):
        for jb, js in enumerate(_blocks(c.Jd)):
            kk, jj = (jb, kb) if defect == "block_swap" else (kb, jb)
            f = pow2_f16((EA[kk] - o.ea[:, kk]) + (EG[jj] - o.eg[:, jj]))
            if defect == "factor_next_row":
                f = np.roll(f, -1)
            ghs, gls = _scaled(o.gh[:, js], o.gl[:, js], f)
            ah, al = o.ah[:, ks], o.al[:, ks]
            if defect == "row_past_end":                    # row M: the clamped re-read of the last row, its factor 1 instead of 0
                ghs, gls = np.vstack([ghs, o.gh[-1:, js]]), np.vstack([gls, o.gl[-1:, js]])
                ah, al = np.vstack([ah, ah[-1:]]), np.vstack([al, al[-1:]])
            unit = np.float32(np.ldexp(1.0, -int(EA[kb]))) * np.float32(np.ldexp(1.0, -int(EG[jb])))
            acc = np.zeros((128, 128), np.float32)
            for s, (b, e) in enumerate(splits):
                if e <= b or (defect == "slab_left_out" and s == 0):
                    continue
                rows = np.arange(b, e)
                if defect == "row_dropped" and e == M:
                    rows = np.delete(rows, _largest_row(o.ea[:, 0] + o.eg[:, 0], b + ((e - b - 1) & ~31), e) - b)
                if defect == "row_past_end" and e == M:
                    rows = np.append(rows, M)
                part = _terms(ah[rows], al[rows], ghs[rows], gls[rows]) * unit
                acc = acc + part
            out[ks, js] = acc
    return out


# ================================================= macx_h2_sb =================================================================
SCase = namedtuple("SCase", "id wide d B N qpg nsteps dy cont fam seed")


def _s(wide, d, B, N, qpg, nsteps=1, dy=0, cont=1, fam="b", seed=0):
    cid = "%s-d%d-B%d-N%d-q%d-p%d%s%s-%s" % ("wide" if wide else "narrow", d, B, N, qpg, nsteps, "-dy" if dy else "", "" if cont else "-cont0", fam)
    return SCase(cid, wide, d, B, N, qpg, nsteps, dy, cont, fam, FIRST_FAIR_SEED.get(cid, seed))


SB_N = (1, 31, 32, 33, 64, 65, 129)
NARROW_CASES = (
    [_s(0, 128, B, N, q, dy=1, fam="bd"[i % 2]) for i, (N, (B, q)) in enumerate(zip(SB_N, ((1, 1), (4, 2), (5, 2), (5, 3), (4, 2), (5, 2), (5, 3))))]
    + [_s(0, 128, 5, N, 2, nsteps=p, fam="db"[i % 2]) for i, (N, p) in enumerate(((1, 3), (33, 3), (65, 1), (129, 3), (32, 1)))]
    + [_s(0, 256, 5, 33, 2, dy=1, fam="d"), _s(0, 256, 4, 65, 2, nsteps=3, fam="b"), _s(0, 384, 5, 33, 3, dy=1, fam="b"),
       _s(0, 384, 4, 31, 2, nsteps=3, fam="d"), _s(0, 128, 5, 129, 3, dy=1, fam="a"), _s(0, 256, 1, 64, 1, fam="c")])
WIDE_CASES = (
    # the per-step form: one step; three steps with fewer than three stages; three steps with the stream switched off
    [_s(1, 256, 5, 65, 2, fam="d"), _s(1, 512, 4, 33, 4, fam="b"), _s(1, 256, 1, 1, 1, fam="b"), _s(1, 256, 5, 33, 2, nsteps=3, fam="d"),
     _s(1, 512, 6, 33, 4, nsteps=3, fam="b"), _s(1, 256, 5, 97, 2, nsteps=3, cont=0, fam="d"), _s(1, 512, 4, 97, 4, nsteps=3, cont=0, fam="b")]
    # the continuous stream
    + [_s(1, 256, 5, 65, 2, nsteps=2, fam="d"), _s(1, 256, 4, 65, 4, nsteps=3, fam="b"), _s(1, 512, 6, 65, 4, nsteps=5, fam="d"),
       _s(1, 256, 1, 96, 1, nsteps=3, fam="b"), _s(1, 512, 5, 96, 2, nsteps=2, fam="c"), _s(1, 256, 5, 97, 2, nsteps=3, fam="d"),
       _s(1, 512, 4, 97, 4, nsteps=3, fam="b"), _s(1, 256, 6, 97, 4, nsteps=5, fam="a"), _s(1, 256, 5, 129, 3, nsteps=2, fam="d"),
       _s(1, 512, 4, 129, 3, nsteps=3, fam="b"), _s(1, 256, 1, 512, 1, nsteps=2, fam="b")])
BOTH_CASES = [c for c in WIDE_CASES if c.id in ("wide-d256-B5-N65-q2-p1-d", "wide-d256-B5-N97-q2-p3-d", "wide-d512-B4-N33-q4-p1-b")]
SB_BY_ID = {c.id: c for c in NARROW_CASES + WIDE_CASES}
assert len(SB_BY_ID) == len(NARROW_CASES) + len(WIDE_CASES) and len(BOTH_CASES) == 3


def sb_data(c):
    """X, dI1 [nsteps][B][N][d], y [nsteps][B][d], W1a [d][d] fp32"""
    rng = np.random.RandomState(5000 + c.seed + c.d + 17 * c.B + 131 * c.N + 7 * c.nsteps + c.wide)
    n = c.nsteps * c.B * c.N
    X = _rows(rng, n, c.d, c.fam, 1.0, +1).reshape(c.nsteps, c.B, c.N, c.d)
    G = _rows(rng, n, c.d, c.fam, 1e-6, -1).reshape(c.nsteps, c.B, c.N, c.d)
    y = rng.standard_normal((c.nsteps, c.B, c.d)).astype(np.float32)
    if c.B >= 2:
        y[0, 1] = y[0, 0]                       # adjacent questions with equal y: a fold coefficient of exactly 0
    W = (rng.standard_normal((c.d, c.d)) / c.d ** 0.5).astype(np.float32)
    if c.fam == "d":
        X[0, 0, c.N // 2] = 0
        G[-1, -1, c.N // 3] = 0
        if c.N >= 3:
            X[0, 0, c.N - c.N // 3:] = 0
            G[0, 0, c.N - c.N // 3:] = 0
        if c.B >= 2:
            X[-1, 1] = 0
            G[-1, 1] = 0
        X[..., 5] = 0
        G[..., 7] = 0
    return X, G, y, W


SOps = namedtuple("SOps", "xh xl ex gh gl eg X1 G1")      # [nsteps][B][N][..]


def sb_operands(c, X, G):
    xh, xl, ex = h2_split(X.reshape(-1, c.d))
    gh, gl, eg = h2_split(G.reshape(-1, c.d))
    sh, se = (c.nsteps, c.B, c.N, c.d), (c.nsteps, c.B, c.N, c.d // 128)
    return SOps(xh.reshape(sh), xl.reshape(sh), ex.reshape(se), gh.reshape(sh), gl.reshape(sh), eg.reshape(se),
                h2_join(xh, xl, ex).reshape(sh), h2_join(gh, gl, eg).reshape(sh))


def sb_reference(c, o, y, W):
    """dW1a, dW1b [d][d], dy [nsteps][B][d] in fp64"""
    S = np.einsum("sbnk,sbnj->sbkj", o.X1.astype(np.float64), o.G1.astype(np.float64))
    return (np.einsum("sbk,sbkj->kj", y.astype(np.float64), S), S.sum(axis=(0, 1)), np.einsum("kj,sbkj->sbk", W.astype(np.float64), S))


def sb_groups(c):
    """per group the questions in processing order: [(step, b)], steps outer"""
    return [[(s, b) for s in range(c.nsteps) for b in range(g, min(c.B, g + c.qpg))] for g in range(0, c.B, c.qpg)]


def sb_units(c, o, s, b):
    """(EX [d / 128], EG per column block as the kernel in use takes it) of question (s, b)"""
    EX, EG = emin(o.ex[s, b]), emin(o.eg[s, b])
    if c.wide:
        EG = np.repeat(np.minimum(EG[0::2], EG[1::2]), 2)
    return EX, EG


def dead(EX, EG):
    return int(EX) + int(EG) >= 150


def _sb_core(c, o, s, b, only_q=False):
    """S^abs and D + Q of question (s, b) in real units, [d, d]; only_q: 0 and Q alone (part 2's share of a bound)"""
    EX, EG = sb_units(c, o, s, b)
    Sa, C = np.zeros((c.d, c.d)), np.zeros((c.d, c.d))
    for kb, ks in enumerate(_blocks(c.d)):
        for jb, js in enumerate(_blocks(c.d)):
            if dead(EX[kb], EG[jb]):
                continue
            p = core(o.xh[s, b][:, ks], o.xl[s, b][:, ks], o.ex[s, b][:, kb], o.gh[s, b][:, js], o.gl[s, b][:, js], o.eg[s, b][:, jb],
                     EX[kb], EG[jb])
            unit = np.ldexp(1.0, -int(EX[kb] + EG[jb]))
            Sa[ks, js], C[ks, js] = (0.0, p.Q * unit) if only_q else (p.S * unit, (p.D + p.Q) * unit)
    return Sa, C


def sb_bound(c, o, y, W, only_q=False):
    """bounds of dW1a, dW1b [d][d] and dy [nsteps][B][d] (dy: narrow only); only_q: what part (2) contributes to each"""
    groups = sb_groups(c)
    ng, N = len(groups), c.N
    ya = np.abs(y.astype(np.float64))
    bA, bB, bY = np.zeros((c.d, c.d)), np.zeros((c.d, c.d)), np.zeros((c.nsteps, c.B, c.d))
    for grp in groups:
        if not c.wide:
            Qn = c.qpg * c.nsteps + ng
            for s, b in grp:
                Sa, C = _sb_core(c, o, s, b, only_q)
                e = (3 * N + 1) * U24 * Sa + C
                bB += e + (Qn + 2) * U24 * Sa
                bA += ya[s, b][:, None] * (e + (Qn + 2) * U24 * Sa)
                bY[s, b] = (np.abs(W.astype(np.float64)) * (e + 7 * U24 * Sa)).sum(axis=1)
        else:
            K = len(grp)
            Tabs, Cc = np.zeros((c.d, c.d)), np.zeros((c.d, c.d))
            for k, (s, b) in enumerate(grp, 1):
                Sa, C = _sb_core(c, o, s, b, only_q)
                Tabs, Cc = Tabs + Sa, Cc + C
                yn = ya[grp[k][0], grp[k][1]] if k < K else 0.0
                bA += (ya[s, b] + yn)[:, None] * ((3 * N * k + K + ng + 3) * U24 * Tabs + Cc)
            bB += (3 * N * K + ng + 1) * U24 * Tabs + Cc
    return bA, bB, bY


def sb_restate(c, o, y, W, defect=None):
    """numpy restatement in fp32 of the kernel the case names (narrow: per-question fold; wide: summation by parts).  defect: None |
    'row_past_end' (the row past a question's end, the re-read last row, with factor 1) | 'row_dropped' (the largest row of
    a question's last stage) | 'prev_question_min' (the
    rows of a question brought to the minima of the question before) | wide only: 'fold_yk' (y_k in place of y_k - y_{k+1}) |
    'step_left_out' (T restarts at every step)"""
    d, f32 = c.d, np.float32
    dA, dB = np.zeros((d, d), f32), np.zeros((d, d), f32)
    dy = np.zeros((c.nsteps, c.B, d), f32)
    yf = y.astype(f32)
    for grp in sb_groups(c):
        accA, accT = np.zeros((d, d), f32), np.zeros((d, d), f32)       # accT: the narrow kernel's accB / the wide kernel's T
        eT = np.zeros((d // 128, d // 128), np.int64)                   # wide: the unit exponent T is held in, per block pair
        yprev, first = None, True
        for i, (s, b) in enumerate(grp):
            EX, EG = sb_units(c, o, s, b)
            if defect == "prev_question_min" and i > 0:
                EXf, EGf = sb_units(c, o, *grp[i - 1])
            else:
                EXf, EGf = EX, EG
            rows = np.arange(c.N)
            if defect == "row_dropped":
                rows = np.delete(rows, _largest_row(o.ex[s, b][:, 0] + o.eg[s, b][:, 0], (c.N - 1) & ~31, c.N))
            if defect == "row_past_end" and c.N % 32:
                rows = np.append(rows, c.N)                 # row N: the re-read last row, its factor 1 instead of 0
            S = np.zeros((d, d), f32)                                   # S_b in the question's units, per block pair
            E = np.zeros((d // 128, d // 128), np.int64)
            live = np.zeros((d // 128, d // 128), bool)
            for kb, ks in enumerate(_blocks(d)):
                for jb, js in enumerate(_blocks(d)):
                    E[kb, jb] = int(EX[kb] + EG[jb])
                    live[kb, jb] = not dead(EX[kb], EG[jb])
                    if not live[kb, jb]:
                        continue
                    f = pow2_f16(np.minimum((EXf[kb] - o.ex[s, b][:, kb]) + (EGf[jb] - o.eg[s, b][:, jb]), 0))
                    ghs, gls = _scaled(o.gh[s, b][:, js], o.gl[s, b][:, js], f)
                    xh, xl = o.xh[s, b][:, ks], o.xl[s, b][:, ks]
                    if defect == "row_past_end":
                        ghs, gls = np.vstack([ghs, o.gh[s, b][-1:, js]]), np.vstack([gls, o.gl[s, b][-1:, js]])
                        xh, xl = np.vstack([xh, xh[-1:]]), np.vstack([xl, xl[-1:]])
                    S[ks, js] = _terms(xh[rows], xl[rows], ghs[rows], gls[rows])
            unit = np.repeat(np.repeat(np.exp2(-E.astype(np.float64)), 128, 0), 128, 1)
            if not c.wide:
                sv = (S * unit.astype(f32)).astype(f32)
                accT = accT + sv
                accA = accA + yf[s, b][:, None] * sv
                dy[s, b] = (W.astype(f32) * sv).sum(axis=1, dtype=f32)
                continue
            # wide: the fold of the question before runs when this one starts; a dead question keeps the unit T is in
            E = np.where(live, E, eT) if not first else E
            if not first:
                if defect == "step_left_out" and s != grp[i - 1][0]:
                    accT = np.zeros((d, d), f32)
                coef = yprev if defect == "fold_yk" else (yprev - yf[s, b]).astype(f32)
                uT = np.repeat(np.repeat(np.exp2(-eT.astype(np.float64)), 128, 0), 128, 1).astype(f32)
                accA = accA + (coef[:, None] * uT).astype(f32) * accT
                mv = np.repeat(np.repeat(np.exp2(np.clip(E - eT, -126, 126).astype(np.float64)), 128, 0), 128, 1).astype(f32)
                accT = (accT * mv).astype(f32)
            eT, yprev, first = E, yf[s, b], False
            accT = accT + S
        if c.wide:
            uT = np.repeat(np.repeat(np.exp2(-eT.astype(np.float64)), 128, 0), 128, 1).astype(f32)
            accA = accA + (yprev[:, None] * uT).astype(f32) * accT
            accT = (accT * uT).astype(f32)
        dA, dB = dA + accA, dB + accT
    return dA, dB, dy


def ratio(err, bound):
    """err / bound elementwise; 0 / 0 = 0, x / 0 = inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
