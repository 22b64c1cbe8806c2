"""-m gpu: the kernels AROUND the cell past their first block and first pass -- what bench.py's model-level number and
CapturedTowerTrainStep run at B = 64 and no other test holds against a reference:

* the question encoder's step kernels (rnn_step_kernel<RNN_LSTM> / rnn_step_bwd_kernel<RNN_LSTM>) against the fp64 oracle over 1 - 4 question blocks
  (a workgroup owns 16 questions), ragged last blocks, questions of length 0, and the widths h = 384 / 512 at which the K loops
  take a second pass (forward: 16 k-groups per pass of h / 16; backward: 64 of h / 4, the later ones loaded from global memory);
* macx_adam_ema_step per element (p, m, v, ema and the norm) against a numpy fp64 evaluation of the header's formulas, over the
  grid-stride loop's second and third pass, within bounds DERIVED from the operation counts (opt_bounds; that they are fair --
  an fp32 evaluation in another summation order stays within half of what they hold beyond a result's own last rounding -- and
  sharp -- one update off by 2^-10 or a dropped eps is rejected -- is shown on the CPU, test_side_kernels_host.py);
* macx_gather_flat over more chunks than workgroups, entries that start a whole number of grids in, a misaligned destination.

`-s` prints every observed error / ratio."""
import numpy as np
import pytest
import torch

from abi_kit import bits_equal, ptr
from helpers import check_margin, rel_err

pytestmark = pytest.mark.gpu


# =====================================================================================================================
# 1. question encoder
# =====================================================================================================================
# (B, S, V, E, h, modes).  In this order: h = 128 before 384 / 512, so the backward kernel's LDS attribute is raised inside one
# process the way a real one raises it.
ENC_CASES = [(16, 3, 9, 7, 128, (False, True)),        # a full block with no clamp
             (17, 5, 13, 20, 128, (False, True)),      # second block with one live question
             (33, 4, 13, 20, 128, (False, True)),      # three blocks
             (64, 9, 30, 300, 256, (True,)),           # the bench's block count and widths
             (3, 4, 9, 20, 384, (False, True)),        # second K pass, half filled, in both directions; 117 KB of LDS
             (2, 3, 9, 20, 512, (False, True))]        # two full passes; 149,760 B of LDS
ENC_PARAMS = [pytest.param(B, S, V, E, h, train, id="B%d-S%d-E%d-h%d-%s" % (B, S, E, h, "train" if train else "eval"))
              for B, S, V, E, h, modes in ENC_CASES for train in modes]
ENC_TOL, ENC_GRAD_TOL, ENC_GRAD_FLOOR = 1e-5, 2e-4, 1e-7


def encoder_errors(macx, enc, words, vecQ, rw, rq, prm, lengths):
    """{name: (error, tolerance)} of one run_case result, plus the exact-zero findings (a list of strings, empty when clean)."""
    B, S = words.shape[:2]
    w, r = words.detach().cpu().double(), rw.detach().double()
    errs = {"words": (rel_err(words, rw), ENC_TOL), "vecQ": (rel_err(vecQ, rq), ENC_TOL)}
    worst, at = 0.0, -1
    for b in range(B):                                   # per question: a wrong block cannot hide behind a larger one
        if int(lengths[b]) == 0:
            continue
        e = float((w[b] - r[b]).abs().max() / r[b].abs().max())
        if e > worst:
            worst, at = e, b
    errs["words_per_question"] = (worst, ENC_TOL)
    for f, name in macx.encoder.REF_NAMES.items():
        errs["d_" + f] = (rel_err(getattr(enc, f).grad, prm[name].grad, floor=ENC_GRAD_FLOOR), ENC_GRAD_TOL)
    zeros = []
    vq = vecQ.detach().cpu()
    for b in range(B):
        L = int(lengths[b])
        if L < S and float(w[b, L:].abs().max()) != 0.0:
            zeros.append("words[%d, %d:] is not exactly 0" % (b, L))
        if L == 0 and float(vq[b].abs().max()) != 0.0:
            zeros.append("vecQ[%d] of a length-0 question is not exactly 0" % b)
        if L == 0 and (float(r[b].abs().max()) != 0.0 or float(rq[b].detach().abs().max()) != 0.0):
            zeros.append("the oracle's rows of length-0 question %d are not exactly 0" % b)
    return errs, zeros, at


@pytest.mark.parametrize("B,S,V,E,h,train", ENC_PARAMS)
def test_encoder_blocks_and_widths_against_fp64(macx, dev, B, S, V, E, h, train):
    from test_gpu_encoder import run_case
    enc, words, vecQ, rw, rq, prm, lengths = run_case(macx, dev, B, S, V, E, h, train, b0=2, min_len=0)
    assert int(lengths[0]) == S and int(lengths[1]) == 0
    errs, zeros, at = encoder_errors(macx, enc, words, vecQ, rw, rq, prm, lengths)
    tag = "side/enc/B%d_S%d_E%d_h%d_%s" % (B, S, E, h, "train" if train else "eval")
    print("\n%s: " % tag + ", ".join("%s %.2e" % (k, e) for k, (e, _) in errs.items()) + " (worst question %d, block %d)" % (at, at // 16))
    assert not zeros, zeros
    bad = {}
    for k, (e, tol) in errs.items():
        ok, bound = check_margin("%s/%s" % (tag, k), e, tol)
        if not ok:
            bad[k] = (e, bound)
    assert not bad, bad


def test_encoder_second_block_is_deterministic(macx, dev):
    from test_gpu_encoder import run_case
    runs = [run_case(macx, dev, 17, 5, 13, 20, 128, True, b0=2, min_len=0) for _ in range(2)]
    (e1, w1, q1, *_), (e2, w2, q2, *_) = runs
    assert bits_equal(w1.detach(), w2.detach()) and bits_equal(q1.detach(), q2.detach())
    for f in macx.encoder.REF_NAMES:
        assert bits_equal(getattr(e1, f).grad, getattr(e2, f).grad), f


# =====================================================================================================================
# 2. optimizer step: one step from a GIVEN state, per element
# =====================================================================================================================
OPT_PASS = 1024 * 256                                        # elements one pass of the grid covers (OPT_BLOCKS x 256 threads)
OPT_SIZES = (255, 257, OPT_PASS, OPT_PASS + 1, 2 * OPT_PASS + 77)
OPT_KINDS = ("clip", "x0.01", "x2^-30", "off")               # N(0,1) under clip = 8 | x 0.01 | x 2^-30 (clip inactive) | clip and EMA off
OPT_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3, decay=0.999)
U = 2.0 ** -24                                               # unit roundoff of fp32
TINY = 2.0 ** -126                                           # smallest normal fp32: what an underflowing operation can lose


def gamma(k):
    """(1 + u)^k - 1 <= k u / (1 - k u): k roundings in a row"""
    return k * U / (1.0 - k * U)


def opt_case(n, kind):
    """fp32 inputs of one step.  The gradient is ONE N(0,1) draw per n, scaled per kind; the state sits at the scale the clipped
    gradient has (m ~ g, v ~ g^2: what training at that gradient scale leaves), so that every term of every formula is live: neither
    moment swamps its gradient term, eps is half of the denominator at 2^-30 and the EMA has a distance to close."""
    gen = torch.Generator().manual_seed(4242 + n)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float32).numpy()
    base, p, rm, rv, re = r(), r(), r(), r(), r()
    gscale = {"clip": 1.0, "x0.01": 0.01, "x2^-30": 2.0 ** -30, "off": 1.0}[kind]
    sigma = np.float32(min(1.0, 8.0 / np.sqrt(n)) if kind == "clip" else gscale)
    c = dict(OPT_HYPER, n=n, kind=kind, clip=0.0 if kind == "off" else 8.0)
    if kind == "off":
        c["decay"] = -1.0
    c["g"] = base * np.float32(gscale)
    c["p"], c["m"], c["v"] = p, rm * sigma, np.square(rv * sigma)
    c["ema"] = p + np.float32(0.01) * re
    return c


def opt_lr_t(macx, c):
    return macx.optim.FlatAdamEMA.bias_corrected_lr(c["lr"], c["beta1"], c["beta2"], c["step"])


def opt_eval(c, lr_t, dt, drop_eps=False):
    """The header's formulas (include/macx.h, macx_adam_ema_step) in numpy at precision dt, on the fp32 inputs and the fp32 values
    of the scalars as the call receives them.  dt = float64: the reference.  dt = float32: every operation rounded once, the norm
    summed pairwise by np.sum -- another order than the kernel's."""
    f = lambda x: dt(np.float32(x))
    g, p, m, v, ema = [c[k].astype(dt) for k in ("g", "p", "m", "v", "ema")]
    b1, b2, eps, clip, decay, lr_t, one = f(c["beta1"]), f(c["beta2"]), f(c["eps"]), f(c["clip"]), f(c["decay"]), f(lr_t), dt(1)
    norm = np.sqrt(np.sum(g * g, dtype=dt))
    scale = clip / max(norm, clip) if clip > 0 else one
    gs = g * scale
    m1 = b1 * m + (one - b1) * gs
    v1 = b2 * v + (one - b2) * gs * gs
    upd = lr_t * m1 / (np.sqrt(v1) + (dt(0) if drop_eps else eps))
    p1 = p - upd
    e1 = ema - (one - decay) * (ema - p1) if decay >= 0 else ema
    assert all(x.dtype == dt for x in (norm, gs, m1, v1, upd, p1, e1))
    return dict(norm=norm, gs=gs, m=m1, v=v1, upd=upd, p=p1, ema=e1)


def opt_bounds(c, lr_t, ref):
    """Per-element error bounds of an fp32 evaluation against `ref` = opt_eval(c, lr_t, float64), from the operation counts alone.

    norm: a sum of non-negative terms whose longest addition chain has k links is within gamma(k) of the exact sum, relatively.  The
      kernels' chain: ceil(n / 262144) fused multiply-adds per thread, 6 shuffle steps, 3 for the four waves, up to 1024 partials
      added in a row.  The square root halves that and rounds once; eps_s = gamma(chain + 2) keeps the unhalved figure, and that
      factor 2 pays for every second-order term below.
    scale = clip / max(norm, clip) carries eps_s when the clip is active, and is exactly 1 when it is not.
    m = b1 m0 + (1 - b1) (g scale): 6 operations (b1 m0 | 1 - b1 | its product | the sum | g scale | clip / norm), so
      gamma(6) (|b1 m0| + |(1 - b1) gs|) + eps_s |(1 - b1) gs|.
    v = b2 v0 + (1 - b2) gs gs: 9 operations (gs enters twice, each time with its product and its division), so
      gamma(9) (b2 v0 + (1 - b2) gs^2) + 2 eps_s (1 - b2) gs^2.
    p = p0 - upd, upd = lr_t m / (sqrt(v) + eps): the first-order propagation of dm and dv, lr_t (dm / D + |m| dv / (2 sqrt(v) D^2))
      with D = sqrt(v) + eps, plus gamma(4) |upd| (product, root, sum, quotient), plus the final rounding: half an ulp of p.
    ema = ema0 - (1 - d) (ema0 - p): (1 - d) dp, plus gamma(3) |(1 - d) (ema0 - p)| (difference, 1 - d, product), plus half an ulp.
    Every bound has TINY on top: an operation whose result underflows loses at most that.
    out["final"]: the part of the p and ema bounds that is the LAST rounding alone.  A correctly rounded fp32 result reaches it by
    itself (half an ulp is what storing the value costs), so no evaluation can stay within a fraction of it; the fairness proof
    (test_side_kernels_host.py) halves only what a bound holds beyond it."""
    n = c["n"]
    f64 = lambda x: float(np.float32(x))
    b1, b2, eps, decay, lr_t = f64(c["beta1"]), f64(c["beta2"]), f64(c["eps"]), f64(c["decay"]), f64(lr_t)
    nparts = min(1024, -(-n // 256))
    chain = -(-n // OPT_PASS) + 6 + 3 + nparts
    eps_s = gamma(chain + 2)
    clipped = c["clip"] > 0 and float(ref["norm"]) > c["clip"]
    if c["clip"] > 0:             # the cases sit far from the threshold: both evaluations take the same side
        assert abs(float(ref["norm"]) - c["clip"]) > 100 * eps_s * c["clip"]
    eps_c = eps_s if clipped else 0.0
    gs, m, v, upd = np.abs(ref["gs"]), np.abs(ref["m"]), ref["v"], np.abs(ref["upd"])
    m0, v0 = np.abs(c["m"].astype(np.float64)), c["v"].astype(np.float64)
    gm, gv = (1 - b1) * gs, (1 - b2) * gs * gs
    dm = gamma(6) * (b1 * m0 + gm) + eps_c * gm + TINY
    dv = gamma(9) * (b2 * v0 + gv) + 2 * eps_c * gv + TINY
    D = np.sqrt(v) + eps
    dupd = lr_t * (dm / D + m * dv / (2 * np.sqrt(v) * D * D)) + gamma(4) * upd + TINY
    dp = U * (np.abs(ref["p"]) + dupd) + dupd
    out = dict(norm=eps_s * float(ref["norm"]) + TINY, m=dm, v=dv, p=dp, final=dict(p=U * np.abs(ref["p"])))
    if c["decay"] >= 0:
        e0 = c["ema"].astype(np.float64)
        out["ema"] = U * np.abs(ref["ema"]) + (1 - decay) * dp + gamma(3) * (1 - decay) * np.abs(e0 - ref["p"]) + TINY
        out["final"]["ema"] = U * np.abs(ref["ema"])
    return out


def opt_ratios(got, ref, bounds, beyond_final=None):
    """{tensor: (largest error / bound, where)} -- a ratio above 1 is a miss.  beyond_final = f: the bound is its last-rounding part
    plus the fraction f of the rest."""
    out = {}
    for k, b in bounds.items():
        if k == "final":
            continue
        if beyond_final is not None:
            fin = bounds["final"].get(k, 0.0)
            b = fin + beyond_final * (b - fin)
        q = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / b
        out[k] = (float(np.max(q)), int(np.argmax(q)) if np.ndim(q) else 0)
    return out


def _gpu_step(macx, dev, c, lr_t, device_rate=False, ema_buffer=True):
    """macx_adam_ema_step(_p) on copies of the case's state -> dict of numpy results (+ the ema buffer as it was left)."""
    L = macx._lib.lib()
    t = {k: torch.from_numpy(c[k].copy()).to(dev) for k in ("p", "g", "m", "v", "ema")}
    if c["decay"] < 0:
        t["ema"].fill_(-12345.0)                          # EMA off: the buffer (passed or not) must keep its sentinel
    ws, norm = torch.empty(1024, device=dev), torch.zeros(1, device=dev)
    ema = ptr(t["ema"]) if ema_buffer else None
    if device_rate:
        rate = torch.tensor([lr_t], dtype=torch.float32, device=dev)
        macx._lib.check(L.macx_adam_ema_step_p(c["n"], ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), ema, ptr(rate), c["beta1"], c["beta2"],
                                               c["eps"], c["clip"], c["decay"], ptr(ws), ptr(norm), None), "macx_adam_ema_step_p")
    else:
        macx._lib.check(L.macx_adam_ema_step(c["n"], ptr(t["p"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), ema, c["lr"], c["beta1"], c["beta2"],
                                             c["eps"], c["step"], c["clip"], c["decay"], ptr(ws), ptr(norm), None), "macx_adam_ema_step")
    torch.cuda.synchronize()
    assert bits_equal(t["g"].cpu(), torch.from_numpy(c["g"]))          # the gradient is read only
    out = {k: t[k].cpu().numpy() for k in ("p", "m", "v", "ema")}
    out["norm"] = float(norm.cpu()[0])
    return out


@pytest.mark.parametrize("kind", OPT_KINDS)
@pytest.mark.parametrize("n", OPT_SIZES)
def test_adam_ema_step_per_element(macx, dev, n, kind):
    c = opt_case(n, kind)
    lr_t = opt_lr_t(macx, c)
    ref = opt_eval(c, lr_t, np.float64)
    bounds = opt_bounds(c, lr_t, ref)
    got = _gpu_step(macx, dev, c, lr_t, ema_buffer=kind != "off")      # "off": ema = NULL
    ratios = opt_ratios(got, ref, bounds)
    print("\nside/opt/n%d/%s: " % (n, kind) + ", ".join("%s %.3f @%d" % (k, r, i) for k, (r, i) in ratios.items())
          + " (error / bound; pass %s)" % ", ".join("%s %d" % (k, i // OPT_PASS) for k, (r, i) in ratios.items() if k != "norm")
          + "; beyond the last rounding: " + ", ".join("%s %.3f" % (k, max(0.0, ((np.abs(got[k].astype(np.float64) - ref[k]) - f) / (bounds[k] - f)).max()))
                                                      for k, f in bounds["final"].items()))
    assert float(ref["norm"]) > 0 and (kind == "off" or (kind == "clip") == (float(ref["norm"]) > 8.0))     # the clip is live where named
    assert not np.array_equal(got["p"], c["p"]) and not np.array_equal(got["m"], c["m"]) and not np.array_equal(got["v"], c["v"])
    bad = {k: (r, i) for k, (r, i) in ratios.items() if not r <= 1.0}
    assert not bad, bad
    if kind == "off":
        assert bool((got["ema"] == -12345.0).all())
        again = _gpu_step(macx, dev, c, lr_t, ema_buffer=True)         # the buffer passed, the decay still off: not touched either
        assert bool((again["ema"] == -12345.0).all())
        assert all(np.array_equal(got[k].view(np.int32), again[k].view(np.int32)) for k in ("p", "m", "v")) and got["norm"] == again["norm"]
    else:
        assert not np.array_equal(got["ema"], c["ema"])


@pytest.mark.parametrize("n", [OPT_PASS + 1, 2 * OPT_PASS + 77])
def test_adam_ema_step_p_second_pass_bits(macx, dev, n):
    c = opt_case(n, "clip")
    lr_t = opt_lr_t(macx, c)
    a, b = _gpu_step(macx, dev, c, lr_t), _gpu_step(macx, dev, c, lr_t, device_rate=True)
    for k in ("p", "m", "v", "ema"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert a["norm"] == b["norm"]


# =====================================================================================================================
# 3. macx_gather_flat past one grid
# =====================================================================================================================
GATHER_G = 1024                                              # workgroups of the launch == floats of a chunk
# (count, what): offsets padded to 4 floats as FlatLayout pads them, except where `what` says otherwise
GATHER_ENTRIES = [(GATHER_G * 1023 + 5, "plain"),            # 1024 chunks: the next entry starts at base % G == 0 with base >= G; partial last quad
                  (3, "plain"),
                  (GATHER_G * 1030, "plain"),                # more chunks than workgroups: the c += G pass
                  (7, "src+1"),                              # source 4 bytes off a 16-byte boundary
                  (1021, "dst+1"),                           # aligned source, dst_offset = 1 (mod 4): the scalar path by the DESTINATION
                  (2 * GATHER_G * GATHER_G + 1, "zero")]     # src = NULL: zero fill across two grid passes


def test_gather_flat_past_one_grid(macx, dev):
    L = macx._lib.lib()
    al4 = lambda k: (k + 3) & ~3
    sentinel = -12345.0
    gen = torch.Generator().manual_seed(8)
    pool = torch.randn(sum(al4(k) + 4 for k, what in GATHER_ENTRIES if what != "zero"), generator=gen).to(dev)
    srcs, offsets, off, at = [], [], 0, 0
    for k, what in GATHER_ENTRIES:
        if what == "dst+1":
            off += 1
        offsets.append(off)
        off = al4(off + k)
        if what == "zero":
            srcs.append(None)
            continue
        lo = at + (1 if what == "src+1" else 0)
        srcs.append(pool[lo:lo + k])
        at += al4(k) + 4
    total = off + 8
    assert pool.data_ptr() % 16 == 0 and srcs[3].data_ptr() % 16 == 4 and srcs[4].data_ptr() % 16 == 0 and offsets[4] % 4 == 1
    assert all(o % 4 == 0 for i, o in enumerate(offsets) if i != 4) and 4_100_000 < total < 4_300_000
    want = torch.full((total,), sentinel, device=dev)
    pads = torch.ones(total, dtype=torch.bool)
    for s, o, (k, _) in zip(srcs, offsets, GATHER_ENTRIES):
        assert o + k <= total - 8                                        # every slice inside the buffer
        if s is None:
            want[o:o + k].zero_()
        else:
            want[o:o + k].copy_(s)
        pads[o:o + k] = False
    rows = [x for s, o, (k, _) in zip(srcs, offsets, GATHER_ENTRIES) for x in (0 if s is None else s.data_ptr(), o, k)]
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    outs = []
    for _ in range(2):
        flat = torch.full((total,), sentinel, device=dev)
        assert flat.data_ptr() % 16 == 0
        macx._lib.check(L.macx_gather_flat(ptr(table), len(GATHER_ENTRIES), ptr(flat), None),
                        "macx_gather_flat")
        torch.cuda.synchronize()
        outs.append(flat)
    flat = outs[0]
    if not bits_equal(flat, want):                                       # name the entry and the chunk of the first difference
        i = int(torch.nonzero(flat.view(torch.int32) != want.view(torch.int32))[0])
        e = max(j for j, o in enumerate(offsets) if o <= i)
        pytest.fail("flat[%d] = %r, expected %r: entry %d (%s), float %d of it, chunk %d"
                    % (i, float(flat[i]), float(want[i]), e, GATHER_ENTRIES[e][1], i - offsets[e], (i - offsets[e]) // 1024))
    assert int(pads.sum()) > 8 and bool((flat.cpu()[pads] == sentinel).all())    # every pad float and the 8 behind the end
    assert bits_equal(outs[0], outs[1])
