"""The recurrent question encoder (rnn_step_kernel<MODE> / rnn_step_bwd_kernel<MODE> of mac-network_amd/csrc/macx_rnn.hip.h, every cell's
step, and the host sequence rnn_forward / rnn_backward of macx_api.hip) at its block, width and length
edges: case table, data, reference, metrics, log.  No device, and nothing of the product is imported here (the callers hand `macx` in).

Shared by tests/test_gpu_recurrent_encoder_edges.py (the kernels) and tests/test_recurrent_encoder_cases_host.py (CPU: the metrics
shown fair and sharp, the table's paths against the restated grid rules, the sizing calls).

Grid rules of the kernels, restated in route() (held to the C++ text by the host file):
  * every launch: grid (h / 16, ceil(B / 16), dirs); a workgroup owns 16 questions x 16 units of one direction, a ragged last block
    clamps its rows to B - 1 and drops them at the write;
  * forward: four waves, PF = 4 k-groups of 16 in flight per wave, so a pass of the K loop covers 16 of the h / 16 k-groups; a group past
    the end is clamped to the last one and skipped by Q0 + 4 u < nQ;
  * backward: 16 waves x PF = 4, a pass covers 64 of the nQ = NG h / 16 k-groups (NG = 1 RNN and GRU candidate, 2 GRU gates, 4 LSTM);
    wave w holds the groups w + 16 u + 64 p; its LDS is rnn_step_bwd_lds(h, NG) = (16 (NG h + 4) + 256 + 16 16 17) floats;
  * the running dh alternates between two buffers with the parity of S - 1 - tau; hs is indexed (dir (S + 1) + tau).

Data.  Parameters from RecurrentQuestionEncoder's generator (seed 3) with the non-zero biases of test_gpu_recurrent_encoder.make_encoder
(seed 7); questions and lengths per pattern; cotangents randn / B (seed 5); the hashed dropout masks of seed SEED at b0 = B0.

Reference.  rnn_ref.question_encoder in fp64 under oracle.dropout_hash masks, built as test_gpu_recurrent_encoder.run_case builds it.

Metrics (errors()).  Tolerances are the project's own for this arithmetic, ENC_TOL = 1e-5 on outputs and ENC_GRAD_TOL = 2e-4 on gradients
(test_gpu_side_kernels.py); what is new is the DENOMINATOR: a row's, a column's or a block's own largest reference entry, never the
tensor's.
  words     per (question, position, direction): largest difference over the h units / the row's largest reference entry; positions
            past a question's end exactly +0; a length-0 question exactly zero
  vecQ      per (question, direction); a length-0 question exactly zero
  d kernel  split into input rows [0, E) and recurrent rows [E, E + h) and into its column blocks (r | u of the GRU's gates, c of its
            candidate, i | j | f | o of the LSTM, one block for the RNN); in each part per column and per row, relative to that
            column's or row's largest reference entry inside the part, floored at 1e-7 x the part's largest entry
  d bias    per column block, relative to the block's largest reference entry (per element is NOT fair: near-cancelled entries of an
            fp32 evaluation reach 1e-4)
  d emb     per token row; the row of a token no live position holds exactly zero
"""
import collections
import math
import os

import numpy as np
import torch

import rnn_ref
from oracle import dropout_hash as dh
from oracle import mac_oracle as mo

ENC_TOL, ENC_GRAD_TOL = 1e-5, 2e-4          # test_gpu_side_kernels.ENC_TOL / ENC_GRAD_TOL
PART_FLOOR = 1e-7                           # x the part's largest entry
FAIR = 1.0 / 3.0
SEED, B0 = 9, 2
PAIRS5 = (("RNN", 1), ("RNN", 2), ("GRU", 1), ("GRU", 2), ("LSTM", 1))
PATTERNS = ("draw", "all_S", "all_1", "ascending", "descending", "alternating")
NG = {"RNN": (1,), "GRU": (1, 2), "LSTM": (4,)}          # gates per backward launch (GRU: candidate, then gates)
RSB_THREADS, PF = 1024, 4


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "B S V E h cell dirs train pattern pool draw reaches")):
    """pattern: how the lengths are set (lengths()); pool: how many of the V tokens the questions draw from (None: all);
    draw: which draw of questions and lengths the row runs on (0 everywhere: no row needed the next one to be fair)"""
    id = property(lambda c: "%sx%d-B%d-S%d-E%d-h%d-%s-%s%s" % (c.cell, c.dirs, c.B, c.S, c.E, c.h, "train" if c.train else "eval", c.pattern,
                                                                 "" if c.pool is None else "-pool%d" % c.pool))
    bi = property(lambda c: c.dirs == 2)
    old_path = property(lambda c: c.cell == "LSTM" and c.dirs == 2)       # macx_encoder_* (macx.QuestionEncoder)


def _case(B, S, V, E, h, pair, train, reaches, pattern="draw", pool=None, draw=0):
    assert pattern in PATTERNS and h in (128, 256, 384, 512)
    return Case(B, S, V, E, h, pair[0], pair[1], train, pattern, pool, draw, reaches)


def _table():
    rows = []
    # h = 128 first: the backward kernels' LDS attribute is raised inside one process the way a real one raises it
    for B, S, train, why in ((33, 4, True, "three question blocks, the third with one live row"),
                             (49, 3, False, "four question blocks, the fourth with one live row; S odd"),
                             (64, 3, True, "four full question blocks")):
        rows += [_case(B, S, 13, 20, 128, pair, train, why) for pair in PAIRS5]
    rows += [_case(64, 9, 30, 300, 256, pair, True, "the bench's block count and widths: an exactly full forward K pass, the padded embedding")
             for pair in (("GRU", 2), ("RNN", 1), ("LSTM", 1))]
    rows += [_case(3, 4, 9, 20, 384, pair, train, "h = 384: a second forward K pass, half filled; backward waves 0 to 7 with one k-group "
                   "more than waves 8 to 15") for train in (False, True) for pair in PAIRS5]
    for B in (2, 17):      # (B = 2: both questions full, see the S = 2 rows below)
        rows += [_case(B, 3, 9, 20, 512, pair, True, "h = 512: two full forward K passes; the GRU gates' 64 k-groups fill the backward pass "
                       "on 84 KB of LDS" + ("; two question blocks" if B == 17 else ""), pattern="draw" if B == 17 else "all_S")
                 for pair in (("RNN", 1), ("RNN", 2), ("GRU", 2))]
    for B, E, train in ((3, 20, False), (17, 300, True)):
        rows += [_case(B, 50, 13, E, 128, pair, train, "the workload's length: 50 steps of round-off, 25 toggles of the dh buffer pair, hs "
                       "rows up to dir 51 + 50") for pair in PAIRS5 + (("LSTM", 2),)]
    # B = 2 with question 1 empty leaves ONE live question: with one or two recurrent steps every recurrent part of a kernel gradient is
    # then one or two outer products, "per column" is per element, and an entry of dG_u that (h - c) nearly cancels decides the figure
    # (the fp32 restatement over the first draws of GRU x 2 at S = 2: 2.0e-4, 1.8e-4, 1.2e-4 of that column, and another CPU moves them by
    # half).  That is the data's doing, not a kernel's, so both questions of these rows are full (pattern all_S): 0.06 of a tolerance at most.
    rows += [_case(2, 2, 9, 16, 128, pair, True, "S = 2: the first toggle of the dh buffer pair", pattern="all_S") for pair in PAIRS5]
    for pattern, why in (("all_S", "no inactive lane in any block"), ("all_1", "the reverse direction reads position 0 only"),
                         ("ascending", "lengths b % (S + 1) across the block boundaries"),
                         ("descending", "lengths S - b % (S + 1) across the block boundaries"),
                         ("alternating", "lengths 0 and S alternating: every other lane inactive throughout")):
        rows += [_case(33, 6, 13, 20, 128, pair, pattern != "all_S", why, pattern=pattern) for pair in (("GRU", 2), ("RNN", 2))]
    rows.append(_case(17, 5, 300, 20, 128, ("GRU", 1), True, "a vocabulary of 300 with 40 tokens in use: 260 embedding rows exactly zero", pool=40))
    return rows


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
DETERMINISM_IDS = ("GRUx2-B33-S4-E20-h128-train-draw", "RNNx1-B17-S50-E300-h128-train-draw")
PERMUTATION_CASES = [c._replace(train=False) for c in CASES if c.B == 33]
HOMOGENEITY_CASES = [_case(17, 5, 13, 20, 128, pair, True, "linear in the cotangents") for pair in (("GRU", 2), ("RNN", 1))]
COTANGENT_CASES = [_case(17, 5, 13, 20, 128, pair, True, "one cotangent at a time") for pair in (("GRU", 2), ("LSTM", 1))]
CLAMP_CASES = [_case(17, 5, 13, 20, 128, pair, True, "lengths outside [0, S]") for pair in (("GRU", 2), ("LSTM", 1))]
WARM_UP = {pair: _case(2, 2, 9, 16, 128, pair, False, "h = 128 before a wider row in the same process") for pair in PAIRS5 + (("LSTM", 2),)}


def lengths_of(c):
    """[B] int32.  draw: uniform in [0, S] with question 0 full and question 1 empty (test_gpu_encoder.make_questions, min_len = 0)"""
    b, S = torch.arange(c.B), c.S
    if c.pattern == "draw":
        g = torch.Generator().manual_seed(11 + 1000 * c.draw)
        L = torch.randint(0, S + 1, (c.B,), generator=g, dtype=torch.int32)
        L[0] = S
        if c.B > 1:
            L[1] = 0
        return L
    return {"all_S": torch.full((c.B,), S), "all_1": torch.ones(c.B), "ascending": b % (S + 1), "descending": S - b % (S + 1),
            "alternating": torch.where(b % 2 == 0, 0, S)}[c.pattern].to(torch.int32)


Data = collections.namedtuple("Data", "q lengths d_words d_vecQ")


def make_data(c):
    """questions [B,S] int32 (0 = pad past a question's end), lengths [B] int32, the two cotangents in fp32"""
    L = lengths_of(c)
    g = torch.Generator().manual_seed(12 + 1000 * c.draw)
    if c.pool is None:
        q = torch.randint(1, c.V + 1, (c.B, c.S), generator=g, dtype=torch.int32)
    else:
        ids = (torch.randperm(c.V, generator=g)[:c.pool] + 1).to(torch.int32)
        q = ids[torch.randint(0, c.pool, (c.B, c.S), generator=g)]
    q = q * (torch.arange(c.S).unsqueeze(0) < L.unsqueeze(1)).to(torch.int32)
    g = torch.Generator().manual_seed(5)
    w = c.dirs * c.h
    return Data(q, L, torch.randn(c.B, c.S, w, generator=g) / c.B, torch.randn(c.B, w, generator=g) / c.B)


def config(c, **over):
    enc = c.dirs * c.h
    return mo.flag_file_config("args", encType=c.cell, encBi=c.bi, ctrlDim=enc, memDim=enc, attDim=enc, encDim=enc, wrdEmbDim=c.E, **over)


def make_encoder(macx, c, dev=None):
    """test_gpu_recurrent_encoder.make_encoder: the class's own draw (seed 3) and biases moved off their initial values (seed 7)"""
    enc = macx.RecurrentQuestionEncoder(config(c), vocab=c.V, generator=torch.Generator().manual_seed(3))
    gb = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for f in enc.FIELDS:
            if f.endswith("bias"):
                getattr(enc, f).add_(torch.rand(getattr(enc, f).shape, generator=gb) - 0.5)
    return enc if dev is None else enc.to(dev)


def masks_of(c, dtype=torch.float64):
    if not c.train:
        return None
    ki, kq = keeps(c)
    return [torch.from_numpy(dh.mask_for(SEED, 11, 0, ki, (c.B, c.S, c.E), b0=B0)).to(dtype),
            torch.from_numpy(dh.mask_for(SEED, 12, 0, kq, (c.B, c.dirs * c.h), b0=B0)).to(dtype)]


def keeps(c):
    cfg = config(c)
    return (float(cfg.encInputDropout), float(cfg.qDropout)) if c.train else (1.0, 1.0)


def reference(macx, c, dtype=torch.float64, d_words=True, d_vecQ=True, scale=1.0):
    """{"words", "vecQ", "grads": {field: tensor}} of rnn_ref.question_encoder in `dtype` (fp64: the reference; fp32: torch's CPU
    kernels, another summation order -- what the fairness proof measures) with the loss (words d_words).sum() + (vecQ d_vecQ).sum()"""
    enc, data = make_encoder(macx, c), make_data(c)
    prm = {k: v.to(dtype).requires_grad_(True) for k, v in enc.to_reference_dict().items()}
    ki, kq = keeps(c)
    rw, rq = rnn_ref.question_encoder(config(c), mo.VarStore(params=prm, dtype=dtype), data.q, data.lengths, c.V, keep_input=ki, keep_question=kq,
                                      masks=masks_of(c, dtype))
    loss = 0
    if d_words:
        loss = loss + (rw * (data.d_words * scale).to(dtype)).sum()
    if d_vecQ:
        loss = loss + (rq * (data.d_vecQ * scale).to(dtype)).sum()
    loss.backward()
    return dict(words=rw.detach(), vecQ=rq.detach(), grads={f: prm[enc.REF_NAMES[f]].grad for f in enc.FIELDS})


_REFS = {}


def cached_reference(macx, c):
    """the fp64 reference of a table row, computed once per process and left unchanged"""
    if c not in _REFS:
        _REFS[c] = reference(macx, c)
    return _REFS[c]


# ---------------------------------------------------------------------------------------------------------------------------
# the grid rules, restated
# ---------------------------------------------------------------------------------------------------------------------------
def rnn_step_bwd_lds(h, gates):
    return (16 * (gates * h + 4) + 256 + (RSB_THREADS // 64) * 16 * 17) * 4


def bwd_groups(h, gates):
    """k-groups of each of the 16 waves: wave w holds w + 16 u + 64 p < nQ"""
    nQ, NW = gates * h // 16, RSB_THREADS // 64
    return [len(range(w, nQ, NW)) for w in range(NW)]


def route(c):
    nQ = c.h // 16
    passes = -(-nQ // 16)
    out = dict(grid=(c.h // 16, -(-c.B // 16), c.dirs), live_in_last_block=c.B - 16 * ((c.B - 1) // 16),
               fwd_passes=passes, fwd_last_fill=nQ - 16 * (passes - 1), S_odd=c.S % 2 == 1, toggles=c.S - 1,
               hs_last_row=(c.dirs - 1) * (c.S + 1) + c.S)
    out["bwd"] = {g: dict(groups=bwd_groups(c.h, g), nQ=g * c.h // 16, passes=-(-(g * c.h // 16) // 64), lds=rnn_step_bwd_lds(c.h, g))
                  for g in NG[c.cell]}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------
def kernel_fields(fields):
    return [f for f in fields if f.endswith("kernel")]


def blocks_of(cell, field):
    """[(name, first block of h columns)] of a kernel or bias"""
    if cell == "RNN":
        return [("h", 0)]
    if cell == "LSTM":
        return [(n, k) for k, n in enumerate("ijfo")]
    return [("c", 0)] if "candidate" in field else [("r", 0), ("u", 1)]


def _f64(t):
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).detach().cpu().double()


def _worst(q):
    i = int(torch.argmax(q.reshape(-1)))
    return float(q.reshape(-1)[i]), np.unravel_index(i, tuple(q.shape))


def _ratio(err, scale):
    """err / scale; where the reference scale is exactly zero the result must be exactly zero (else inf)"""
    q = err / scale.clamp_min(1e-300)
    return torch.where(scale > 0, q, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def _not_plus_zero(t):
    t = (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).detach().cpu()
    return (t != 0) | torch.signbit(t)


def unit_where(u):
    return "unit %d (unit // 16 = %d)" % (u, u // 16)


def errors(c, got, ref, data=None):
    """{name: (value, tolerance, where)}: got and ref as reference() returns them (got in fp32 from the device, or any CPU evaluation);
    a broken exact-zero condition is a value of inf"""
    data = data or make_data(c)
    L, h, D = data.lengths.long(), c.h, c.dirs
    out = {}
    live = torch.arange(c.S).unsqueeze(0) < L.unsqueeze(1)                                        # [B,S]
    # words
    g, r = _f64(got["words"]).reshape(c.B, c.S, D, h), _f64(ref["words"]).reshape(c.B, c.S, D, h)
    q = _ratio((g - r).abs().amax(-1), r.abs().amax(-1))
    bad = _not_plus_zero(got["words"]).reshape(c.B, c.S, D, h).any(-1) & ~live.unsqueeze(-1)
    q = torch.where(bad, torch.full_like(q, math.inf), q)
    v, (b, s, d) = _worst(q)
    u = int(torch.argmax((g - r).abs()[b, s, d]))
    out["words"] = (v, ENC_TOL, "question %d (block %d, length %d) position %d direction %d %s%s"
                    % (b, b // 16, int(L[b]), s, d, unit_where(u), " NOT +0 PAST THE END" if bool(bad[b, s, d]) else ""))
    # vecQ
    g, r = _f64(got["vecQ"]).reshape(c.B, D, h), _f64(ref["vecQ"]).reshape(c.B, D, h)
    q = _ratio((g - r).abs().amax(-1), r.abs().amax(-1))
    q = torch.where(((g != 0).any(-1)) & (L == 0).unsqueeze(-1), torch.full_like(q, math.inf), q)
    v, (b, d) = _worst(q)
    u = int(torch.argmax((g - r).abs()[b, d]))
    out["vecQ"] = (v, ENC_TOL, "question %d (block %d, length %d) direction %d %s" % (b, b // 16, int(L[b]), d, unit_where(u)))
    # gradients
    for f, gr in got["grads"].items():
        if gr is None:
            continue
        g, r = _f64(gr), _f64(ref["grads"][f])
        assert g.shape == r.shape, (f, g.shape, r.shape)
        if f == "emb":
            q = _ratio((g - r).abs().amax(-1), r.abs().amax(-1))
            held = torch.zeros(c.V + 1, dtype=torch.bool)
            held[data.q[live].long()] = True
            q = torch.where((g != 0).any(-1) & ~held[1:], torch.full_like(q, math.inf), q)
            v, (t,) = _worst(q)
            out["d emb"] = (v, ENC_GRAD_TOL, "token %d (embedding row %d, %s)" % (t + 1, t, "held by a live position" if bool(held[t + 1]) else "held by none"))
        elif f.endswith("bias"):
            for name, k in blocks_of(c.cell, f):
                gb, rb = g[k * h:(k + 1) * h], r[k * h:(k + 1) * h]
                v, (u,) = _worst(_ratio((gb - rb).abs(), rb.abs().amax().expand(h)))
                out["d %s/%s" % (f, name)] = (v, ENC_GRAD_TOL, "block %s %s" % (name, unit_where(u)))
        else:
            for part, lo, hi in (("in", 0, c.E), ("rec", c.E, c.E + h)):
                for name, k in blocks_of(c.cell, f):
                    gp, rp = g[lo:hi, k * h:(k + 1) * h], r[lo:hi, k * h:(k + 1) * h]
                    err, top = (gp - rp).abs(), float(rp.abs().max())
                    for axis, what in ((0, "col"), (1, "row")):
                        scale = rp.abs().amax(axis)
                        q = _ratio(err.amax(axis), scale.clamp_min(PART_FLOOR * top) if top > 0 else scale)
                        v, (i,) = _worst(q)
                        j = int(torch.argmax(err[:, i] if axis == 0 else err[i]))
                        row, u = (j, i) if axis == 0 else (i, j)
                        out["d %s %s/%s %s" % (f, part, name, what)] = (v, ENC_GRAD_TOL, "%s row %d (kernel row %d), block %s %s"
                                                                        % (part, row, lo + row, name, unit_where(u)))
    return out


def failures(errs):
    return {k: v for k, v in errs.items() if not v[0] <= v[1]}


def group_of(name):
    """the log's columns: words | vecQ | d emb | d bias | d kernel in col | in row | rec col | rec row"""
    if name in ("words", "vecQ", "d emb"):
        return name
    if "bias" in name:
        return "d bias"
    _, _, part, what = name.split(" ")
    return "d kernel %s %s" % (part.split("/")[0], what)


GROUPS = ("words", "vecQ", "d emb", "d bias", "d kernel in col", "d kernel in row", "d kernel rec col", "d kernel rec row")


def worst_by_group(errs):
    """{group: (largest value / tolerance, metric name, where)}"""
    out = {}
    for k, (v, tol, where) in errs.items():
        g = group_of(k)
        if g not in out or v / tol > out[g][0]:
            out[g] = (v / tol, k, where)
    return out


def line(c, what, errs):
    w = worst_by_group(errs)
    return "%-44s %-10s " % (c.id, what) + "  ".join("%s %.4f" % (g, w[g][0]) for g in GROUPS if g in w)


def old_rel_errs(c, got, ref):
    """what test_gpu_recurrent_encoder.check_case measures: helpers.rel_err per tensor -> {name: (value, tolerance)}"""
    from helpers import rel_err
    out = {"words": (rel_err(_f64(got["words"]), ref["words"]), 1e-5), "vecQ": (rel_err(_f64(got["vecQ"]), ref["vecQ"]), 1e-5)}
    for f, g in got["grads"].items():
        if g is not None:
            out["d " + f] = (rel_err(_f64(g), ref["grads"][f], floor=1e-7), 2e-4)
    return out


def log(text):
    """append to the file MACX_RECURRENT_ENCODER_LOG names (how profiles/recurrent_encoder_errors.txt is recorded); always printed (-s)"""
    print(text)
    path = os.environ.get("MACX_RECURRENT_ENCODER_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(text + "\n")


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' loops in numpy (fp32 by default), with the defects of the sharpness proof
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "reverse_position": "a question's reverse direction reads position L - tau instead of L - 1 - tau",
    "zeroed_state": "one question's state is zeroed instead of carried past its end",
    "candidate_h": "the candidate is fed h instead of r * h for one question",
    "swapped_gates": "r and u are swapped in one 16-unit block",
    "missing_step": "one time step is missing from one question's sum into the recurrent rows of a kernel gradient",
    "bias_block": "one 16-question block is left out of a bias gradient",
    "neighbour_column": "one unit's recurrent column is taken from its neighbour",
}
DEFECT_BLOCK, DEFECT_UNIT = slice(16, 32), 37


def victim(c, lengths, lo, hi=None):
    """the first question with lo <= length <= hi (None: S), or None"""
    hi = c.S if hi is None else hi
    for b, n in enumerate(lengths.tolist()):
        if lo <= n <= hi:
            return b
    return None


def defect_is_live(name, c, lengths=None):
    L = lengths_of(c) if lengths is None else lengths
    if c.old_path and name in ("candidate_h", "swapped_gates"):
        return False
    return {"reverse_position": c.dirs == 2 and victim(c, L, 2) is not None,
            "zeroed_state": victim(c, L, 1, c.S - 1) is not None,
            "candidate_h": c.cell == "GRU" and victim(c, L, 2) is not None,
            "swapped_gates": c.cell == "GRU" and victim(c, L, 1) is not None,
            "missing_step": victim(c, L, 2) is not None,
            "bias_block": bool((L[16 * ((c.B - 1) // 16):] > 0).any()),
            "neighbour_column": victim(c, L, 2) is not None}[name]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def restated(macx, c, dtype=np.float32, defect=None):
    """rnn_forward / rnn_backward of macx_api.hip as plain loops: Zx = X Wx + b for every position, one cell step per tau with the state
    copied through past a question's end, the backward steps with their dG (per step) and dZ (per position), the kernel gradients as
    X^T dZ and sum_tau h_prev^T dG_tau, the bias gradients as dG's column sums -> what reference() returns.  defect: a key of DEFECTS."""
    enc, data = make_encoder(macx, c), make_data(c)
    P = {f: getattr(enc, f).detach().numpy().astype(dtype) for f in enc.FIELDS}
    B, S, E, h, D = c.B, c.S, c.E, c.h, c.dirs
    q, L = data.q.numpy().astype(np.int64), np.clip(data.lengths.numpy().astype(np.int64), 0, S)
    ki, kq = keeps(c)
    m = masks_of(c)
    m_in = np.ones((B, S, E), dtype) if m is None else (m[0].numpy().astype(dtype) / dtype(ki))
    m_q = np.ones((B, D * h), dtype) if m is None else (m[1].numpy().astype(dtype) / dtype(kq))
    X = np.concatenate([np.zeros((1, E), dtype), P["emb"]], 0)[q] * m_in
    dW, dQ = data.d_words.numpy().astype(dtype), data.d_vecQ.numpy().astype(dtype) * m_q
    rows = np.arange(B)
    mats = {"RNN": [("", 1)], "LSTM": [("", 4)], "GRU": [("", 2), ("candidate_", 1)]}[c.cell]
    vb = {"reverse_position": victim(c, data.lengths, 2), "zeroed_state": victim(c, data.lengths, 1, S - 1),
          "candidate_h": victim(c, data.lengths, 2), "missing_step": victim(c, data.lengths, 2)}.get(defect)
    words, vec, grads = np.zeros((B, S, D * h), dtype), np.zeros((B, D * h), dtype), {f: np.zeros_like(v) for f, v in P.items()}
    dX = np.zeros((B, S, E), dtype)
    for d, dn in enumerate(("fw", "bw")[:D]):
        K = [P["%s_%skernel" % (dn, pre)].copy() for pre, _ in mats]
        bias = [P["%s_%sbias" % (dn, pre)].copy() for pre, _ in mats]
        if d == 0 and defect == "swapped_gates":
            for t in (K[0], bias[0]):
                lo, hi = t[..., DEFECT_BLOCK].copy(), t[..., h + DEFECT_BLOCK.start:h + DEFECT_BLOCK.stop].copy()
                t[..., DEFECT_BLOCK], t[..., h + DEFECT_BLOCK.start:h + DEFECT_BLOCK.stop] = hi, lo
        if d == 0 and defect == "neighbour_column":
            K[0][E:, DEFECT_UNIT] = K[0][E:, DEFECT_UNIT + 1]
        Zx = [X.reshape(B * S, E) @ k[:E] + b for k, b in zip(K, bias)]
        Zx = [z.reshape(B, S, -1) for z in Zx]
        hst, cst = np.zeros((B, h), dtype), np.zeros((B, h), dtype)
        steps = []
        for tau in range(S):
            active = tau < L
            pos = np.full(B, tau) if d == 0 else np.maximum(L - 1 - tau, 0)
            rpos = pos.copy()
            if defect == "reverse_position" and d == 1:
                rpos[vb] = min(L[vb] - tau, S - 1) if L[vb] - tau >= 0 else 0
            z = [zz[rows, rpos] for zz in Zx]
            st = dict(active=active, pos=pos, rpos=rpos, hp=hst, cp=cst)
            if c.cell == "RNN":
                hn = np.tanh(hst @ K[0][E:] + z[0])
                cn = cst
            elif c.cell == "GRU":
                g = _sig(hst @ K[0][E:] + z[0]).astype(dtype)
                r, u = g[:, :h], g[:, h:]
                rc = r.copy()
                if defect == "candidate_h":
                    rc[vb] = 1
                rh = rc * hst
                cand = np.tanh(rh @ K[1][E:] + z[1])
                hn = u * hst + (1 - u) * cand
                cn = cst
                st.update(r=r, u=u, c=cand, rc=rc, rh=rh)
            else:
                a = hst @ K[0][E:] + z[0]
                gi, gj, gf, go = _sig(a[:, :h]).astype(dtype), np.tanh(a[:, h:2 * h]), _sig(a[:, 2 * h:3 * h] + 1).astype(dtype), _sig(a[:, 3 * h:]).astype(dtype)
                cn = cst * gf + gi * gj
                hn = np.tanh(cn) * go
                st.update(gi=gi, gj=gj, gf=gf, go=go, cn=cn)
            st["hn"] = hn
            words[rows[active], pos[active], d * h:(d + 1) * h] = hn[active]
            keep = ~active[:, None]
            hst, cst = np.where(keep, hst, hn), np.where(keep, cst, cn)
            if defect == "zeroed_state":
                gone = np.zeros(B, bool)
                gone[vb] = not active[vb]
                hst, cst = np.where(gone[:, None], 0, hst).astype(dtype), np.where(gone[:, None], 0, cst).astype(dtype)
                st["gone"] = gone
            steps.append(st)
        vec[:, d * h:(d + 1) * h] = hst
        # ---- backward
        dh, dc = dQ[:, d * h:(d + 1) * h].copy(), np.zeros((B, h), dtype)
        dZ = [np.zeros((B, S, w * h), dtype) for _, w in mats]
        dKrec = [np.zeros((h, w * h), dtype) for _, w in mats]
        dB = [np.zeros(w * h, dtype) for _, w in mats]
        for tau in reversed(range(S)):
            st = steps[tau]
            act = st["active"][:, None]
            if "gone" in st:
                dh, dc = np.where(st["gone"][:, None], 0, dh).astype(dtype), np.where(st["gone"][:, None], 0, dc).astype(dtype)
            dht = dh + np.where(act, dW[rows, st["pos"], d * h:(d + 1) * h], 0)
            if c.cell == "RNN":
                dG = [np.where(act, dht * (1 - st["hn"] ** 2), 0).astype(dtype)]
                new = dG[0] @ K[0][E:].T
                A = [st["hp"]]
            elif c.cell == "GRU":
                r, u, cand, hp = st["r"], st["u"], st["c"], st["hp"]
                gc = np.where(act, dht * (1 - u) * (1 - cand * cand), 0).astype(dtype)
                drh = gc @ K[1][E:].T
                gr = drh * hp * r * (1 - r)
                if defect == "candidate_h":
                    gr[vb] = 0
                gu = dht * (hp - cand) * u * (1 - u)
                gg = np.where(act, np.concatenate([gr, gu], 1), 0).astype(dtype)
                new = gg @ K[0][E:].T + drh * st["rc"] + dht * u
                dG, A = [gg, gc], [hp, st["rh"]]
            else:
                gi, gj, gf, go = st["gi"], st["gj"], st["gf"], st["go"]
                tc = np.tanh(st["cn"])
                dO = dht * tc * go * (1 - go)
                dct = dc + dht * go * (1 - tc * tc)
                gg = np.concatenate([dct * gj * gi * (1 - gi), dct * gi * (1 - gj * gj), dct * st["cp"] * gf * (1 - gf), dO], 1)
                gg = np.where(act, gg, 0).astype(dtype)
                dc = np.where(act, dct * gf, dc).astype(dtype)
                new = gg @ K[0][E:].T
                dG, A = [gg], [st["hp"]]
            dh = np.where(act, new, dh).astype(dtype)
            a1 = st["active"]
            for mi in range(len(mats)):
                dZ[mi][rows[a1], st["rpos"][a1]] = dG[mi][a1]
                Am = A[mi]
                if defect == "missing_step" and d == 0 and mi == 0 and tau == 1:
                    Am = Am.copy()
                    Am[vb] = 0
                dKrec[mi] += Am.T @ dG[mi]
                lo = 16 * ((B - 1) // 16) if (defect == "bias_block" and d == 0 and mi == 0) else B
                dB[mi] += dG[mi][:lo].sum(0)
        for mi, (pre, w) in enumerate(mats):
            grads["%s_%skernel" % (dn, pre)] = np.concatenate([X.reshape(B * S, E).T @ dZ[mi].reshape(B * S, -1), dKrec[mi]], 0)
            grads["%s_%sbias" % (dn, pre)] = dB[mi]
            dX += (dZ[mi].reshape(B * S, -1) @ K[mi][:E].T).reshape(B, S, E)
    dX = dX * m_in
    np.add.at(grads["emb"], q[q > 0] - 1, dX[q > 0])
    return dict(words=words, vecQ=vec * m_q, grads=grads)
