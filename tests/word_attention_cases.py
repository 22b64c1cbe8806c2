"""The word attention of the control unit (control_attend_kernel, control_bwd_dl_kernel, control_bwd_apply_kernel of
mac-network_amd/csrc/macx_small.hip.h) at its batch, slab and step edges: case tables, data, reference, bounds.  No device.

Shared by tests/test_gpu_word_attention.py (the kernels) and tests/test_word_attention_host.py (CPU: the reference against the oracle,
the bounds shown fair and sharp, the inputs live, the table's paths against the restated loop rules, the workspace size).

Loop rules of the three kernels, restated below (held to the C++ text by the host file):
  * logit and da passes: wave w of four takes the words w + 4 u + 32 t, u < CA_U = 8, trip t; a row past the end re-reads word
    min(s, S - 1) and is dropped by s < S; a lane takes 4 columns per pass of 256;
  * softmax, dot and the dl sum: one word per thread (S <= C_MAXS = 256 = the block), six shuffle steps, (r0 + r1) + (r2 + r3);
  * control: thread t takes columns 2 t, 2 t + 1 per pass of 512 and walks the S words with fused multiply-adds;
  * apply: one workgroup per (question, 64-column slab), 64 words per pass through LDS; group g of four owns the steps z = g + 4 i in
    Racc[i], i < CB_MAXZ / 4 = 8, carried across the passes, and the words s = g + 4 j of a pass for d_words, summed over z in order;
  * d_w: per question cc R summed per group, (g0 + g1) + (g2 + g3), then rowsum over the questions; d_b: rowsum over nz B partials;
  * recurrent control: one launch pair per step with nz = 1, d_words and the d_w partials read, added to and written back.

Bounds.  u = 2^-24; every bound is k u sum|terms| with k an operation count, the terms those of the fp64 run:
  logit_s      E_s = (d + 4) u (sum_k |cc w words_s| + |b|): any order of d additions, the two products, the bias;
  att_s        att_s rho_s, rho_s = E_s + sum_j att_j E_j + (|l_s - max| + 16) u: the softmax carries a logit error dl_s as
               dl_s - sum_j att_j dl_j; the difference l - max is rounded (u |l_s - max| in the exponent); 16 = expf in the numerator
               and in the terms of the sum (2 + 2), the sum (own term, six shuffle steps, two for the waves: 9), the reciprocal (2),
               the product (1);
  control_k    sum_s (rho_s + (S + 1) u) |att_s words_sk|: a chain of S fused multiply-adds;
  da_s         e_da = K_D u (sum_k |dc words_s| + |g_s|), K_D = 4 ceil(d / 256) + 8: a lane's chain, six shuffle steps, the product, g;
  dot          e_dot = sum_s (rho_s + 10 u) |att_s da_s| + sum_s att_s e_da_s (product, own term, six steps, two for the waves);
  dl_s         e_dl = (rho_s + 2 u) |dl_s| + att_s (e_da_s + e_dot);
  d_cc_k       |w_k| sum_s (e_dl_s + (S + 2) u |dl_s|) |words_sk|: S fused multiply-adds into R, the product with w;
  d_w_k        sum_z sum_b |cc_k| sum_s (e_dl_s + (S + 2 + B + Z) u |dl_s|) |words_sk|: as d_cc, the sums over steps and questions;
  d_words_sk   sum_z (rho_s + (4 + Z) u) |att_s dc_k| + (e_dl_s + (4 + Z) u |dl_s|) |cc_k w_k|: cc w, two products, the sums;
  d_b          (57 + min(Z B, 64)) u sum |dl|.  The att error does NOT enter: the backward reads the att the forward wrote, and
               sum_s att'_s (da'_s - dot') = D - dot' A with D = sum att' da', |dot' - D| <= 10 u sum|att da| and |A - 1| <= 12 u,
               so at most 22 u sum|att da|; the products of dl (2), its sum (9) and the row sum (min(Z B, 64) + 2) are relative to
               sum|dl|.  sum|att da| <= 2 sum|dl| over the questions longer than one word is a property of the DATA, asserted on
               the CPU (test_word_attention_host.test_inputs_are_live); a one-word question gives att = 1 and dl = 0 exactly.
An entry whose bound is exactly zero (a padded word, a one-word question's dl) admits exactly zero.
Nothing here was fitted to a device: test_word_attention_host.py holds the constants from both sides -- an fp32 evaluation of the same
formulas in another summation order stays within HALF of every bound on every row, and six planted defects of a numpy restatement of
the kernels' loops each exceed one.  The counts are worst cases: both fp32 evaluations and the device use about a hundredth of each
bound on this data (profiles/word_attention_errors.txt: at most 0.011 on the device), so what the bounds still catch is exactly what
the planted defects show -- every one exceeds a bound by a factor of 19 or more.
"""
import collections
import math
import os

import numpy as np
import torch

from oracle import mac_oracle as mo

U = 2.0 ** -24
BIAS = 0.3
C_MAXS, CA_U, CB_MAXZ, SLAB = 256, 8, 32, 64
FAIR = 0.5
C_LOGIT, C_SOFT = 4, 16
OUTPUTS_FWD = ("att", "control")
OUTPUTS_BWD = ("d_cc", "d_words", "d_w", "d_b")
OUTPUTS = OUTPUTS_FWD + OUTPUTS_BWD


# ---------------------------------------------------------------------------------------------------------------------------
# the loop rules, restated
# ---------------------------------------------------------------------------------------------------------------------------
def al4(n):
    return (n + 3) & ~3


def ws_floats(B, S, d):
    """macx_control_attend_bwd_ws_floats: dl [B S], the d_w partials [B d], the d_b partials [B]"""
    return al4(B * S) + al4(B * d) + al4(B)


def route(S, d, p=1):
    """what the three kernels do with S words, d columns and p steps in one launch"""
    batch = 4 * CA_U
    t_last = (S - 1) // batch
    starts = [batch * t_last + wave for wave in range(4)]             # s0 of the four waves in the last trip
    passes = (S + SLAB - 1) // SLAB
    return dict(trips=(S + batch - 1) // batch,                       # trips of wave 0 (s0 = 0, 32, ..)
                idle_waves=max(0, 4 - S),                              # waves without a word at all
                idle_last=sum(1 for s0 in starts if s0 >= S),          # waves that do not enter the last trip
                reread=sum(1 for s0 in starts if s0 < S for u in range(CA_U) if s0 + 4 * u >= S),   # rows of the last trip clamped to S - 1
                passes=passes, last_pass=S - SLAB * (passes - 1),
                racc=(p + 3) // 4,                                     # Racc slots group 0 uses
                k256=(d + 255) // 256, k512=(d + 511) // 512, lanes_last=((d - 1) % 256) // 4 + 1,
                slabs=d // SLAB if d % SLAB == 0 else None)


def word_where(s):
    return "word %d (mod 32: %d, mod 64: %d, pass %d)" % (s, s % 32, s % 64, s // SLAB)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Row(collections.namedtuple("Row", "B S d lengths bwd reaches expect")):
    id = property(lambda r: "B%d-S%d-d%d" % (r.B, r.S, r.d))
    Z = 1
    recurrent = False


def _row(B, S, d, lengths, reaches, bwd=True, **expect):
    assert len(lengths) == B and lengths[0] == S and all(n in (1, S - 1, S, 32, 33, 64, 65) and n <= S for n in lengths[1:])
    return Row(B, S, d, tuple(lengths), bwd, reaches, expect)


# question 0 has length S; the others draw from {1, S - 1, 32, 33, 64, 65}, named here so that a boundary falls on and next to an edge
ROWS = [
    _row(1, 1, 64, [1], "one word: three idle waves, seven re-read rows, a slab pass of one word", trips=1, idle_waves=3, reread=7, idle_last=3,
         passes=1, last_pass=1, slabs=1),
    _row(3, 4, 128, [4, 1, 3], "one word per wave", trips=1, idle_waves=0, reread=28, idle_last=0),
    _row(3, 5, 128, [5, 4, 1], "wave 0's second word", trips=1, reread=27, idle_last=0),
    _row(3, 31, 128, [31, 30, 1], "one word short of a full batch: wave 3 re-reads word 30 once", trips=1, reread=1),
    _row(3, 32, 128, [32, 31, 1], "a full batch, nothing re-read", trips=1, reread=0),
    _row(3, 33, 128, [33, 32, 1], "the first second trip: wave 0 alone, seven rows re-read", trips=2, reread=7, idle_last=3),
    _row(3, 63, 256, [63, 33, 32], "two trips, one row short; one 64-word pass of 63", trips=2, reread=1, passes=1, last_pass=63, k256=1),
    _row(3, 64, 256, [64, 63, 33], "two full trips, one full pass", trips=2, reread=0, passes=1, last_pass=64),
    _row(3, 65, 256, [65, 64, 1], "a third trip and a second pass of one word", trips=3, reread=7, idle_last=3, passes=2, last_pass=1, slabs=4),
    _row(2, 65, 64, [65, 33], "d = 64: one slab, 16 of a wave's lanes hold columns, 32 threads in the control pass", passes=2,
         last_pass=1, slabs=1, k256=1, lanes_last=16),
    _row(2, 96, 320, [96, 65], "d = 320: a second 256-pass of 16 lanes, five slabs; three full trips", trips=3, reread=0, k256=2,
         lanes_last=16, slabs=5, passes=2, last_pass=32),
    _row(3, 127, 128, [127, 64, 65], "four trips, one row short; two passes, 63 in the last", trips=4, reread=1, passes=2, last_pass=63),
    _row(3, 128, 128, [128, 127, 33], "four full trips, two full passes", trips=4, reread=0, passes=2, last_pass=64),
    _row(3, 129, 128, [129, 128, 65], "a fifth trip of one word, a third pass of one word", trips=5, reread=7, idle_last=3, passes=3, last_pass=1),
    _row(2, 129, 576, [129, 64], "d = 576: a third 256-pass of 16 lanes, a second 512-pass of 32 threads, nine slabs", k256=3, k512=2,
         lanes_last=16, slabs=9, passes=3, last_pass=1),
    _row(2, 255, 128, [255, 254], "eight trips, one row short; four passes, 63 in the last", trips=8, reread=1, passes=4, last_pass=63),
    _row(2, 256, 128, [256, 65], "C_MAXS: eight full trips, four full passes, every thread of the softmax holds a word", trips=8,
         reread=0, passes=4, last_pass=64),
    _row(2, 33, 1024, [33, 32], "d = 1024: four 256-passes, two 512-passes, 16 slabs, past one batch", trips=2, k256=4, k512=2, slabs=16),
    _row(2, 256, 1024, [256, 255], "both maxima at once", trips=8, passes=4, k256=4, k512=2, slabs=16),
    _row(5, 65, 512, [65, 64, 33, 32, 1], "five questions, every boundary length; two full 256-passes, one 512-pass, eight slabs",
         passes=2, last_pass=1, k256=2, k512=1, slabs=8),
    _row(3, 33, 68, [33, 32, 1], "forward only, d % 4 == 0 alone: lane 16 holds the last four columns; the backward refuses d % 64",
         bwd=False, k256=1, lanes_last=17, slabs=None),
    _row(3, 65, 260, [65, 64, 33], "forward only: a second 256-pass of ONE lane; the backward refuses d % 64", bwd=False, k256=2,
         lanes_last=1, slabs=None),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
# padding content, a length of 0 and a length above S run on these two
PADDING_ROWS = [BY_ID["B3-S65-d256"], _row(2, 129, 128, [129, 65], "three passes, the last of one word; question 1 ends one word into the second",
                                           passes=3, last_pass=1, trips=5)]


class Multi(collections.namedtuple("Multi", "flags B S p d N recurrent draw reaches expect")):
    """a row of the cell table (2b); on the CPU the same (B, S, p, d) with drawn cc / d_control / g_att per step drives the restated loops.
    draw: which draw of the cell's inputs the row runs on (cell_seed; chosen on the CPU alone, see cell_fairness)"""
    id = property(lambda r: "%s-B%d-S%d-p%d-d%d" % (r.flags, r.B, r.S, r.p, r.d))
    Z = property(lambda r: r.p)
    bwd = True
    lengths = property(lambda r: cell_lengths(r))


def _multi(flags, B, S, p, reaches, d=128, N=9, draw=0, **expect):
    return Multi(flags, B, S, p, d, N, flags == "args1", draw, reaches, expect)


# draw: the first draw of the row's inputs that is fair to the finer metrics (cell_fairness); d = 512 holds 512 entries of ctrlLogits_w's
# gradient, and few draws keep every one of them above 2^-8 of the largest
CELL_ROWS = [
    _multi("args", 3, 33, 4, "grid (3, 4): a second trip in every step, Racc[0] in all four groups", trips=2, racc=1, passes=1),
    _multi("args", 2, 64, 8, "Racc[1] in every group, one full pass", draw=5, racc=2, passes=1, last_pass=64),
    _multi("args", 2, 65, 5, "a second pass with i = 1 live in group 0 alone", racc=2, passes=2, last_pass=1),
    _multi("args", 2, 65, 9, "Racc[2] across two passes", draw=2, racc=3, passes=2, last_pass=1),
    _multi("args", 2, 129, 32, "CB_MAXZ: all eight Racc slots of every group across three passes, the last of one word", draw=1, racc=8, passes=3,
           last_pass=1, trips=5),
    _multi("args", 2, 256, 7, "C_MAXS with two Racc slots across four passes", draw=2, racc=2, passes=4, trips=8),
    _multi("args", 2, 65, 5, "d = 512: eight slabs, two passes, two Racc slots", d=512, N=20, draw=713, racc=2, passes=2, slabs=8, k256=2),
    _multi("args1", 2, 65, 3, "recurrent control: three accumulating launch pairs of nz = 1 over two passes", draw=1, racc=1, passes=2, last_pass=1),
    _multi("args1", 2, 130, 5, "recurrent control: five accumulating launch pairs over three passes, two words in the last", draw=14, racc=1,
           passes=3, last_pass=2),
    _multi("args3", 2, 65, 5, "self attention: d_control of every step arrives through the write unit too", draw=6, racc=2, passes=2),
    _multi("args4", 2, 129, 3, "memory gate; three passes, the last of one word", racc=1, passes=3, last_pass=1),
]
assert len({r.id for r in CELL_ROWS}) == len(CELL_ROWS)


def cell_seed(r):
    return 4000 + 97 * r.S + 7 * r.p + r.d // 64 + (11 if r.recurrent else 0) + {"args": 0, "args1": 1, "args3": 3, "args4": 4}[r.flags] + 1000 * r.draw


def cell_inputs(r):
    """(cfg, vq, words, lengths, kb) as tests/helpers.make_case draws them (padded words zero, question 0 of length S)"""
    from helpers import make_case
    return make_case(r.flags, r.B, r.S, r.N, r.d, r.p, seed=cell_seed(r))


def cell_targets(p):
    """the loss of the cell rows: the final state, every att_question map (g_att live at every step) and the controls history"""
    return [("att_question", i) for i in range(p)] + [("controls", None), ("memory", None), ("control", None)]


def cell_params(macx, cfg, p, gen_seed=5):
    """the parameters tests/test_gpu_state_grads._build draws (non-zero biases), on the host"""
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(gen_seed))
    g = torch.Generator().manual_seed(gen_seed + 1)
    with torch.no_grad():
        for f in params.fields:
            t = getattr(params, f)
            if f.endswith("_b"):
                t.copy_((torch.rand(t.shape, generator=g) - 0.5) * 0.2)
    return params


def cell_reference(macx, r, ref_params=None, seed=5, dtype=torch.float64):
    """state_grads_ref.oracle_aux of row r in training mode under the hashed masks of `seed`: the oracle's forward and every gradient,
    in fp64 (the reference) or in `dtype` (fp32: what cell_fairness measures)"""
    import state_grads_ref as sr
    cfg, vq, words, lengths, kb = cell_inputs(r)
    if ref_params is None:
        ref_params = cell_params(macx, cfg, r.p).to_reference_dict()
    Gs = sr.incoming(cell_targets(r.p), r.B, r.S, r.N, r.d, r.p)
    if dtype is torch.float64:
        ref = sr.oracle_aux(cfg, ref_params, vq, words, lengths, kb, Gs, train=True, seed=seed)
    else:
        params = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in ref_params.items()}
        vs = mo.VarStore(params=params, dtype=dtype)
        ins = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (vq, words, kb)]
        keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout)
        c, m, cell = mo.mac_network(cfg, vs, ins[0], ins[1], ins[1], lengths.cpu(), ins[2], train=True, mask_fn=mo.hash_mask_fn(seed, keeps),
                                    keeps=keeps)
        sr.aux_loss(cell, sr._State(c, m), Gs, lambda G: G.to(dtype)).backward()
        ref = dict(control=c, memory=m, cell=cell, params=params, inputs=tuple(ins))
    ref["Gs"] = Gs
    return ref


CTRL_W = "MACnetwork/MACCell/control/inter2logits/linearLayerlogits/weights/weight"
W_FLOOR = 2.0 ** -8


def per_row_err(got, ref):
    """largest |got - ref| of each row (last axis) over that row's largest |ref|; an exactly zero reference row admits exactly zero"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err, scale = (got - ref).abs().amax(-1), ref.abs().amax(-1)
    q = err / scale.clamp_min(1e-300)
    return torch.where(scale > 0, q, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def cell_fairness(macx, r):
    """The finer metrics of 2b on the CPU: {"d_words", "d_vecQuestions", "ctrlLogits_w"}: the fp32 oracle's largest per-word, per-question
    and per-column error against the fp64 oracle, and "floor": the smallest |entry| of the reference ctrlLogits_w gradient over its
    largest.  ctrlLogits_w is a vector, so "per column" divides an entry's error by the entry itself, and an entry the sum over steps,
    questions and words nearly cancels has a relative error of its condition number times 2^-24 in ANY fp32 arithmetic.  An fp32
    evaluation leaves every entry an absolute error of a few 2^-24 of the tensor's largest (the fp32 oracle: at most 5 over these rows);
    GRAD_TOL = 2e-4 = 3355 x 2^-24 of an entry admits 13 x 2^-24 of the largest where the entry is at least 2^-8 of it.  A row runs on the
    FIRST draw of its inputs (cell_seed, draw = 0, 1, ..) whose reference keeps floor >= W_FLOOR = 2^-8 and whose fp32 oracle keeps all
    three figures within half of GRAD_TOL (first_fair_draw; the host file asserts it for the draw recorded).  The data changes, never
    the bound, and nothing of the choice depends on the library."""
    a, b = cell_reference(macx, r), cell_reference(macx, r, dtype=torch.float32)
    w = a["params"][CTRL_W].grad
    return dict(d_words=float(per_row_err(b["inputs"][1].grad, a["inputs"][1].grad).max()),
                d_vecQuestions=float(per_row_err(b["inputs"][0].grad, a["inputs"][0].grad).max()),
                ctrlLogits_w=float(per_row_err(b["params"][CTRL_W].grad.reshape(-1, 1), w.reshape(-1, 1)).max()),
                floor=float(w.abs().min() / w.abs().max()))


def cell_is_fair(f, tol):
    return f["floor"] >= W_FLOOR and all(f[k] <= 0.5 * tol for k in ("d_words", "d_vecQuestions", "ctrlLogits_w"))


def first_fair_draw(macx, r, tol=2e-4, limit=2000):
    for k in range(limit):
        if cell_is_fair(cell_fairness(macx, r._replace(draw=k)), tol):
            return k
    raise ValueError(r.id)


def cell_lengths(r):
    return tuple(int(n) for n in mo.synthetic_inputs(r.B, r.S, 1, r.d, seed=cell_seed(r))[2])


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
Data = collections.namedtuple("Data", "cc dc words w bias lengths g_att")      # [Z,B,d] [Z,B,d] [B,S,d] [d] float [B] [Z,B,S] | None


def make_data(r, lengths=None, seed=0):
    """cc ~ N(0, 1), words ~ U(-1, 1), w ~ N(0, 1) / sqrt(d), bias 0.3, d_control ~ N(0, 1) (and g_att ~ N(0, 1) for a multi-step row),
    fp32, from a generator keyed on the row.  Padded words keep their draw."""
    g = torch.Generator().manual_seed(100000 + 1000 * r.S + 10 * r.d + r.B + 7919 * r.Z + seed)
    Z = r.Z
    cc = torch.randn(Z, r.B, r.d, generator=g)
    words = torch.rand(r.B, r.S, r.d, generator=g) * 2 - 1
    w = torch.randn(r.d, generator=g) / r.d ** 0.5
    dc = torch.randn(Z, r.B, r.d, generator=g)
    g_att = torch.randn(Z, r.B, r.S, generator=g) if Z > 1 else None
    L = torch.tensor(list(r.lengths if lengths is None else lengths), dtype=torch.int32)
    return Data(cc, dc, words, w, BIAS, L, g_att)


def zero_padding(data):
    words = data.words.clone()
    for b, n in enumerate(data.lengths.tolist()):
        words[b, max(0, min(n, words.shape[1])):] = 0.0
    return data._replace(words=words)


def fill_padding(data, lim=100.0, seed=5):
    """the words past each length drawn from U(-lim, lim): finite content that must not reach any output"""
    g = torch.Generator().manual_seed(seed)
    words = data.words.clone()
    for b, n in enumerate(data.lengths.tolist()):
        n = max(0, min(n, words.shape[1]))
        words[b, n:] = (torch.rand(words.shape[1] - n, words.shape[2], generator=g) * 2 - 1) * lim
    return data._replace(words=words)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: a plain fp64 restatement and torch's backward of it
# ---------------------------------------------------------------------------------------------------------------------------
def forward_fp64(cc, words, w, b, lengths):
    """mac_cell.py:153-181 for one step in the operands' dtype: logits ((cc words) w).sum + b, expMask, softmax, att2Smry"""
    logits = ((cc.unsqueeze(1) * words) * w).sum(-1) + b
    att = torch.softmax(mo.Ops.expMask(logits, lengths), dim=-1)
    return att, mo.Ops.att2Smry(att, words)


def reference(data):
    """{"att" [Z,B,S], "control" [Z,B,d], "d_cc" [Z,B,d], "d_words" [B,S,d], "d_w" [d], "d_b" []} in fp64; the loss is
    sum_z (control_z d_control_z).sum() (+ (att_z g_att_z).sum())"""
    dt = torch.float64
    cc, words, w = [t.to(dt).clone().requires_grad_(True) for t in (data.cc, data.words, data.w)]
    b = torch.tensor(data.bias, dtype=dt, requires_grad=True)
    atts, ctls, loss = [], [], 0
    for z in range(cc.shape[0]):
        att, ctl = forward_fp64(cc[z], words, w, b, data.lengths)
        loss = loss + (ctl * data.dc[z].to(dt)).sum()
        if data.g_att is not None:
            loss = loss + (att * data.g_att[z].to(dt)).sum()
        atts.append(att)
        ctls.append(ctl)
    loss.backward()
    return dict(att=torch.stack(atts).detach(), control=torch.stack(ctls).detach(), d_cc=cc.grad, d_words=words.grad, d_w=w.grad, d_b=b.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds (module docstring)
# ---------------------------------------------------------------------------------------------------------------------------
def _np64(t):
    return t.detach().cpu().double().numpy()


def terms(data):
    """the fp64 intermediates the bounds are made of"""
    cc, dc, words, w = [_np64(t) for t in (data.cc, data.dc, data.words, data.w)]
    Z, B, d = cc.shape
    S = words.shape[1]
    L = data.lengths.numpy().astype(np.int64)
    live = np.arange(S)[None, :] < L[:, None]
    ccw = cc * w
    absT = np.einsum("zbk,bsk->zbs", np.abs(ccw), np.abs(words)) + abs(data.bias)
    logits = np.einsum("zbk,bsk->zbs", ccw, words) + data.bias
    masked = logits + (1.0 - live[None]) * (-1e30)
    m = masked.max(-1, keepdims=True)
    e = np.exp(masked - m)
    att = e / e.sum(-1, keepdims=True)
    g = 0.0 if data.g_att is None else _np64(data.g_att)
    da = np.einsum("zbk,bsk->zbs", dc, words) + g
    abs_da = np.einsum("zbk,bsk->zbs", np.abs(dc), np.abs(words)) + np.abs(g)
    dot = (att * da).sum(-1, keepdims=True)
    dl = att * (da - dot)
    return dict(Z=Z, B=B, S=S, d=d, L=L, live=live, cc=cc, dc=dc, words=words, w=w, ccw=ccw, absT=absT, spread=np.abs(masked - m), att=att,
                da=da, abs_da=abs_da, dot=dot, dl=dl)


def bounds(data, t=None):
    """{output: array of per-element bounds} (module docstring)"""
    t = t or terms(data)
    Z, B, S, d, att, dl, aw = t["Z"], t["B"], t["S"], t["d"], t["att"], t["dl"], np.abs(t["words"])
    E = (d + C_LOGIT) * U * t["absT"]
    rho = E + (att * E).sum(-1, keepdims=True) + (np.where(att > 0, t["spread"], 0.0) + C_SOFT) * U
    out = dict(att=att * rho)
    out["control"] = np.einsum("zbs,bsk->zbk", att * (rho + (S + 1) * U), aw)
    e_da = (4 * (-(-d // 256)) + 8) * U * t["abs_da"]
    e_dot = (np.abs(att * t["da"]) * (rho + 10 * U)).sum(-1, keepdims=True) + (att * e_da).sum(-1, keepdims=True)
    e_dl = (rho + 2 * U) * np.abs(dl) + att * (e_da + e_dot)
    out["d_cc"] = np.abs(t["w"]) * np.einsum("zbs,bsk->zbk", e_dl + (S + 2) * U * np.abs(dl), aw)
    out["d_w"] = (np.abs(t["cc"]) * np.einsum("zbs,bsk->zbk", e_dl + (S + 2 + B + Z) * U * np.abs(dl), aw)).sum((0, 1))
    out["d_words"] = (np.einsum("zbs,zbk->bsk", att * (rho + (4 + Z) * U), np.abs(t["dc"])) +
                      np.einsum("zbs,zbk->bsk", e_dl + (4 + Z) * U * np.abs(dl), np.abs(t["ccw"])))
    out["d_b"] = np.asarray((57 + min(Z * B, 64)) * U * np.abs(dl).sum())
    return out


def db_condition(t):
    """(sum |att da|, sum |dl|) over the questions longer than one word: the data property d_b's constant rests on"""
    many = t["L"] != 1
    return float(np.abs(t["att"] * t["da"])[:, many].sum()), float(np.abs(t["dl"])[:, many].sum())


def ratios(got, ref, bnd, outputs=OUTPUTS):
    """{output: (largest error / bound, where)}; an element whose bound is exactly zero admits exactly zero (else inf).  got, ref: torch
    tensors or arrays in reference()'s shapes (a leading step axis may be missing for Z = 1)"""
    res = {}
    for k in outputs:
        g = np.asarray(_np64(got[k]) if torch.is_tensor(got[k]) else got[k], dtype=np.float64).reshape(bnd[k].shape)
        r = _np64(ref[k]).reshape(bnd[k].shape) if torch.is_tensor(ref[k]) else np.asarray(ref[k], dtype=np.float64).reshape(bnd[k].shape)
        err = np.abs(g - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(bnd[k] > 0, err / np.where(bnd[k] > 0, bnd[k], 1.0), np.where(err > 0, np.inf, 0.0))
        q = np.where(np.isfinite(g), q, np.inf)
        i = np.unravel_index(int(np.argmax(q)), q.shape) if q.ndim else ()
        res[k] = (float(q.max()), _where(k, i))
    return res


def _where(k, i):
    if k == "att":
        return "step %d question %d %s" % (i[0], i[1], word_where(i[2]))
    if k in ("control", "d_cc"):
        return "step %d question %d column %d (256-pass %d, slab %d)" % (i[0], i[1], i[2], i[2] // 256, i[2] // SLAB)
    if k == "d_words":
        return "question %d %s column %d (slab %d)" % (i[0], word_where(i[1]), i[2], i[2] // SLAB)
    if k == "d_w":
        return "column %d (slab %d)" % (i[0], i[0] // SLAB)
    return "-"


def line(r, what, res):
    return "%-22s %-8s " % (r.id, what) + " ".join("%s %.3f" % (k, v[0]) for k, v in res.items())


def log(text):
    """append to the file MACX_WORD_ATTENTION_LOG names (how profiles/word_attention_errors.txt is recorded); always printed (-s)"""
    print(text)
    path = os.environ.get("MACX_WORD_ATTENTION_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(text + "\n")


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 in another order (fairness): plain np.sum over d and over S, steps summed last
# ---------------------------------------------------------------------------------------------------------------------------
def _np32(t):
    return t.detach().cpu().float().numpy()


def eval_fp32(data):
    f = np.float32
    cc, dc, words, w = [_np32(t) for t in (data.cc, data.dc, data.words, data.w)]
    S = words.shape[1]
    live = (np.arange(S)[None, :] < data.lengths.numpy()[:, None])
    logits = ((cc[:, :, None, :] * words[None]) * w).sum(-1, dtype=f) + f(data.bias)
    masked = logits + (f(1) - live[None].astype(f)) * f(-1e30)
    e = np.exp(masked - masked.max(-1, keepdims=True))
    att = e / e.sum(-1, keepdims=True, dtype=f)
    control = (att[..., None] * words[None]).sum(2, dtype=f)
    da = (dc[:, :, None, :] * words[None]).sum(-1, dtype=f)
    if data.g_att is not None:
        da = da + _np32(data.g_att)
    dot = (att * da).sum(-1, keepdims=True, dtype=f)
    dl = att * (da - dot)
    R = (dl[..., None] * words[None]).sum(2, dtype=f)
    d_words = (att[..., None] * dc[:, :, None, :] + dl[..., None] * (cc * w)[:, :, None, :]).sum(0, dtype=f)
    out = dict(att=att, control=control, d_cc=R * w, d_words=d_words, d_w=(cc * R).sum(1, dtype=f).sum(0, dtype=f),
               d_b=dl.sum(-1, dtype=f).sum(-1, dtype=f).sum(0, dtype=f))
    assert all(v.dtype == f for v in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' loops in numpy fp32, with the defects of the sharpness proof
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "a": "a word with s >= 32 reads word s - 1 in the logit pass",
    "b": "the last word of question 0 is dropped from the softmax sum",
    "c": "the second 64-word pass is left out of R",
    "d": "step 4 is missing from the d_words sum of question 0's last word",
    "e": "question 0 is missing from d_w",
    "f": "the recurrent form overwrites d_words at its last launch",
}


def defect_is_live(name, r):
    return {"a": r.S >= 33, "b": r.S >= 2, "c": r.S >= 65 and r.bwd, "d": r.Z >= 5 and not r.recurrent and r.bwd, "e": r.B >= 2 and r.bwd,
            "f": r.recurrent and r.Z >= 2}[name]


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1; lane 0's value"""
    v = v.astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., np.arange(64) ^ o]
    return v[..., 0]


def _block_sum(v):
    """a per-thread value of the 256 threads (last axis, zero where the thread holds nothing) -> (r0 + r1) + (r2 + r3)"""
    r = _butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def _fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64, one rounding of the sum to fp64 and one to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lane_dot(x, y, w=None):
    """[.., d] -> the logit / da pass: a lane adds ((p0 + p1) + p2) + p3 of its four columns to its part per pass of 256, then wave_sum"""
    d = x.shape[-1]
    dp = -(-d // 256) * 256
    prod = x * y if w is None else (x * y) * w
    prod = np.concatenate([prod, np.zeros(prod.shape[:-1] + (dp - d,), np.float32)], -1).reshape(prod.shape[:-1] + (dp // 256, 64, 4))
    part = np.zeros(prod.shape[:-3] + (64,), np.float32)
    for j in range(dp // 256):
        q = prod[..., j, :, :]
        part = part + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
    return _butterfly(part)


def _pad256(v):
    return np.concatenate([v, np.zeros(v.shape[:-1] + (256 - v.shape[-1],), np.float32)], -1)


def kernel_forward(data, defect=None):
    """control_attend_kernel per (question, step) -> att [Z,B,S], control [Z,B,d]"""
    f = np.float32
    cc, words, w = [_np32(t) for t in (data.cc, data.words, data.w)]
    Z, B, d = cc.shape
    S = words.shape[1]
    L = data.lengths.numpy()
    src = np.arange(S)
    if defect == "a":
        src = np.where(src >= 32, src - 1, src)
    logits = _lane_dot(cc[:, :, None, :], words[None][:, :, src, :], w) + f(data.bias)
    masked = logits + np.where(np.arange(S)[None, :] < L[:, None], f(0), f(1))[None] * f(-1e30)
    m = masked.max(-1, keepdims=True)
    e = np.exp(masked - m)
    e_sum = e.copy()
    if defect == "b":
        e_sum[:, 0, max(0, min(int(L[0]), S) - 1)] = 0
    inv = f(1) / _block_sum(_pad256(e_sum))
    att = e * inv[..., None]
    control = np.zeros((Z, B, d), f)
    for s in range(S):
        control = _fma(att[:, :, s, None], words[None, :, s, :], control)
    return att, control


def _backward_launch(att, cc, dc, words, w, g_att, d_words, dw_part, acc, defect):
    """one launch pair over the steps of its arguments -> d_cc [nz,B,d], db partials [nz,B]; d_words and dw_part written or added to"""
    f = np.float32
    nz, B, d = cc.shape
    S = words.shape[1]
    da = _lane_dot(dc[:, :, None, :], words[None])
    if g_att is not None:
        da = da + g_att
    dot = _block_sum(_pad256(att * da))[..., None]
    dl = att * (da - dot)
    db = _block_sum(_pad256(dl))
    ccw = cc * w
    R = np.zeros((nz, B, d), f)
    for s in range(S):
        if defect == "c" and 64 <= s < 128:
            continue
        R = _fma(dl[:, :, s, None], words[None, :, s, :], R)
    v = np.zeros((B, S, d), f)
    for z in range(nz):
        term = att[z][..., None] * dc[z][:, None, :] + dl[z][..., None] * ccw[z][:, None, :]
        if defect == "d" and z == 4:
            term[0, S - 1] = 0
        v = v + term
    d_words[...] = d_words + v if acc else v
    groups = np.zeros((4, B, d), f)
    for z in range(nz):
        groups[z % 4] = groups[z % 4] + cc[z] * R[z]
    t = (groups[0] + groups[1]) + (groups[2] + groups[3])
    dw_part[...] = dw_part + t if acc else t
    return R * w, db


def kernel_backward(data, att, defect=None, recurrent=False):
    """control_bwd_dl_kernel + control_bwd_apply_kernel + the row sums, from the att the forward wrote: one launch pair over all steps,
    or (recurrent) one per step from the last to the first, accumulating into a zeroed d_words / d_w partial"""
    f = np.float32
    cc, dc, words, w = [_np32(t) for t in (data.cc, data.dc, data.words, data.w)]
    g = None if data.g_att is None else _np32(data.g_att)
    Z, B, d = cc.shape
    S = words.shape[1]
    d_words, dw_part = np.zeros((B, S, d), f), np.zeros((B, d), f)
    if recurrent:
        d_cc, db = np.zeros((Z, B, d), f), np.zeros((Z, B), f)
        for z in reversed(range(Z)):
            acc = not (defect == "f" and z == 0)
            d_cc[z:z + 1], db[z:z + 1] = _backward_launch(att[z:z + 1], cc[z:z + 1], dc[z:z + 1], words, w, None if g is None else g[z:z + 1],
                                                          d_words, dw_part, acc, defect)
    else:
        d_cc, db = _backward_launch(att, cc, dc, words, w, g, d_words, dw_part, False, defect)
    d_w = np.zeros(d, f)
    for b in range(1 if defect == "e" else 0, B):
        d_w = d_w + dw_part[b]
    d_b = f(0)
    for x in db.reshape(-1):
        d_b = d_b + x
    return dict(d_cc=d_cc, d_words=d_words, d_w=d_w, d_b=np.asarray(d_b))


def kernel_restatement(data, defect=None, recurrent=False, bwd=True):
    att, control = kernel_forward(data, defect)
    out = dict(att=att, control=control)
    if bwd:
        out.update(kernel_backward(data, att, defect, recurrent))
    return out
