"""The answer side (macx.OutputClassifier on macx_output_forward_w / _backward_w, the generic classifier, macx_answer_loss and its
weighted twin) at real vocabulary and batch sizes: case table, data, metrics.  No device.

Shared by tests/test_gpu_output_geometry.py (the kernels) and tests/test_output_geometry_host.py (CPU: the restatement below against the
oracle, the table's claims against restated launch rules, the inputs' fairness under the finer metrics, the size calls).

Launch rules of the fused unit (mac-network_amd/csrc/macx_api.hip "output unit + classifier", macx_small.hip.h), restated below:
  * every linear runs on small_linear_kernel<1> (16-row tiles) while rows <= 128 and on small_linear_kernel<4> (64-row tiles) above;
    a tile's four waves take interleaved 16-wide k groups, 512 k per pass;
  * fc_1 runs on the answer axis padded to Ap = pad16(A): the forward pack of fc1_W zero-fills columns A .. Ap (n_src = A < Nout = Ap),
    the transposed backward pack zero-fills k (k_src = A < K = Ap), with 16-byte loads iff A % 4 == 0;
  * crop_cols / add_bias / pad_cols launch 16 x 256 threads over B A (B Ap) elements, drop2 64 x 256 over B 2d / B hidden,
    outer_sum 64 x 256 over hidden A outputs (512 x 256 over 2d hidden, 256 x 256 over d d);
  * rowsum: 64 row groups; row group rg adds rows rg, rg + 128, ... into s0 and rg + 64, rg + 192, ... into s1;
  * the dropout index (b0 + r) * width + j is taken modulo 2^32 (oracle.dropout_hash.mask_for wraps the same way).

GRAD_TOL.  The ceiling is the project's 1e-4 (tests/test_gpu_output.py), and it is the figure used.  It was taken from the fp32
restatement of the same expressions on the CPU (test_output_geometry_host.test_fp32_restatement_is_within_a_third_of_every_bound) over
every case and mode of the table: at most 3e-6 per question, column, row and bias element wherever B >= 16 (7e-6 at B = 5, 1.1e-5 at
B = 3 with d = 512 into hidden = 16), but 2.7e-5 per row of fc1_W's gradient, 2.3e-5 per row of fc0_W's and 1.5e-5 for outQuestion_b at
B = 3, d = hidden = 1024 -- three questions under dropout leave columns whose only live entry is a nearly cancelled 1024-term sum, and
there a relative figure is the sum's condition number times 2^-24 in ANY fp32 arithmetic.  Three times the worst measurement is 8.1e-5;
the ceiling is the round figure above it.
Data seeds.  Every case draws from seed 2 except four whose draw at seed 2 is ill-conditioned in that sense (fp32 restatement above a
third of a bound: 0.56 at A = 1848, 0.45 at B = 1, 0.38 at d = 1024, 0.60 at d = 512 into hidden = 16); each takes the FIRST seed from 2
upwards at which the restatement meets the third (3, 4, 5, 3).  The data changes, never the bound; nothing of it depends on the library.
Observed on the device: profiles/output_geometry_errors.txt (at most 0.24 of a bound; the fp32 restatement 0.29).
"""
import collections
import math
import os

import torch

from oracle import dropout_hash as dh

SEED = 9                      # dropout seed (sites 7 / 8), as test_gpu_output.test_classifier_matches_oracle
B0 = 4
LOGIT_TOL = 2e-5              # largest absolute logit error (tests/test_gpu_output.py)
GRAD_TOL = 1e-4               # every gradient figure below (see the module docstring)
FAIR = 1.0 / 3.0              # the fp32 restatement's share of a bound
PEAK = 2.0                    # standard deviation fc1_W is scaled to give the logits: a peaked softmax
WORD = 0x9E3779B9             # the non-zero mask word of the `-word` case


# ---------------------------------------------------------------------------------------------------------------------------
# the launch rules, restated
# ---------------------------------------------------------------------------------------------------------------------------
def pad16(n):
    return (n + 15) & ~15


def al4(n):
    return (n + 3) & ~3


def tile_rows(rows):
    """small_linear_launch: rows per tile"""
    return 16 if rows <= 128 else 64


def k_passes(k):
    """small_linear_tile: passes of 512 k"""
    return (k + 511) // 512


def idle_waves(k):
    """waves of a tile without a 16-wide k group in a reduction of depth k"""
    return max(0, 4 - k // 16)


def grid_passes(n, blocks, threads=256):
    """passes of a grid-stride loop over n elements"""
    return (n + blocks * threads - 1) // (blocks * threads)


def t_pack(A):
    """the transposed pack of fc1_W (k = answers): (16-byte loads?, zero-tail groups k0 >= A, groups cut by A)"""
    vec4 = A % 4 == 0
    groups = pad16(A) // 4
    tail = sum(1 for g in range(groups) if 4 * g >= A)
    cut = sum(1 for g in range(groups) if 4 * g < A < 4 * g + 4)
    return vec4, tail, cut


def rowsum_loop(rows):
    """rowsum_kernel, row group 0: (iterations of the two-accumulator loop, whether the tail row is added, row groups whose s1 is used)"""
    r, it = 0, 0
    while r + 64 < rows:
        it, r = it + 1, r + 128
    return it, r < rows, max(0, min(64, rows - 64))


def saved_floats(B, d, H, A):
    """OutLayout (macx_api.hip), as include/macx.h documents the unit: three packed weights, eq, x0, h, x1, padded logits"""
    Ap = pad16(A)
    return sum(al4(n) for n in (d * d, 2 * d * H, H * Ap, B * d, B * 2 * d, B * H, B * H, B * Ap))


def ws_floats(B, d, H, A):
    """OutBwdLayout: three transposed packs, padded d_logits, dx1, dh, dx0, deq"""
    Ap = pad16(A)
    return sum(al4(n) for n in (d * d, H * 2 * d, Ap * H, B * Ap, B * H, B * H, B * 2 * d, B * d))


def route(c):
    """what the library does with case c"""
    A, Ap = c.A, pad16(c.A)
    vec4, tail, cut = t_pack(A)
    it, tailrow, s1 = rowsum_loop(c.B)
    wraps = lambda width: (c.b0 * width) >> 32 != ((c.b0 + c.B) * width - 1) >> 32
    crosses = lambda width: (c.b0 * width) % (1 << 32) < (1 << 31) <= ((c.b0 + c.B) * width - 1) % (1 << 32) and not wraps(width)
    return dict(tile=tile_rows(c.B), tiles=(c.B + tile_rows(c.B) - 1) // tile_rows(c.B), last_tile_rows=(c.B - 1) % tile_rows(c.B) + 1,
                Ap=Ap, zero_cols=Ap - A, col_tiles=Ap // 16, vec4=vec4, zero_tail=tail, cut_groups=cut,
                crop_passes=grid_passes(c.B * A, 16), pad_passes=grid_passes(c.B * Ap, 16), second_pass=c.B * A > 4096,
                outer1_passes=grid_passes(c.H * A, 64), drop0_passes=grid_passes(c.B * 2 * c.d, 64),
                rowsum_iters=it, rowsum_tail=tailrow, rowsum_s1=s1,
                k_passes=k_passes(2 * c.d), idle_waves=max(idle_waves(c.d), idle_waves(c.H)),
                wrap0=wraps(2 * c.d), wrap1=wraps(c.H), cross0=crosses(2 * c.d))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "id B d H A b0 keep1 word cot seed reaches expect")):
    """keep1: the case also runs at keep = 1 (evaluation masks, same backward pass); word: the run's mask word; cot: "ce" (d_logits of the
    mean cross-entropy over drawn answers) | "randn"; expect: the entries of route(c) the row exists for"""
    modes = property(lambda c: (True, False) if c.keep1 else (True,))


def _case(B, d, H, A, reaches, b0=B0, keep1=False, word=0, cot="ce", tag="", seed=2, **expect):
    cid = "B%d-d%d-h%d-A%d%s" % (B, d, H, A, tag)
    return Case(cid, B, d, H, A, b0, keep1, word, cot, seed, reaches, expect)


def _cases():
    out = []
    # ---- the answers axis
    S = (5, 64, 48)
    out.append(_case(*S, 1, "A = 1: 15 zero columns; the loss gradient of one answer is exactly zero, so the cotangent is randn",
                     cot="randn", Ap=16, zero_cols=15, vec4=False, zero_tail=3, cut_groups=1))
    out.append(_case(*S, 15, "A = 15: one column short of the 16-column tile, scalar transposed pack", Ap=16, zero_cols=1, vec4=False, cut_groups=1))
    out.append(_case(*S, 16, "A = 16: no padding at all", Ap=16, zero_cols=0, vec4=True, zero_tail=0, cut_groups=0))
    out.append(_case(*S, 17, "A = 17: one column into a second tile", Ap=32, zero_cols=15, col_tiles=2, vec4=False, zero_tail=3))
    out.append(_case(65, 64, 48, 1845, "A = 1845 (the GQA vocabulary): 116 column tiles on the scalar pack; B A = 119,925: 30 passes of crop_cols; "
                     "outer_sum over 88,560 outputs: 6 passes", keep1=True, Ap=1856, col_tiles=116, vec4=False, crop_passes=30, second_pass=True,
                     outer1_passes=6, rowsum_s1=1))
    out.append(_case(*S, 1848, "A = 1848: 16-byte transposed pack with a zero tail (A % 16 == 8)", seed=3, Ap=1856, vec4=True, zero_tail=2, cut_groups=0,
                     second_pass=True))
    out.append(_case(64, 512, 512, 3129, "A = 3129 (the VQA vocabulary): outer_sum over 1.6 M outputs, 98 grid passes", Ap=3136,
                     outer1_passes=98, second_pass=True))
    # ---- the batch axis
    for B, why, kw in (
            (1, "one question", dict(tile=16, tiles=1, last_tile_rows=1)),
            (16, "the last row of a 16-row tile", dict(tile=16, tiles=1, last_tile_rows=16)),
            (17, "one row into a second 16-row tile", dict(tile=16, tiles=2, last_tile_rows=1)),
            (64, "rowsum: every row group holds one row, no s1", dict(rowsum_iters=0, rowsum_tail=True, rowsum_s1=0)),
            (65, "rowsum's second register: row 64 is the only one in s1", dict(rowsum_iters=1, rowsum_tail=False, rowsum_s1=1)),
            (128, "the last batch on 16-row tiles (8 of them); s1 in every row group", dict(tile=16, tiles=8, rowsum_s1=64, rowsum_tail=False)),
            (129, "the first batch on 64-row tiles, the last tile of one row; rowsum's tail row after one iteration",
             dict(tile=64, tiles=3, last_tile_rows=1, rowsum_iters=1, rowsum_tail=True)),
            (192, "three full 64-row tiles; one iteration and a tail row in every row group", dict(tile=64, tiles=3, last_tile_rows=64, rowsum_iters=1)),
            (193, "rowsum's second iteration (row 192 into s1)", dict(tile=64, tiles=4, last_tile_rows=1, rowsum_iters=2, rowsum_tail=False)),
            (256, "four full 64-row tiles, two full rowsum iterations", dict(tile=64, tiles=4, rowsum_iters=2, rowsum_tail=False, second_pass=True))):
        out.append(_case(B, 64, 32, 33, "B = %d: %s" % (B, why), keep1=B in (65, 129), seed=4 if B == 1 else 2, **kw))
    # ---- the width axis
    out.append(_case(3, 16, 16, 28, "d = hidden = 16 (out_check's minima): 16-deep reductions, three of a tile's four waves idle", keep1=True,
                     idle_waves=3, k_passes=1))
    out.append(_case(3, 1024, 1024, 28, "d = hidden = 1024: in = 2048, four 512-k passes of small_linear_tile", seed=5, k_passes=4, idle_waves=0))
    out.append(_case(3, 512, 16, 28, "d = 512 into hidden = 16: a 1024-deep reduction into one column tile, a 16-deep one behind it",
                     seed=3, k_passes=2, idle_waves=3))
    # ---- the GQA training shape
    out.append(_case(128, 512, 512, 1845, "the GQA training shape (configs[2]'s batch): 58 passes of crop_cols, 58 of outer_sum", keep1=True,
                     tile=16, tiles=8, Ap=1856, crop_passes=58, outer1_passes=58, rowsum_s1=64))
    # ---- the 32-bit wrap of the dropout index (b0 + r) * width + j
    W = (5, 64, 48, 17)
    out.append(_case(*W, "b0 = 2^25 - 2: layer 0's index (width 128) wraps past 2^32 at the third question", b0=(1 << 25) - 2, tag="-wrap",
                     wrap0=True, wrap1=False))
    out.append(_case(*W, "b0 = 2^24 - 2: layer 0's index crosses 2^31 at the third question", b0=(1 << 24) - 2, tag="-cross", cross0=True, wrap0=False))
    out.append(_case(*W, "b0 = 2^25 - 2 under a non-zero mask word", b0=(1 << 25) - 2, word=WORD, tag="-word", wrap0=True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
FIELDS = ("outQuestion_W", "outQuestion_b", "fc0_W", "fc0_b", "fc1_W", "fc1_b")
PRE = {"outQuestion_b": "eq", "fc0_b": "pre0", "fc1_b": "logits"}      # the pre-activation tensor each bias is added to


# ---------------------------------------------------------------------------------------------------------------------------
# data and the reference
# ---------------------------------------------------------------------------------------------------------------------------
def config(mo, c):
    return mo.flag_file_config("args", memDim=c.d, ctrlDim=c.d, attDim=c.d, outClassifierDims=[c.H], answerWordsNum=c.A)


def masks_for(c, keep, dtype):
    return [torch.from_numpy(dh.mask_for(SEED, 7, 0, keep, (c.B, 2 * c.d), b0=c.b0, word=c.word)).to(dtype),
            torch.from_numpy(dh.mask_for(SEED, 8, 0, keep, (c.B, c.H), b0=c.b0, word=c.word)).to(dtype)]


def activation(cfg):
    return {"ELU": torch.nn.functional.elu, "STD": torch.relu}[cfg.relu]


def classifier_fp64(prm, memory, vecQ, act, keep=1.0, masks=None):
    """outputOp + classifier (model.py:512-576) in plain torch, in the dtype of its operands: outQuestion linear, concat, mask, fc_0, act,
    mask, fc_1.  prm: {field: tensor}.  -> logits, {"eq", "pre0", "logits"}: the three pre-activation tensors (retain_grad where they
    take part in a graph)"""
    eq = vecQ @ prm["outQuestion_W"] + prm["outQuestion_b"]
    x0 = torch.cat([memory, eq], dim=-1)
    if masks is not None:
        x0 = (x0 / keep) * masks[0]
    pre0 = x0 @ prm["fc0_W"] + prm["fc0_b"]
    x1 = act(pre0)
    if masks is not None:
        x1 = (x1 / keep) * masks[1]
    logits = x1 @ prm["fc1_W"] + prm["fc1_b"]
    pre = dict(eq=eq, pre0=pre0, logits=logits)
    for t in pre.values():
        if t.requires_grad:
            t.retain_grad()
    return logits, pre


def make_case(macx, mo, c):
    """(cfg, unit on the host, memory, vecQ, answers): seeded in the style of test_classifier_matches_oracle -- biases uniform in +-0.5,
    memory randn, vecQ uniform in +-1 -- with fc1_W scaled so that the evaluation logits have standard deviation PEAK"""
    cfg = config(mo, c)
    out = macx.OutputClassifier(cfg, generator=torch.Generator().manual_seed(1))
    assert type(out) is macx.OutputClassifier
    g = torch.Generator().manual_seed(c.seed)
    with torch.no_grad():
        for f in ("outQuestion_b", "fc0_b", "fc1_b"):
            getattr(out, f).copy_(torch.rand(getattr(out, f).shape, generator=g) - 0.5)
    mem = torch.randn(c.B, c.d, generator=g)
    vq = torch.rand(c.B, c.d, generator=g) * 2 - 1
    answers = torch.randint(0, c.A, (c.B,), generator=g)
    if c.A > 1:
        prm = {f: getattr(out, f).detach().double() for f in FIELDS}
        lg, _ = classifier_fp64(prm, mem.double(), vq.double(), activation(cfg))
        spread = float((lg - prm["fc1_b"]).std())
        with torch.no_grad():
            out.fc1_W.mul_(PEAK / spread)
    return cfg, out, mem, vq, answers


def cotangent(c, logits, answers):
    """d_logits as fp32 data: the gradient of the mean cross-entropy of the REFERENCE logits over the drawn answers ("ce"), so that the
    per-answer scales differ as in training; randn / B for A = 1, whose loss gradient is exactly zero"""
    if c.cot == "randn":
        return (torch.randn(c.B, c.A, generator=torch.Generator().manual_seed(3)) / c.B).float()
    p = torch.softmax(logits.detach().double(), dim=-1)
    p[torch.arange(c.B), answers] -= 1.0
    return (p / c.B).float()


def reference(c, cfg, out, mem, vq, answers, train, dtype=torch.float64, dl=None):
    """{"logits", "d_memory", "d_vecQ", field: gradient, "sum_abs": {bias field: sum_b |d preactivation|}, "dl": the cotangent}: the
    restatement and its gradients in `dtype`.  dl: the cotangent to use (None: drawn from this run's logits)"""
    prm = {f: getattr(out, f).detach().cpu().to(dtype).clone().requires_grad_(True) for f in FIELDS}
    m, v = mem.to(dtype).clone().requires_grad_(True), vq.to(dtype).clone().requires_grad_(True)
    keep = float(out.keep) if train else 1.0
    masks = masks_for(c, keep, dtype) if keep < 1.0 else None
    logits, pre = classifier_fp64(prm, m, v, activation(cfg), keep, masks)
    if dl is None:
        dl = cotangent(c, logits, answers)
    (logits * dl.to(dtype)).sum().backward()
    res = dict(logits=logits.detach(), d_memory=m.grad, d_vecQ=v.grad, dl=dl)
    res.update({f: prm[f].grad for f in FIELDS})
    res["sum_abs"] = {f: pre[k].grad.abs().sum(dim=0) for f, k in PRE.items()}
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------
def _ratio(err, scale):
    """err / scale per group; a group whose reference is exactly zero admits exactly zero (0) and nothing else (inf)"""
    out = err / scale.clamp_min(1e-300)
    return torch.where(scale > 0, out, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def _f64(t):
    return t.detach().cpu().double()


def per_question_err(got, ref):
    """[B]: largest |got - ref| of each question over that question's largest |ref|"""
    got, ref = _f64(got), _f64(ref)
    return _ratio((got - ref).abs().amax(dim=1), ref.abs().amax(dim=1))


def per_line_err(got, ref):
    """a [K, J] weight gradient: ([J] per column, [K] per row), each over that column's / row's largest |ref|"""
    got, ref = _f64(got), _f64(ref)
    d, a = (got - ref).abs(), ref.abs()
    return _ratio(d.amax(dim=0), a.amax(dim=0)), _ratio(d.amax(dim=1), a.amax(dim=1))


def bias_err(got, ref, sum_abs):
    """[J]: |got - ref| per element over sum_b |d preactivation[b, j]| of the fp64 run (division by the result itself is ill-posed under
    cancellation)"""
    return _ratio((_f64(got) - _f64(ref)).abs(), _f64(sum_abs))


METRICS = ("logits", "d_memory", "d_vecQ") + FIELDS


def errors(got, ref):
    """{metric: figure}, "where": the worst question / column / row of each, described.  got: {"logits", "d_memory", "d_vecQ", fields}"""
    e, where = {}, []
    e["logits"] = float((_f64(got["logits"]) - _f64(ref["logits"])).abs().max())
    for k in ("d_memory", "d_vecQ"):
        q = per_question_err(got[k], ref[k])
        e[k] = float(q.max())
        where.append("%s question %d" % (k, int(q.argmax())))
    for f in FIELDS:
        if f.endswith("_W"):
            col, row = per_line_err(got[f], ref[f])
            e[f] = max(float(col.max()), float(row.max()))
            where.append("%s column %d (%.2e) row %d (%.2e)" % (f, int(col.argmax()), float(col.max()), int(row.argmax()), float(row.max())))
        else:
            b = bias_err(got[f], ref[f], ref["sum_abs"][f])
            e[f] = float(b.max())
            where.append("%s element %d" % (f, int(b.argmax())))
    e["where"] = "; ".join(where)
    return e


def tolerances():
    t = {k: GRAD_TOL for k in METRICS}
    t["logits"] = LOGIT_TOL
    return t


def line(c, what, train, e):
    tol = tolerances()
    return "%-24s %-5s %-5s " % (c.id, what, "train" if train else "keep1") + " ".join("%s %.2f" % (k, e[k] / tol[k]) for k in METRICS)


def log(text):
    """append to the file MACX_OUTPUT_GEOMETRY_LOG names (how profiles/output_geometry_errors.txt is recorded); always printed (-s)"""
    print(text)
    path = os.environ.get("MACX_OUTPUT_GEOMETRY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(text + "\n")


# ---------------------------------------------------------------------------------------------------------------------------
# the generic classifier (no --outQuestion, two hidden layers of 128): data, reference, metrics
# ---------------------------------------------------------------------------------------------------------------------------
GENERIC = ((65, 1845, 1920), (5, 17, 128))      # (B, answers, the answer axis padded to the kernels' 128-column granule)
GENERIC_D, GENERIC_DIMS, GENERIC_B0 = 128, (128, 128), 3
GENERIC_W = ["classifier/linearLayerfc_%d/weights/weight" % i for i in range(3)]
GENERIC_B = ["classifier/linearLayerfc_%d/biases/bias" % i for i in range(3)]


def generic_config(mo, A):
    return mo.flag_file_config("args", memDim=GENERIC_D, ctrlDim=GENERIC_D, attDim=GENERIC_D, answerWordsNum=A, outQuestion=False,
                               outClassifierDims=list(GENERIC_DIMS))


def generic_fp64(prm, memory, act, keep=1.0, masks=None):
    """classifier (model.py:547-576) over the memory alone: mask, fc_i, act between layers.  -> logits, [pre-activations]"""
    x, pre = memory, []
    for i in range(3):
        if masks is not None:
            x = (x / keep) * masks[i]
        x = x @ prm[GENERIC_W[i]] + prm[GENERIC_B[i]]
        if x.requires_grad:
            x.retain_grad()
        pre.append(x)
        if i < 2:
            x = act(x)
    return x, pre


def generic_data(mo, B, A):
    """(cfg, {reference name: fp32 tensor}, memory, answers): the oracle's own initialisers, biases uniform in +-0.5, the last weight
    scaled as make_case scales fc1_W"""
    cfg = generic_config(mo, A)
    vs = mo.VarStore(generator=torch.Generator().manual_seed(4))
    mo.output_classifier(cfg, vs, torch.zeros(B, GENERIC_D), torch.zeros(B, GENERIC_D))
    g = torch.Generator().manual_seed(5)
    prm = {k: v.detach().clone().float() for k, v in vs.params.items()}
    assert list(prm) == [n for pair in zip(GENERIC_W, GENERIC_B) for n in pair]
    for k in GENERIC_B:
        prm[k] = torch.rand(prm[k].shape, generator=g) - 0.5
    mem = torch.randn(B, GENERIC_D, generator=g)
    answers = torch.randint(0, A, (B,), generator=g)
    lg, _ = generic_fp64({k: v.double() for k, v in prm.items()}, mem.double(), activation(cfg))
    prm[GENERIC_W[2]] = prm[GENERIC_W[2]] * (PEAK / float((lg - prm[GENERIC_B[2]].double()).std()))
    return cfg, prm, mem, answers


def generic_masks(site_of, B, keep, dtype, seed=SEED, b0=GENERIC_B0):
    widths = (GENERIC_D,) + GENERIC_DIMS
    return [torch.from_numpy(dh.mask_for(seed, site_of(i), 0, keep, (B, w), b0=b0)).to(dtype) for i, w in enumerate(widths)]


def generic_reference(cfg, prm, mem, answers, keep, masks, dtype=torch.float64, dl=None):
    """{"logits", "d_memory", name: gradient, "sum_abs": {bias name: ...}, "dl"} in `dtype`"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in prm.items()}
    m = mem.to(dtype).clone().requires_grad_(True)
    logits, pre = generic_fp64(p, m, activation(cfg), keep, masks)
    if dl is None:
        q = torch.softmax(logits.detach().double(), dim=-1)
        q[torch.arange(mem.shape[0]), answers] -= 1.0
        dl = (q / mem.shape[0]).float()
    (logits * dl.to(dtype)).sum().backward()
    res = dict(logits=logits.detach(), d_memory=m.grad, dl=dl)
    res.update({k: v.grad for k, v in p.items()})
    res["sum_abs"] = {k: pre[i].grad.abs().sum(dim=0) for i, k in enumerate(GENERIC_B)}
    return res


def generic_label(name):
    """fc0_W ... fc2_b for the six reference names"""
    return "fc%d_%s" % (GENERIC_W.index(name), "W") if name in GENERIC_W else "fc%d_b" % GENERIC_B.index(name) if name in GENERIC_B else name


def generic_errors(got, ref):
    e = dict(logits=float((_f64(got["logits"]) - _f64(ref["logits"])).abs().max()), d_memory=float(per_question_err(got["d_memory"], ref["d_memory"]).max()))
    for k in GENERIC_W:
        col, row = per_line_err(got[k], ref[k])
        e[k] = max(float(col.max()), float(row.max()))
    for k in GENERIC_B:
        e[k] = float(bias_err(got[k], ref[k], ref["sum_abs"][k]).max())
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# the loss kernels on their own
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(65, 1845), (129, 1845), (1000, 17), (3, 3129)]
LOSS_TOL = 1e-5               # loss rows and the mean loss, absolute (tests/test_gpu_output.py, tests/test_gpu_answer_weights.py)


def loss_case(B, A, seed=0):
    """(logits, answers, {row: first maximum}): randn * 2; row 0 ties its maximum in columns 5 and 1797 (one lane's passes 0 and 28; 5 and
    A - 1 where the row is shorter), row 1 in columns 63 and 64 (two lanes, two passes; 0 and A - 1 where shorter); row 2's label is A - 1"""
    g = torch.Generator().manual_seed(7000 + 10 * B + A + seed)
    logits = torch.randn(B, A, generator=g) * 2
    answers = torch.randint(0, A, (B,), generator=g, dtype=torch.int32)
    top = logits.max(dim=1).values + 1.0
    ties = {0: (5, 1797) if A > 1797 else (5, A - 1), 1: (63, 64) if A > 64 else (0, A - 1)}
    for r, (a, b) in ties.items():
        logits[r, a] = logits[r, b] = top[r]
    answers[2] = A - 1
    return logits, answers, {r: a for r, (a, b) in ties.items()}


def dlogits_bound(logits, answers, scale):
    """[B, A]: the error admitted per element of dlogits = (softmax - onehot) * scale.  Relative to (softmax + onehot) * scale:
    (R + A / 64 + 16) * 2^-24, R the row's logit range -- the rounding of the exponent's argument (half an ulp of at most R: a relative
    R * 2^-24 of the exponential), a lane's A / 64 sequential additions into z, and 16 for expf (numerator and terms of z), the six levels
    of the wave sum, the reciprocal and the two products."""
    x = logits.double()
    p = torch.softmax(x, dim=-1)
    hot = torch.zeros_like(p)
    hot[torch.arange(x.shape[0]), answers.long()] = 1.0
    R = (x.amax(dim=1) - x.amin(dim=1)).unsqueeze(1)
    return (R + x.shape[1] / 64.0 + 16.0) * 2.0 ** -24 * (p + hot) * scale
