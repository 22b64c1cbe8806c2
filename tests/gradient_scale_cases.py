"""Backward passes at the gradient scales training produces: case builders, references and metrics shared by
tests/test_gradient_scale_host.py (no GPU: the inputs are well-conditioned) and tests/test_gpu_gradient_scale.py (-m gpu).
Pure torch plus the oracle; `macx` is handed in by the caller and only its host side (parameter modules) is touched here.

What the other backward tests cannot see: they feed unit-scale gradients and divide an error by the largest entry of the WHOLE
tensor (helpers.rel_err, floored at 1e-6), so a question whose gradients sit 2^-20 below its neighbour's may be wrong in every
element, and a batch of small gradients passes whatever it holds.  Here

    per_question_err(got, ref)        max |got_b - ref_b| / max |ref_b| for every question b, no absolute floor; a question whose
                                      reference is exactly zero must be exactly zero
    scaled_rel_err(got, ref, unit)    max |got - ref| / max(max |ref|, floor * unit) for parameter gradients (sums over questions):
                                      unit = the case's largest per-question gradient scale, so the project's floors (5e-2 for the
                                      analytically zero softmax logit biases, 1e-6 otherwise) scale with the gradients

are held to the bounds the suite already uses (test_gpu_cell.GRAD_TOL / FWD_TOL).  Whether an input is FAIR is decided by the fp32
oracle against the fp64 oracle on the same data (test_gradient_scale_host.py: a tenth of the bound), never by the HIP code.

Every result -- oracle or HIP -- is a flat {key: tensor}: "memory", "d_kb", "d_words", "d_vq" and "param:<reference variable>"."""
import math

import torch

from oracle import dropout_hash as dh
from oracle import mac_oracle as mo
from helpers import make_case, oracle_run, rel_err

GRAD_TOL = 2e-4          # = test_gpu_cell.GRAD_TOL (the GPU tests assert the two are the same numbers)
FWD_TOL = 2e-5           # = test_gpu_cell.FWD_TOL
LOGIT_BIAS = "linearLayerlogits/biases/bias"
INPUT_KEYS = ("d_kb", "d_words", "d_vq")
INF = float("inf")

B = 4
SCALES = (0, -10, -20, -30)              # per-question gradient scales 2^s_b
SCALES_PERMUTED = (-20, -30, 0, -10)     # ... with the large question not in front
# (config, S, N, d, p): the smallest shapes that still select each route of the backward pass (asserted on the library's own route
# plan by tests/test_route_host.py)
SHAPES = {
    "launch": ("args", 7, 49, 128, 2),       # the narrowest chain kernel (64-row tiles), S_b deferred on the 128 x 128 kernel
    "step_sb": ("args1", 7, 20, 256, 3),     # N < 32: the per-step S_b route
    "nochain": ("args", 7, 14, 128, 2),      # N < 16: no chain kernels
    "chain": ("args", 7, 196, 512, 2),       # chain kernels, 16-row tiles
    "selfatt": ("args3", 6, 49, 128, 3),     # self-attention (args3 has no gate)
}
ZERO_QUESTIONS = (1, 3)
HOMOGENEITY_K = (-40, -16, 16, 40)
HOMOGENEITY_FLOOR = 2.0 ** -100           # elements of base * 2^k below this are left out of the bit comparison (< 1 % of a tensor)


# ---------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------
def per_question_err(got, ref):
    """[B, ...] tensors -> list of max |got_b - ref_b| / max |ref_b|.  No floor: a question whose reference is exactly zero must be
    exactly zero (0.0), anything else -- and anything not finite -- is inf."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    out = []
    for b in range(ref.shape[0]):
        g, r = got[b].reshape(-1), ref[b].reshape(-1)
        top = float(r.abs().max())
        if not bool(torch.isfinite(g).all()):
            out.append(INF)
        elif top == 0.0:
            out.append(0.0 if not bool((g != 0).any()) else INF)
        else:
            out.append(float((g - r).abs().max()) / top)
    return out


def scaled_rel_err(got, ref, unit, floor=1e-6):
    """max |got - ref| / max(max |ref|, floor * unit); inf for anything not finite"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return INF
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), floor * unit)


def param_floor(key):
    return 5e-2 if key.endswith(LOGIT_BIAS) else 1e-6


def errors(got, ref, unit, grad_tol=GRAD_TOL, fwd_tol=FWD_TOL, floor=param_floor):
    """{key: (error, bound)} of a result against a reference: input gradients per question (the worst question), parameter
    gradients with the scaled floor, the final memory as everywhere else in the suite."""
    out = {}
    for k, r in ref.items():
        if k == "memory":
            out[k] = (rel_err(got[k], r), fwd_tol)
        elif k in INPUT_KEYS:
            out[k] = (max(per_question_err(got[k], r)), grad_tol)
        else:
            out[k] = (scaled_rel_err(got[k], r, unit, floor=floor(k)), grad_tol)
    return out


def worst(errs):
    """(key, error / bound) of the entry closest to (or farthest past) its bound"""
    k = max(errs, key=lambda k: errs[k][0] / errs[k][1])
    return k, errs[k][0] / errs[k][1]


def scaled(res, k):
    """a result times 2^k (gradients only: the forward pass does not see the loss scale)"""
    return {key: (t if key == "memory" else t * 2.0 ** k) for key, t in res.items()}


def excluded_fraction(t, k, floor=HOMOGENEITY_FLOOR):
    """share of the elements of t with |t| * 2^k below the floor of the homogeneity test"""
    t = t.detach().cpu().double().abs() * 2.0 ** k
    return float((t < floor).double().mean()) if t.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the cell
# ---------------------------------------------------------------------------------------------------------------------------
class CellCase:
    """One set of inputs of a cell run in training mode (dropout as the configuration has it).

    scales        per-question exponents s_b: d_memory[b], d_control[b] = randn * 2^s_b;  None: unit scale, randn
    grad_scale    a factor on both (the 1e-6 of the zero-question cases)
    zero_grad     questions whose d_memory / d_control rows are exactly zero
    kb_range      r: knowledge-base row (b, n) times 2^u, u uniform in [-r, r]
    logits_gain   factor on the read unit's logit weights (kbLogits_w): 16 drives attentions up to ~0.98
    zero_kb       a question whose knowledge-base rows are all exactly zero
    unit          the largest per-question gradient scale (what scaled_rel_err takes): grad_scale * 2^max(s) * 2^(2 kb_range)"""

    def __init__(self, shape, scales=SCALES, grad_scale=1.0, zero_grad=(), kb_range=0.0, logits_gain=1.0, zero_kb=None):
        self.shape = shape
        self.key = (shape, tuple(scales) if scales is not None else None, grad_scale, tuple(zero_grad), kb_range, logits_gain, zero_kb)
        name, S, N, d, p = SHAPES[shape]
        self.B, self.S, self.N, self.d, self.p = B, S, N, d, p
        self.cfg, self.vq, self.words, self.lengths, kb = make_case(name, B, S, N, d, p)
        g = torch.Generator().manual_seed(9)
        dmem = torch.randn(B, d, generator=g)
        dctl = torch.randn(B, d, generator=g)
        if kb_range:
            u = (torch.rand(B, N, 1, generator=g) * 2 - 1) * kb_range
            kb = kb * torch.exp2(u)
        if zero_kb is not None:
            kb = kb.clone()
            kb[zero_kb] = 0.0
        f = torch.full((B, 1), float(grad_scale))
        if scales is not None:
            f = f * torch.exp2(torch.tensor(scales, dtype=torch.float32)).reshape(B, 1)
        for b in zero_grad:
            f[b] = 0.0
        self.kb, self.dmem, self.dctl = kb.contiguous(), dmem * f, dctl * f
        # kb_range: the gradient of a knowledge-base logit is linear in the scale of the row it reads out (da_n = <dinfo, kb_n>), and
        # from the second-last step backwards dinfo itself arrives through the next step's interactions, which are linear in it
        # again: with p >= 2 the per-question gradient scale grows by the SQUARE of the largest row scale.  The fp64 reference
        # agrees -- its logit-weight and memKbProj gradients are 2^11 .. 2^12 times those of the plain case -- and the fp32 oracle
        # shows what ignoring it means: the analytically zero logit-bias sums, held to 5e-2 * 2^0, would sit at 1.5 (N = 49) and
        # 12 (N = 196, d = 512) times the bound in a plain fp32 restatement (tests/test_gradient_scale_host.py).
        self.unit = float(grad_scale) * (2.0 ** max(scales) if scales is not None else 1.0) * 2.0 ** (2 * kb_range)
        self.zero_grad, self.logits_gain, self.seed = tuple(zero_grad), float(logits_gain), 5

    def params(self, macx):
        """The cell's parameters as test_gpu_cell.build_cell draws them (host tensors; the caller moves them)."""
        prm = macx.MACCellParams(self.cfg, self.p, generator=torch.Generator().manual_seed(5))
        g = torch.Generator().manual_seed(6)
        with torch.no_grad():
            for f in prm.fields:
                t = getattr(prm, f)
                if f.endswith("_b"):          # non-zero biases so that bias paths are exercised
                    t.copy_((torch.rand(t.shape, generator=g) - 0.5) * 0.2)
            prm.kbLogits_w.mul_(self.logits_gain)
        return prm


def oracle_result(out):
    """helpers.oracle_run(...) -> the flat result (an input or parameter the configuration never reads: zeros)"""
    vq, words, kb = out["inputs"]
    zero_if_none = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = {"memory": out["memory"].detach(), "d_kb": zero_if_none(kb), "d_words": zero_if_none(words), "d_vq": zero_if_none(vq)}
    for name, t in out["params"].items():
        res["param:" + name] = zero_if_none(t)
    return res


def oracle_cell(case, ref_params, dtype):
    return oracle_result(oracle_run(case.cfg, ref_params, case.vq, case.words, case.lengths, case.kb, train=True, seed=case.seed,
                                    dtype=dtype, need_grad=True, d_memory=case.dmem, d_control=case.dctl))


_REFERENCES = {}


def cell_reference(macx, case):
    """(fp64 oracle result, {key: (error, bound)} of the fp32 oracle against it) -- computed once per set of inputs and shared
    by every kernel family and route that runs on them; nobody writes into it."""
    if case.key not in _REFERENCES:
        ref_params = case.params(macx).to_reference_dict()
        r64 = oracle_cell(case, ref_params, torch.float64)
        r32 = oracle_cell(case, ref_params, torch.float32)
        _REFERENCES[case.key] = (r64, errors(r32, r64, case.unit))
    return _REFERENCES[case.key]


def cell_cases():
    """{id: CellCase} for the distinct INPUTS of items 1-4 (kernel families and routes share them)."""
    cases = {}
    for shape in SHAPES:                                              # 1. per-question gradient scales
        cases["scales-" + shape] = CellCase(shape)
    cases["scales-permuted-chain"] = CellCase("chain", scales=SCALES_PERMUTED)
    for shape in ("launch", "chain"):
        cases["zeros-" + shape] = CellCase(shape, scales=None, grad_scale=1e-6, zero_grad=ZERO_QUESTIONS)      # 2.
        cases["unit-" + shape] = CellCase(shape, scales=None)                                                   # 3. (k = 0)
        cases["kbrange-" + shape] = CellCase(shape, kb_range=6.0)                                               # 4.
        cases["gain16-" + shape] = CellCase(shape, logits_gain=16.0)
        cases["zerokb-" + shape] = CellCase(shape, zero_kb=1)
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# the stem: one exponent per operand tensor (macx_gemm3h.hip.h)
# ---------------------------------------------------------------------------------------------------------------------------
STEM_SHAPE = dict(B=3, H=4, W=3, Cin=128, Cmid=128, Cout=128)
STEM_FWD_SCALES = (0, -8, -16)
STEM_BWD_SCALES = (0, -10, -20)
STEM_FWD_TOL = 1e-5       # the stem tests' own (test_gpu_stem.test_stem_matches_conv2d_oracle)
STEM_SEED = 5


def stem_case(macx, image_scales=None, dout_scales=None, zero_dout=False):
    """(cfg, stem module on the host, images, d_out): test_gpu_stem.run_case's data with per-image scales 2^s"""
    s = STEM_SHAPE
    cfg = mo.flag_file_config("args", memDim=s["Cout"], ctrlDim=s["Cout"], attDim=s["Cout"])
    cfg.stemDim = s["Cmid"]
    stem = macx.Stem(cfg, H=s["H"], W=s["W"], inDim=s["Cin"], generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        stem.bias0.copy_(torch.rand(s["Cmid"], generator=g) - 0.5)
        stem.bias1.copy_(torch.rand(s["Cout"], generator=g) - 0.5)
    img = torch.relu(torch.randn(s["B"], s["H"] * s["W"], s["Cin"], generator=g))
    dout = torch.randn(s["B"], s["H"] * s["W"], s["Cout"], generator=g)
    pow2 = lambda e: torch.exp2(torch.tensor(e, dtype=torch.float32)).reshape(-1, 1, 1)
    if image_scales is not None:
        img = img * pow2(image_scales)
    if dout_scales is not None:
        dout = dout * pow2(dout_scales)
    if zero_dout:
        dout = torch.zeros_like(dout)
    return cfg, stem, img, dout


def oracle_stem(cfg, stem, img, dout, dtype):
    """{"out": stem output, "param:<name>": gradient} of the oracle's conv2d restatement in training mode (masks of STEM_SEED)"""
    s = STEM_SHAPE
    prm = {k: v.cpu().to(dtype).requires_grad_(True) for k, v in stem.to_reference_dict().items()}
    vs = mo.VarStore(params=prm, dtype=dtype)
    n = s["H"] * s["W"]
    masks = [torch.from_numpy(dh.mask_for(STEM_SEED, 9, 0, stem.keep, (s["B"], n, s["Cin"]))).to(dtype),
             torch.from_numpy(dh.mask_for(STEM_SEED, 10, 0, stem.keep, (s["B"], n, s["Cmid"]))).to(dtype)]
    out = mo.stem_cnn(cfg, vs, img.to(dtype), s["H"], s["W"], keep=stem.keep, masks=masks)
    (out * dout.to(dtype)).sum().backward()
    res = {"out": out.detach()}
    for k, v in prm.items():
        res["param:" + k] = v.grad
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the tower (test_gpu_encoder.test_full_tower_ids_to_logits_gradients, at its shape)
# ---------------------------------------------------------------------------------------------------------------------------
TOWER = dict(B=3, H=4, W=3, Cin=128, d=256, p=2, S=6, A=7, V=12, E=20)
TOWER_TOL = 3e-4          # that test's bound
TOWER_K = (-24, 24)
TOWER_SEED = 21


def tower_floor(key):
    return 5e-2 if key.endswith(LOGIT_BIAS) else 1e-7       # that test's floors


def tower_case(macx):
    """(cfg, MACNet on the host, images, question ids, lengths, answers)"""
    t = TOWER
    cfg = mo.flag_file_config("args", netLength=t["p"], memDim=t["d"], ctrlDim=t["d"], attDim=t["d"], encDim=t["d"], wrdEmbDim=t["E"],
                              outClassifierDims=[32], answerWordsNum=t["A"])
    cfg.stemDim = 128
    net = macx.MACNet(cfg, vocab=t["V"], H=t["H"], W=t["W"], imageInDim=t["Cin"], answerWordsNum=t["A"],
                      generator=torch.Generator().manual_seed(4))
    g = torch.Generator().manual_seed(6)
    img = torch.relu(torch.randn(t["B"], t["H"] * t["W"], t["Cin"], generator=g))
    from test_gpu_encoder import make_questions
    q, lengths = make_questions(t["B"], t["S"], t["V"], seed=3, min_len=2)
    return cfg, net, img, q, lengths, torch.tensor([1, 5, 2])


def tower_modules(macx, cfg, net):
    """[(module, {field: [(reference variable, index or None)]})] over the tower's four parts"""
    one = lambda names: {f: [(n, None)] for f, n in names.items()}
    return [(net.enc, one(macx.encoder.REF_NAMES)), (net.stem, one(macx.stem.REF_NAMES)),
            (net.cell, macx.params.reference_names(cfg, TOWER["p"])), (net.out, one(macx.output.REF_NAMES))]


def oracle_tower(cfg, net, img, q, lengths, ans, dtype):
    """{"logits", "loss", "param:<name>": d loss / d parameter} of the oracle chain with the masks of TOWER_SEED (loss scale 1)"""
    t = TOWER
    B, n, d = t["B"], t["H"] * t["W"], t["d"]
    prm = {}
    for src in (net.enc.to_reference_dict(), net.stem.to_reference_dict(), net.cell.to_reference_dict(), net.out.to_reference_dict()):
        prm.update({k: v.cpu().to(dtype).requires_grad_(True) for k, v in src.items()})
    vs = mo.VarStore(params=prm, dtype=dtype)
    keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout)
    sk, ok, ki, kq = net.stem.keep, net.out.keep, net.enc.keep_in, net.enc.keep_q
    mk = lambda site, keep, shape: torch.from_numpy(dh.mask_for(TOWER_SEED, site, 0, keep, shape)).to(dtype)
    words, vq = mo.question_encoder(cfg, vs, q, lengths, t["V"], keep_input=ki, keep_question=kq,
                                    masks=[mk(11, ki, (B, t["S"], t["E"])), mk(12, kq, (B, d))])
    kb = mo.stem_cnn(cfg, vs, img.to(dtype), t["H"], t["W"], keep=sk, masks=[mk(9, sk, (B, n, t["Cin"])), mk(10, sk, (B, n, 128))])
    c, m, _ = mo.mac_network(cfg, vs, vq, words, words, lengths, kb, train=True, mask_fn=mo.hash_mask_fn(TOWER_SEED, keeps), keeps=keeps)
    logits = mo.output_classifier(cfg, vs, m, vq, output_keep=ok, masks=[mk(7, ok, (B, 2 * d)), mk(8, ok, (B, 32))])
    loss, _ = mo.answer_loss_and_pred(logits, ans)
    loss.backward()
    res = {"logits": logits.detach(), "loss": loss.detach()}
    for k, v in prm.items():
        res["param:" + k] = torch.zeros_like(v) if v.grad is None else v.grad
    return res


def log2(x):
    return math.log2(x) if x > 0 else -INF
