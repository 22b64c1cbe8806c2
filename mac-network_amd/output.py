"""Output unit + classifier (model.py:512-576, ops.py:349-359) over libmacx.so: the consumer of the
cell's final memory, and the tensor the parity bar is stated on (classifier logits within 1e-4,
identical answer argmax).  SURVEY.md 8f row 2.

    out = OutputClassifier(config, answerWordsNum=28).to(device)
    logits = out(memory, vecQuestions, train=True, seed=step)       # [B, answers], differentiable
"""
import torch

from . import _lib, generic, unit
from .generic import B_SAME, OP_MUL, GenericParams, _Binary, _Dropout, _Linear, _Ops
from .options import UnsupportedOptions, _resolve_act, fresh_seed

REF_NAMES = {
    "outQuestion_W": "outputUnit/linearLayeroutQuestion/weights/weight",
    "outQuestion_b": "outputUnit/linearLayeroutQuestion/biases/bias",
    "fc0_W": "classifier/linearLayerfc_0/weights/weight", "fc0_b": "classifier/linearLayerfc_0/biases/bias",
    "fc1_W": "classifier/linearLayerfc_1/weights/weight", "fc1_b": "classifier/linearLayerfc_1/biases/bias",
}


def _check_fused(config):
    g = lambda n, dflt: getattr(config, n, dflt)
    if not g("outQuestion", False) or g("outQuestionMul", False) or g("outImage", False) or g("answerMod", "NON") != "NON":
        raise UnsupportedOptions("output unit: only --outQuestion (no outQuestionMul/outImage/answerMod) has a fused HIP path")
    if len(list(g("outClassifierDims", [512]))) != 1:
        raise UnsupportedOptions("classifier: exactly one hidden layer (outClassifierDims=[h]) has a fused HIP path")
    if g("outputBN", False):
        raise UnsupportedOptions("--outputBN has no fused HIP path")
    if g("relu", "ELU") == "PRM":
        raise UnsupportedOptions("--relu PRM has no fused HIP path in the classifier")


class OutputClassifier(unit.FusedUnit):
    """Fused output unit (--outQuestion, one hidden layer).  Constructing it for any other legal option set returns a
    GenericOutputClassifier: the same interface on one HIP kernel per reference op."""
    FIELDS, REF_NAMES, ABI = _lib.OUT_FIELDS, REF_NAMES, "output"
    SHAPES, PARAMS, GRADS = _lib.MacxOutShapes, _lib.MacxOutParams, _lib.MacxOutGrads
    check_fused = staticmethod(_check_fused)
    SIZE_ERROR = "output unit: d and hidden must be multiples of 16"

    def __init__(self, config, answerWordsNum=None, generator=None):
        super().__init__()
        g = lambda n, dflt: getattr(config, n, dflt)
        _check_fused(config)
        dims = list(g("outClassifierDims", [512]))
        d = g("memDim", 512)
        self.d, self.hidden = d, dims[0]
        self.answers = int(answerWordsNum if answerWordsNum is not None else g("answerWordsNum", 28))
        self.act = _resolve_act(config, "RELU")          # FCLayer's default act (ops.py:349)
        self.keep = float(g("outputDropout", 0.85))
        shapes = {"outQuestion_W": (d, d), "outQuestion_b": (d,), "fc0_W": (2 * d, self.hidden), "fc0_b": (self.hidden,),
                  "fc1_W": (self.hidden, self.answers), "fc1_b": (self.answers,)}
        for f in self.FIELDS:
            sh = shapes[f]
            t = torch.zeros(sh) if f.endswith("_b") else unit.xavier_uniform(sh, sh[0] + sh[1], generator)      # ops.py:20
            self.register_parameter(f, torch.nn.Parameter(t))

    def forward(self, memory, vecQuestions, train=False, seed=None, b0=0, mask_word=None):
        """mask_word: None, or the run's mask word (1-element int32 device tensor, as MACCell's), XORed into the keys of both
        layer-input dropouts when the kernels run."""
        unit.require_device(memory, "the output unit")
        B, d = memory.shape
        sh = self.SHAPES(B=B, d=d, hidden=self.hidden, answers=self.answers, b0=int(b0))
        keep = self.keep if train else 1.0          # model.py:118-125
        return self._call(sh, (self.act, keep), seed, train, mask_word, memory, vecQuestions)

    def _outputs(self, sh, inputs):
        return (torch.empty(sh.B, self.answers, dtype=torch.float32, device=inputs[0].device),), inputs

    def _backward(self, sh, X, d_outs):
        d_inputs = tuple(torch.empty_like(x) for x in X)      # d_memory, d_vecQuestions
        return (d_outs[0].contiguous(),), d_inputs, d_inputs


def fc_site(layer):
    """Dropout site of the input of classifier layer `layer` on the stateless stream (macx_common.hip.h: 7, 8; 13, 14, ... for
    deeper classifiers)."""
    return 7 + layer if layer < 2 else 11 + layer


class GenericOutputClassifier(generic.ParamsUnit, torch.nn.Module):
    """outputOp (model.py:512-528) + classifier (model.py:547-576) for the legal option sets the fused kernels refuse --
    no --outQuestion, --outQuestionMul, any number of classifier layers, --relu PRM/STD -- as ONE HIP KERNEL PER REFERENCE
    OP (generic._Ops on macx_linear / macx_wgrad / macx_op_*), variables under the reference's names in its creation
    order.  --outImage and --answerMod != NON raise what the reference raises (its own calls do not match its own
    signatures); --outputBN is refused.  Layer widths must be multiples of 128 (the last layer's answerWordsNum is padded
    with zero columns inside the call)."""

    def __init__(self, config, answerWordsNum=None, generator=None, device=None):
        super().__init__()
        dflt = dict(outImage=False, answerMod="NON", outputBN=False, outputDropout=0.85, memDim=512, ctrlDim=512,
                    outClassifierDims=[512], outQuestion=False, outQuestionMul=False, relu="STD")        # config.py:196, 281-288
        g = lambda n: getattr(config, n, dflt[n])
        if g("outImage"):
            # model.py:521-522 calls ops.linearizeFeatures(..., outputDim=...); its parameter is `outDim` (ops.py:595)
            raise TypeError("linearizeFeatures() got an unexpected keyword argument 'outputDim'")
        if g("answerMod") == "DIAG":
            raise UnboundLocalError("local variable 'output' referenced before assignment")      # ops.py:704-707 via model.py:561
        if g("answerMod") != "NON":
            raise NameError("name 'outputDim' is not defined")          # model.py:563
        if g("outputBN"):
            raise UnsupportedOptions("--outputBN: batch normalisation inside ops.linear has no HIP path")
        self.config = config
        self.answers = int(answerWordsNum if answerWordsNum is not None else getattr(config, "answerWordsNum", 28))
        self.keep = float(g("outputDropout"))
        self.d, self.ctrl = int(g("memDim")), int(g("ctrlDim"))
        self.dims = [int(x) for x in g("outClassifierDims")]
        self.params = GenericParams(device=device, generator=generator)
        self.ops = _Ops(config, self.params)
        self._declare()

    # the variables, in the order the reference's graph creates them (the forward pass below finds them by name)
    def _declare(self):
        vs, ops, cfg = self.params, self.ops, self.config
        dim = self.d
        with vs.scope("outputUnit"):
            if getattr(cfg, "outQuestion", False):
                with vs.scope("linearLayeroutQuestion"):
                    ops.getWeight((self.ctrl, self.d))
                    ops.getBias((self.d,))
                dim = 3 * self.d if getattr(cfg, "outQuestionMul", False) else 2 * self.d
        self.in_dim = dim
        dims = [dim] + self.dims + [self.answers]
        with vs.scope("classifier"):
            for i in range(len(dims) - 1):
                with vs.scope("linearLayerfc_%d" % i):
                    ops.getWeight((dims[i], dims[i + 1]))
                    ops.getBias((dims[i + 1],))
                if i < len(dims) - 2 and getattr(cfg, "relu", "ELU") == "PRM":
                    with vs.scope("prelu", default=True):
                        vs.get("alpha", (dims[i + 1],), 0.25)

    def forward(self, memory, vecQuestions, train=False, seed=None, b0=0, mask_word=None):
        unit.refuse_mask_word(mask_word, "output unit", "macx_output_forward_w", "classifier")
        generic._require_device(memory, "memory")                        # no CPU path
        vs, ops, cfg = self.params, self.ops, self.config
        keep = self.keep if train else 1.0                               # model.py:118-125
        seed = fresh_seed(seed, train)
        features, dim = memory, self.d
        with vs.scope("outputUnit"):
            if getattr(cfg, "outQuestion", False):
                eq = ops.linear(vecQuestions, self.ctrl, self.d, name="outQuestion")
                parts = [features, eq]
                if getattr(cfg, "outQuestionMul", False):
                    parts.append(_Binary.apply(features.contiguous(), eq, OP_MUL, B_SAME, 1.0))
                features = torch.cat(parts, dim=-1)                       # ops.concat (ops.py:65-78)
                dim = self.d * len(parts)
        dims = [dim] + self.dims + [self.answers]
        with vs.scope("classifier"):                                     # ops.FCLayer (ops.py:349-359), act = RELU -> config.relu
            for i in range(len(dims) - 1):
                drop = None
                if keep < 1.0:
                    per_q = dims[i]
                    drop = (lambda x, i=i, per_q=per_q: _Dropout.apply(x, seed, fc_site(i), 0, keep, int(b0) * per_q))
                last = i == len(dims) - 2
                if last and dims[i + 1] % 128:
                    # answerWordsNum is not a multiple of the kernels' 128-column granule: zero columns are appended for the
                    # call and cut off again (memory ops only; their gradient is exactly zero)
                    with vs.scope("linearLayerfc_%d" % i):
                        W, b = ops.getWeight((dims[i], dims[i + 1])), ops.getBias((dims[i + 1],))
                    pad = (-dims[i + 1]) % 128
                    x = drop(features) if drop is not None else features
                    Wp = torch.cat([W, W.new_zeros(dims[i], pad)], dim=1)
                    bp = torch.cat([b, b.new_zeros(pad)])
                    features = _Linear.apply(x, Wp, bp)[:, : dims[i + 1]]
                else:
                    features = ops.linear(features, dims[i], dims[i + 1], dropout=drop, name="fc_%d" % i)
                if not last:
                    features = ops.act("RELU", features)
        return features


OutputClassifier.GENERIC = GenericOutputClassifier


class _AnswerLoss(torch.autograd.Function):
    """macx_answer_loss: per-question cross-entropy + argmax in one kernel; the backward pass returns the dlogits the same
    kernel wrote (gradient of the MEAN loss), scaled by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, answers):
        if not logits.is_cuda:
            raise RuntimeError("logits must live on the HIP device: the loss has no CPU path")
        L = _lib.lib()
        lg = logits.detach().contiguous()
        B, A = lg.shape
        ans = answers.to(device=lg.device, dtype=torch.int32).contiguous()      # out-of-range labels: NaN loss, as TF on a GPU
        rows = torch.empty(B, dtype=torch.float32, device=lg.device)
        pred = torch.empty(B, dtype=torch.int32, device=lg.device)
        dl = torch.empty_like(lg)
        ptr = _lib.ptr
        _lib.check(L.macx_answer_loss(ptr(lg), ptr(ans), B, A, ptr(rows), ptr(pred), ptr(dl), 1.0 / B, _lib.stream_of(lg)), "macx_answer_loss")
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(pred)
        return rows, pred

    @staticmethod
    def backward(ctx, g_rows, _g_pred):
        (dl,) = ctx.saved_tensors
        # rows feed a mean: g_rows is constant 1/B * upstream; dl already carries 1/B, so scale by B * g_rows per row
        return dl * (g_rows * dl.shape[0]).unsqueeze(1), None


class AnswerTotals:
    """The running totals of macx_answer_loss_weighted: three doubles in device memory -- sum of w * loss, sum of w * [pred == answer],
    sum of w -- to which every call that is handed this object ADDS, replays of a captured graph included, until reset().

        totals = macx.output.AnswerTotals(device)
        for batch in loader: ... net.loss_and_pred(logits, answers, weights, totals=totals)       # no host synchronisation
        totals.read()                                  # {"loss": .., "accuracy": .., "weight": ..}: the one synchronisation

    `tensor` is the buffer ([3] float64).  A captured class allocates it before its capture: the host clears it outside the graph
    (DESIGN 8)."""

    def __init__(self, device):
        self.tensor = torch.zeros(3, dtype=torch.float64, device=device)

    def reset(self):
        self.tensor.zero_()

    def read(self):
        """dict(loss = sum w l / W, accuracy = sum w [correct] / W, weight = W); both ratios are 0 when W == 0.  Synchronises."""
        loss, hit, w = self.tensor.tolist()
        return dict(loss=loss / w if w > 0 else 0.0, accuracy=hit / w if w > 0 else 0.0, weight=w)


def _answer_weights(weights, B):
    """the weights= argument, in the style of losses._device_f32: a [B] float32 tensor on the HIP device (None: all ones)"""
    if weights is None:
        return None
    if not torch.is_tensor(weights) or weights.dtype != torch.float32:
        raise TypeError("weights must be a float32 tensor")
    if tuple(weights.shape) != (B,):
        raise ValueError("weights must be [%d] (one per question), got %s" % (B, list(weights.shape)))
    if not weights.is_cuda:
        raise RuntimeError("weights must live on the HIP device: the loss has no CPU path")
    return weights.detach().contiguous()


def _answer_totals(totals):
    if totals is None:
        return None
    if not isinstance(totals, AnswerTotals):
        raise TypeError("totals is None or a macx.output.AnswerTotals, not %r" % (totals,))
    if not totals.tensor.is_cuda:
        raise RuntimeError("totals must live on the HIP device: the loss has no CPU path")
    return totals.tensor


class _WeightedAnswerLoss(torch.autograd.Function):
    """macx_answer_loss_weighted: the weighted-mean cross-entropy (a 0-dim tensor the kernel wrote), argmax with -1 in dead rows, and
    the gradient of that mean from the same launch; the backward pass returns the stored dlogits times the incoming scalar.  Weights
    and totals are data: no gradient flows to them.  Without a gradient to compute (no_grad, constant logits) dlogits is NULL."""

    @staticmethod
    def forward(ctx, logits, answers, weights, totals):
        if not logits.is_cuda:
            raise RuntimeError("logits must live on the HIP device: the loss has no CPU path")
        L = _lib.lib()
        lg = logits.detach().contiguous()
        B, A = lg.shape
        ans = answers.to(device=lg.device, dtype=torch.int32).contiguous()
        rows = torch.empty(B, dtype=torch.float32, device=lg.device)
        pred = torch.empty(B, dtype=torch.int32, device=lg.device)
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        dl = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        ptr = _lib.ptr
        _lib.check(L.macx_answer_loss_weighted(ptr(lg), ptr(ans), ptr(weights), B, A, ptr(rows), ptr(pred), ptr(dl), ptr(loss), ptr(totals),
                                               1.0, _lib.stream_of(lg)), "macx_answer_loss_weighted")
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(pred, rows)
        return loss, pred, rows

    @staticmethod
    def backward(ctx, g_loss, _g_pred, _g_rows):
        (dl,) = ctx.saved_tensors
        return dl * g_loss, None, None, None


def answer_loss_and_pred(logits, answers, weights=None, totals=None):
    """addAnswerLossOp (model.py:593-599) + addPredOp (model.py:603-612): mean sparse CE, int32 argmax -- one HIP kernel
    (macx_answer_loss) for both and for the gradient.

    weights / totals (both None: the call above, launch for launch): one launch of macx_answer_loss_weighted instead.
    weights: a [B] float32 tensor on the HIP device, read when the kernel runs; question b is live iff weights[b] > 0.  The loss becomes
    the weighted mean  sum_live w_b l_b / W,  W = sum_live w_b  (0 when no question is live), differentiable with respect to logits;
    pred is -1 in dead rows, whose logits and answers are never read (a partial batch pads with anything) and whose gradient rows are
    exactly +0.  None with totals given: all ones.  totals: an AnswerTotals to which the launch adds its weighted loss, correct count
    and weight.  TypeError / ValueError / RuntimeError for anything else; no CPU path.
    The call only sees logits, so it serves every tower, the ones with generic modules included (whose capture stays refused:
    graph.CapturedTowerTrainStep).  Out of scope: several processes -- the weighted mean over a global batch needs W summed over the
    ranks, which this call does not do; the cell-level captured classes, whose caller owns d_memory and so the loss."""
    if weights is None and totals is None:
        rows, pred = _AnswerLoss.apply(logits, answers)
        return rows.mean(), pred
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise ValueError("logits must be a [B, answers] tensor")
    weights, totals = _answer_weights(weights, logits.shape[0]), _answer_totals(totals)
    loss, pred, _ = _WeightedAnswerLoss.apply(logits, answers, weights, totals)
    return loss, pred
