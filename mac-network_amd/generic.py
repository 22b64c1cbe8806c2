"""The GENERIC option path of the MAC cell: every legal option combination of mac_cell.py that the fused cell kernels
(cell.py -> macx_cell_*) answer with UnsupportedOptions -- the reference's DEFAULT configuration, writeInputs != BOTH,
readMemAttType BL / ADD, relu = PRM, writeConcatMul, controlProj, controlConcatWords, unsharedCells, mulBias, ... -- runs
as one HIP kernel per primitive of a PLAN that plan.compile_cell derives from the option set once (plan.py: variable table in
the reference's creation order + a flat operation list per zero_state / step, executed and differentiated by plan.run_segment).
This module holds what both stacks of the path stand on -- the plan's executor (plan._Exec: the cell) and the eager autograd
nodes below (_Binary, _Act, _Linear, _Dropout, _Embed: the generic question encoder, output unit and stem):
  * the kernel calls (k_*), the only place that touches libmacx.so;
  * one RULE per primitive the two stacks share, directly under them: bin_bwd (backward of scale * (a op b) under the four
    spreads), linear_fwd / linear_bwd, act_bwd, and the two routing decisions mid_of / big_of.  _Exec's "bin" / "linear" / "act"
    branches and the eager nodes' forward / backward are calls of these, so a spread mode, a primitive or a fix exists once;
  * act_code, the one table from config.py's activation names (and --relu) to kernel codes, raising what the reference raises;
  * ScopeNames, the one TF scope namer, under the variable store (GenericParams) and under the plan's compiler;
  * the cell class that feeds the plan's segments, and the layer helpers (_Ops) of the generic encoder / output unit.

Every arithmetic step is a kernel of libmacx.so behind the C ABI (include/macx.h: macx_linear / macx_h2_gemm / macx_wgrad and
the macx_op_* primitives); PyTorch owns the device memory, the stream, the concat / slice copies and the autograd tape that
orders the backward kernels -- plumbing.  There is no CPU path: tensors must live on the HIP device.

Variables are created on first use under the reference's TF names (the same scope stacking as ops.py / mac_cell.py), so a
reference checkpoint loads by name (GenericParams.load_reference_dict) whatever the option set.

Widths off the kernels' 128-column granule run zero-padded inside the products (k_matmul, k_wgrad).  Not covered
(UnsupportedOptions, never a silent fallback): widths that are not multiples of 4.
"""
import collections
import math
from contextlib import contextmanager
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import ptr, stream_of
from .options import UnsupportedOptions, fresh_seed, get, reject_like_reference, DEFAULTS
from .unit import _kb_lengths, _mask_word

MACCellTuple = collections.namedtuple("MACCellTuple", ("control", "memory"))

OP_ADD, OP_MUL = 0, 1
B_SAME, B_MID, B_CHANNEL, B_ROW = 0, 1, 2, 3
R_MID, R_LAST, R_ROWS = 0, 1, 2
ACT_PRELU = 16
ACT_RSQRT_EPS = 17
SITE_MEM_VAR, SITE_MEM, SITE_READ_KB, SITE_READ_MEM, SITE_READ_ATT, SITE_WRITE_INFO = 1, 2, 3, 4, 5, 6


def _require_device(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the HIP device: the MAC cell has no CPU path" % name)


def _dev(t, name="tensor"):
    _require_device(t, name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32" % name)
    return t.contiguous()


def _L():
    return _lib.lib()


# -------------------------------------------------------------------------------------------------------------------
# the kernel calls (everything below this block is host logic; tests/test_generic_host.py swaps exactly these functions for
# torch restatements to check the chaining, the variable names and the backward formulas on a machine without a GPU)
# -------------------------------------------------------------------------------------------------------------------
def k_binary(op, bmode, a, b, mid, inner, scale=1.0):
    out = torch.empty_like(a)
    _lib.check(_L().macx_op_binary(op, bmode, ptr(a), ptr(b), a.numel(), mid, inner, scale, ptr(out), stream_of(a)), "macx_op_binary")
    return out


def k_reduce(mode, x, outer, mid, inner):
    shape = {R_MID: (outer, inner), R_LAST: (outer,), R_ROWS: (inner,)}[mode]
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    ws = torch.empty(64 * inner, dtype=torch.float32, device=x.device) if mode == R_ROWS else None
    _lib.check(_L().macx_op_reduce(mode, ptr(x), outer, mid, inner, ptr(out), ptr(ws), stream_of(x)), "macx_op_reduce")
    return out


def k_act(act, x, alpha):
    out = torch.empty_like(x)
    _lib.check(_L().macx_op_act(act, ptr(x), ptr(alpha), x.numel(), x.shape[-1], ptr(out), stream_of(x)), "macx_op_act")
    return out


def k_act_bwd(act, x, alpha, g):
    dx = torch.empty_like(x)
    de = torch.empty_like(x) if act == ACT_PRELU else None          # (ACT_RSQRT_EPS: alpha holds eps, no gradient)
    _lib.check(_L().macx_op_act_bwd(act, ptr(x), ptr(alpha), ptr(g), x.numel(), x.shape[-1], ptr(dx), ptr(de), stream_of(x)), "macx_op_act_bwd")
    return dx, de


def k_softmax(x, lengths):
    n = x.shape[-1]
    rows = x.numel() // n
    out = torch.empty_like(x)
    rpl = rows // lengths.numel() if lengths is not None else 1
    _lib.check(_L().macx_op_softmax(ptr(x), ptr(lengths), rpl, rows, n, ptr(out), stream_of(x)), "macx_op_softmax")
    return out


def k_softmax_bwd(a, g):
    n = a.shape[-1]
    dx = torch.empty_like(a)
    _lib.check(_L().macx_op_softmax_bwd(ptr(a), ptr(g), a.numel() // n, n, ptr(dx), stream_of(a)), "macx_op_softmax_bwd")
    return dx


def k_dropout(x, seed, site, step, keep, first, mask_word=None):
    """mask_word: macx_dropout.mask_word (1-element int32 device tensor XORed into the site key when the kernel runs) or None"""
    out = torch.empty_like(x)
    _lib.check(_L().macx_op_dropout_w(ptr(x), x.numel(), seed, site, step, keep, first, ptr(mask_word), ptr(out),
                                      stream_of(x)), "macx_op_dropout")
    return out


def _pad128(v):
    return (v + 127) // 128 * 128


def k_matmul(x, W, b, big):
    """x [rows, K] @ W [K, n] (+ b): the knowledge-base GEMM for [B, N, .] operands (big = (B, N)), macx_linear otherwise.
    Layer widths the kernels' 128-column granule does not divide (config.py:294-296 and every *Dim option take any integer) run
    zero-padded: zero rows of W meet zero columns of x, the padded output columns are dropped."""
    L = _L()
    rows, K = x.shape
    n = W.shape[1]
    Kp, np_ = _pad128(K), _pad128(n)
    if Kp != K or np_ != n:
        pad = torch.nn.functional.pad
        xp = pad(x, (0, Kp - K)).contiguous() if Kp != K else x
        Wp = pad(W, (0, np_ - n, 0, Kp - K)).contiguous()
        bp = pad(b, (0, np_ - n)).contiguous() if b is not None else None
        return k_matmul(xp, Wp, bp, big)[:, :n].contiguous()
    out = torch.empty((rows, n), dtype=torch.float32, device=x.device)
    bias = b if b is not None else torch.zeros(n, dtype=torch.float32, device=x.device)
    if big is not None:
        B, N = big
        nws = L.macx_h2_floats(rows, K) + L.macx_h2_floats(rows, n) + K * n + 64
        ws = torch.empty(nws, dtype=torch.float32, device=x.device)
        _lib.check(L.macx_h2_gemm(ptr(x), B, N, K, ptr(W), n, ptr(bias), 0, ptr(out), ptr(ws), nws, stream_of(x)), "macx_h2_gemm")
    else:
        wp = torch.empty(K * n, dtype=torch.float32, device=x.device)
        _lib.check(L.macx_pack_weight(ptr(W), K, n, _lib.PACK_F32MFMA, ptr(wp), stream_of(x)), "macx_pack_weight")
        _lib.check(L.macx_linear(ptr(x), K, None, 0, rows, ptr(wp), ptr(bias), 0.0, n, 0, ptr(out), stream_of(x)), "macx_linear")
    return out


def k_embed(ids, emb, E, ld, keep, seed, first_row):
    """rows of the zero-padded embedding table for `ids` [rows] int32, through the input dropout: [rows, ld] (columns >= E zero)."""
    out = torch.empty((ids.numel(), ld), dtype=torch.float32, device=emb.device)
    _lib.check(_L().macx_embed_lookup(ptr(ids), ptr(emb), ids.numel(), E, ld, keep, seed & 0xFFFFFFFF, first_row, ptr(out), stream_of(emb)),
               "macx_embed_lookup")
    return out


def k_embed_bwd(ids, dx, E, V, keep, seed, first_row):
    d_emb = torch.empty((V, E), dtype=torch.float32, device=dx.device)
    _lib.check(_L().macx_embed_lookup_bwd(ptr(ids), ptr(dx), ids.numel(), E, dx.shape[1], V, keep, seed & 0xFFFFFFFF, first_row,
                                          ptr(d_emb), stream_of(dx)), "macx_embed_lookup_bwd")
    return d_emb


def k_wgrad(x2, g2):
    """dW [K, n] = x2^T g2 (fixed-order split reduction)."""
    L = _L()
    rows, K = x2.shape
    n = g2.shape[1]
    Kp, np_ = _pad128(K), _pad128(n)
    if Kp != K or np_ != n:                       # widths off the 128-column granule: zero-padded operands, the padding dropped
        pad = torch.nn.functional.pad
        return k_wgrad(pad(x2, (0, Kp - K)).contiguous(), pad(g2, (0, np_ - n)).contiguous())[:K, :n].contiguous()
    dW = torch.empty((K, n), dtype=torch.float32, device=g2.device)
    ws = torch.empty(L.macx_wgrad_splits(rows, K, n) * K * n, dtype=torch.float32, device=g2.device)
    _lib.check(L.macx_wgrad(ptr(x2), K, ptr(g2), n, rows, K, n, ptr(dW), ptr(ws), stream_of(g2)), "macx_wgrad")
    return dW


# -------------------------------------------------------------------------------------------------------------------
# the rules of the primitives both stacks run -- the eager autograd nodes below and the plan's executor (plan._Exec) --
# stated once, on the kernel calls above (looked up in this module's globals at call time: a test's swap reaches both stacks).
# Tensors arrive contiguous; a gradient nobody wants is None and launches nothing.
# -------------------------------------------------------------------------------------------------------------------
def mid_of(bmode, a):
    """the middle extent macx_op_binary spreads b over: a's second-to-last axis under B_MID, 1 otherwise"""
    return a.shape[-2] if (bmode == B_MID and a.dim() >= 2) else 1


def big_of(x):
    """(B, N) when [B, N <= 1024, K] takes the knowledge-base GEMM (macx_h2_gemm), None for macx_linear"""
    return (x.shape[0], x.shape[1]) if (x.dim() == 3 and x.shape[1] <= 1024) else None


def bin_bwd(op, bmode, scale, g, a, b, mid, inner, want_a, want_b):
    """backward of scale * (a op b), b spread over a by `bmode` -> (da, db); db summed over the spread, in b's shape"""
    if op == OP_ADD:
        full = g if scale == 1.0 else k_binary(OP_ADD, B_SAME, g, torch.zeros_like(g), 1, inner, scale)
        da = full if want_a else None
    else:
        da = k_binary(OP_MUL, bmode, g, b, mid, inner, scale) if want_a else None
        full = k_binary(OP_MUL, B_SAME, g, a, 1, inner, scale) if want_b else None
    if not want_b:
        return da, None
    n = g.numel()
    if bmode == B_SAME:
        db = full
    elif bmode == B_MID:
        db = k_reduce(R_MID, full, n // (mid * inner), mid, inner)
    elif bmode == B_CHANNEL:
        db = k_reduce(R_ROWS, full, n // inner, 1, inner)
    else:
        db = k_reduce(R_LAST, full, n // inner, 1, inner)
    return da, db.reshape(b.shape)


def linear_fwd(x, W, b):
    """x W (+ b) over the last axis -> (y, big); `big` goes back into linear_bwd"""
    K, n = W.shape
    big = big_of(x)
    return k_matmul(x.reshape(-1, K), W, b, big).reshape(x.shape[:-1] + (n,)), big


def linear_bwd(x, W, g, big, want_x, want_W, want_b):
    """-> (dx, dW, db): backward-data on the forward's route, macx_wgrad, a fixed-order column sum"""
    K, n = W.shape
    g2 = g.reshape(-1, n)
    dx = k_matmul(g2, W.t().contiguous(), None, big).reshape(x.shape) if want_x else None
    dW = k_wgrad(x.reshape(-1, K), g2) if want_W else None
    db = k_reduce(R_ROWS, g2, g2.shape[0], 1, n) if want_b else None
    return dx, dW, db


def act_bwd(code, x, alpha, g, want_alpha):
    """-> (dx, dalpha); dalpha: the PReLU slope's per-element gradient summed over the rows"""
    dx, de = k_act_bwd(code, x, alpha, g)
    inner = x.shape[-1]
    dalpha = k_reduce(R_ROWS, de, x.numel() // inner, 1, inner) if (de is not None and want_alpha) else None
    return dx, dalpha


def act_code(name, relu):
    """config.py's activation name -> macx_op_act code; "RELU" is whatever --relu (`relu`) selects, ACT_PRELU for PRM, and
    raises what ops.relu raises (ops.py:161-187): reluAlpha's flag is commented out, SELU has no branch"""
    if name != "RELU":
        return _lib.ACT[name]
    if relu == "LKY":
        raise AttributeError("'Config' object has no attribute 'reluAlpha'")
    if relu == "SELU":
        raise UnboundLocalError("local variable 'output' referenced before assignment")
    return {"STD": _lib.ACT["RELU"], "ELU": _lib.ACT["ELU"], "PRM": ACT_PRELU}[relu]


# -------------------------------------------------------------------------------------------------------------------
# autograd nodes: forward and backward are the kernels and rules above
# -------------------------------------------------------------------------------------------------------------------
class _Binary(torch.autograd.Function):
    """out = scale * (a op b); b broadcast by `bmode` (macx_op_binary).  a: [..., mid, inner] contiguous."""

    @staticmethod
    def forward(ctx, a, b, op, bmode, scale):
        a, b = _dev(a), _dev(b)
        mid, inner = mid_of(bmode, a), a.shape[-1]
        ctx.meta = (op, bmode, scale, mid, inner)
        ctx.save_for_backward(a, b)
        return k_binary(op, bmode, a, b, mid, inner, scale)

    @staticmethod
    def backward(ctx, g):
        op, bmode, scale, mid, inner = ctx.meta
        a, b = ctx.saved_tensors
        da, db = bin_bwd(op, bmode, scale, g.contiguous(), a, b, mid, inner, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return da, db, None, None, None


class _Act(torch.autograd.Function):
    """ops.activations / ops.relu (ops.py:161-187) on macx_op_act; PRELU carries a per-channel alpha."""

    @staticmethod
    def forward(ctx, x, act, alpha):
        x = _dev(x)
        al = _dev(alpha) if alpha is not None else None
        ctx.act = act
        ctx.save_for_backward(x, al)
        return k_act(act, x, al)

    @staticmethod
    def backward(ctx, g):
        x, al = ctx.saved_tensors
        dx, dal = act_bwd(ctx.act, x, al, g.contiguous(), ctx.needs_input_grad[2])
        return dx, None, dal


class _Dropout(torch.autograd.Function):
    """tf.nn.dropout on the stateless stream: x / keep * mask(seed, site, step, first + i) (macx_op_dropout)."""

    @staticmethod
    def forward(ctx, x, seed, site, step, keep, first):
        ctx.meta = (seed, site, step, keep, first)
        return k_dropout(_dev(x), seed, site, step, keep, first)

    @staticmethod
    def backward(ctx, g):
        return (k_dropout(g.contiguous(), *ctx.meta),) + (None,) * 5


class _Linear(torch.autograd.Function):
    """y = x W + b over the last axis (ops.multiply + bias, ops.py:50-58, 320-323): macx_h2_gemm / macx_linear forward and
    backward-data, macx_wgrad for dW, a fixed-order column sum for db."""

    @staticmethod
    def forward(ctx, x, W, b):
        x, W = _dev(x), _dev(W)
        y, ctx.big = linear_fwd(x, W, _dev(b) if b is not None else None)
        ctx.save_for_backward(x, W)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        return linear_bwd(x, W, g.contiguous(), ctx.big, *ctx.needs_input_grad)


class _Embed(torch.autograd.Function):
    """tf.nn.embedding_lookup(concat([zeros(1, E), emb]), ids) + tf.nn.dropout (model.py:207-219, ops.py:812/880):
    macx_embed_lookup forward, macx_embed_lookup_bwd (one workgroup per vocabulary row, fixed order) backward."""

    @staticmethod
    def forward(ctx, ids, emb, ld, keep, seed, first_row):
        emb = _dev(emb, "emb")
        _require_device(ids, "questions")
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        ctx.save_for_backward(ids)
        ctx.meta = (emb.shape[0], emb.shape[1], keep, seed, first_row)
        return k_embed(ids, emb, emb.shape[1], ld, keep, seed, first_row)

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        V, E, keep, seed, first_row = ctx.meta
        return None, k_embed_bwd(ids, g.contiguous(), E, V, keep, seed, first_row), None, None, None, None


# -------------------------------------------------------------------------------------------------------------------
# variables under the reference's names
# -------------------------------------------------------------------------------------------------------------------
class ScopeNames:
    """TF variable scopes, names only: `with names("a"):` is tf.variable_scope("a"); default=True is
    tf.variable_scope(None, default_name=name) -- `name`, then `name_1`, ... within one opening of the enclosing scope (ops.py:163;
    the counts of a scope's children reset when it closes, as in TF).  The variable store below and the plan's compiler
    (plan._Emitter) both name their variables through one of these."""

    def __init__(self):
        self.stack, self.opened = [], {}          # opened: full scope name -> times opened

    @contextmanager
    def __call__(self, name, default=False):
        if default:
            base = "/".join(self.stack + [name])
            if self.opened.get(base, 0):
                k = 1
                while self.opened.get("%s_%d" % (base, k), 0):
                    k += 1
                name = "%s_%d" % (name, k)
        self.stack.append(name)
        full = "/".join(self.stack)
        self.opened[full] = self.opened.get(full, 0) + 1
        try:
            yield
        finally:
            self.stack.pop()
            for key in [k for k in self.opened if k.startswith(full + "/")]:
                self.opened[key] = 0

    def full(self, leaf):
        return "/".join(self.stack + [leaf])


class GenericParams(torch.nn.Module):
    """name -> Parameter, created on first use with the reference's initialisers (xavier-uniform weights ops.py:20, zero
    biases ops.py:40, N(0,1) state variables mac_cell.py:498-499, 0.25 PReLU slopes ops.py:172)."""

    def __init__(self, device=None, generator=None):
        super().__init__()
        self.device = device
        self.gen = generator
        self.table = torch.nn.ParameterDict()
        self.names = {}               # reference name -> ParameterDict key
        self.scopes = ScopeNames()

    def scope(self, name, default=False):
        """tf.variable_scope(name); default=True: tf.variable_scope(None, default_name=name) (ScopeNames)"""
        return self.scopes(name, default)

    def get(self, name, shape, init):
        """the variable `name` of the open scope"""
        return self.ensure(self.scopes.full(name), shape, init)

    def ensure(self, key, shape, init):
        """the variable `key` (a complete scope path), created with `init` unless it exists (a loaded checkpoint)"""
        shape = tuple(shape)
        if key not in self.names:
            if init == "xavier":
                fan_in, fan_out = (shape[0], shape[0]) if len(shape) == 1 else (shape[-2], shape[-1])
                lim = math.sqrt(6.0 / (fan_in + fan_out))
                t = (torch.rand(shape, generator=self.gen, dtype=torch.float64) * 2 - 1) * lim
            elif init == "zeros":
                t = torch.zeros(shape, dtype=torch.float64)
            elif init == "normal":
                t = torch.randn(shape, generator=self.gen, dtype=torch.float64)
            else:
                t = torch.full(shape, float(init), dtype=torch.float64)
            self._add(key, t.to(torch.float32))
        v = self.table[self.names[key]]
        if tuple(v.shape) != shape:
            raise ValueError("variable %s has shape %s, expected %s" % (key, tuple(v.shape), shape))
        return v

    def _apply(self, fn, *a, **kw):
        """.to(device) / .cuda() on this module or on any module that holds it: variables created later follow."""
        out = super()._apply(fn, *a, **kw)
        held = self.tensors()
        if held:
            self.device = held[0].device
        else:
            try:
                probe = torch.empty(0, device=self.device) if self.device is not None else torch.empty(0)
                self.device = fn(probe).device
            except Exception:          # noqa: BLE001 -- keep the device
                pass
        return out

    def _add(self, key, t):
        mangled = "v%d" % len(self.names)
        self.names[key] = mangled
        self.table[mangled] = torch.nn.Parameter(t.to(self.device) if self.device is not None else t)

    def tensors(self):
        return [self.table[m] for m in self.names.values()]

    def to_reference_dict(self):
        return {k: self.table[m].detach().clone() for k, m in self.names.items()}

    def grads_by_name(self):
        return {k: self.table[m].grad for k, m in self.names.items()}

    @torch.no_grad()
    def load_reference_dict(self, ref):
        """Adopt {TF variable name: array} (names with or without a leading 'macModel/' and a trailing ':0')."""
        for k, v in ref.items():
            k = k[len("macModel/"):] if k.startswith("macModel/") else k
            k = k[:-2] if k.endswith(":0") else k
            t = torch.as_tensor(v).detach().to(torch.float32)
            if k in self.names:
                self.table[self.names[k]].copy_(t.reshape(self.table[self.names[k]].shape))
            else:
                self._add(k, t.clone())
        return self


class ParamsUnit:
    """Mixin of the modules that keep their variables in a GenericParams at self.params (GenericQuestionEncoder,
    GenericOutputClassifier): what they show of it."""

    def tensors(self):
        return self.params.tensors()

    def to_reference_dict(self):
        return self.params.to_reference_dict()

    def load_reference_dict(self, ref):
        own = set(self.params.names)
        self.params.load_reference_dict({k: v for k, v in ref.items() if k in own})
        return self

    def to(self, *a, **kw):
        out = super().to(*a, **kw)
        t = self.params.tensors()
        self.params.device = t[0].device if t else self.params.device
        return out


# -------------------------------------------------------------------------------------------------------------------
# eager layer helpers for the generic question encoder and output unit (encoder.py, output.py): a dense layer of the
# "linearLayer<name>" family and the activation table, on the autograd nodes above
# -------------------------------------------------------------------------------------------------------------------
class _Ops:
    def __init__(self, config, store):
        self.config, self.vs = config, store

    def g(self, name):
        return get(self.config, name)

    def getWeight(self, shape):
        with self.vs.scope("weights"):
            return self.vs.get("weight", shape, "xavier")

    def getBias(self, shape):
        with self.vs.scope("biases"):
            return self.vs.get("bias", shape, "zeros")

    def act(self, name, x):
        """config.py's activation names on macx_op_act; "RELU" is whatever --relu selects (ops.py:161-187)"""
        if name == "NON":
            return x
        code, alpha = act_code(name, self.g("relu")), None
        if code == ACT_PRELU:
            with self.vs.scope("prelu", default=True):
                alpha = self.vs.get("alpha", (x.shape[-1],), 0.25)
        return _Act.apply(x, code, alpha)

    def linear(self, inp, inDim, outDim, dropout=None, act="NON", name=""):
        """[.., inDim] -> [.., outDim] under "linearLayer<name>" (ops.py:298-333): input dropout, x W + b, activation and -- with an
        activation -- the stacked "<name>_2" layer.  (Widths of 1 and constant bias offsets only occur inside the cell: plan.py.)"""
        with self.vs.scope("linearLayer" + name):
            W, b = self.getWeight((inDim, outDim)), self.getBias((outDim,))
            y = self.act(act, _Linear.apply(dropout(inp) if dropout is not None else inp, W, b))
            return y if act == "NON" else self.linear(y, outDim, outDim, name=name + "_2")


# -------------------------------------------------------------------------------------------------------------------
# the cell (the interface of mac_cell.py:30-592 over a compiled plan)
# -------------------------------------------------------------------------------------------------------------------
class GenericMACCell:
    """Same constructor / zero_state / __call__ / attribute surface as mac_cell.MACCell and macx.MACCell; built by
    macx.MACCell(...) when the option set has no fused kernels.  zero_state and every step execute one segment of the plan
    compiled from the option set (plan.compile_cell) -- one autograd node each."""

    generic = True

    def __init__(self, vecQuestions, questionWords, questionCntxWords, questionLengths, knowledgeBase,
                 memoryDropout, readDropout, writeDropout, batchSize, train, reuse=None, *, config=None, params=None,
                 netLength=None, seed=None, b0=0, mask_word=None, tune=None, kb_lengths=None):
        del tune            # (the A/B hooks of macx_opts.tune select among FUSED kernels; this path has one kernel per op)
        self.mask_word = _mask_word(mask_word, knowledgeBase)
        # live cells per question: the read unit's softmax of the plan then runs behind the length mask (plan.compile_cell)
        self.kb_lengths = _kb_lengths(kb_lengths, knowledgeBase.shape[0])
        self.config = config if config is not None else SimpleNamespace()
        reject_like_reference(self.config)
        bad = [k for k in ("memDim", "ctrlDim", "attDim") if self.g(k) % 4]
        if bad:
            raise UnsupportedOptions("the generic path needs %s %% 4 == 0 (16-byte rows; widths off the 128-column granule of the "
                                     "product kernels run zero-padded inside them)" % bad[0])
        _L()                                           # fails loudly without libmacx.so
        _require_device(questionLengths, "questionLengths")
        lengths = questionLengths.to(torch.int32).contiguous()
        if lengths.shape != (vecQuestions.shape[0],):
            raise ValueError("questionLengths must be [batchSize]")
        self.train, self.batchSize, self.b0, self.reuse = bool(train), int(batchSize), int(b0), reuse
        # the reference's attribute names (mac_cell.py:59-79), device-checked fp32 tensors
        self.__dict__.update(vecQuestions=_dev(vecQuestions, "vecQuestions"), questionWords=questionWords,
                             questionCntxWords=questionCntxWords, questionLengths=lengths,
                             knowledgeBase=_dev(knowledgeBase, "knowledgeBase"))
        rates = dict(memory=memoryDropout, read=readDropout, write=writeDropout)
        self.dropouts = {k: (float(v) if self.train else 1.0) for k, v in rates.items()}      # evaluation feeds keep = 1 (model.py:118-125)
        self.netLength = int(netLength if netLength is not None else self.g("netLength"))
        self.seed = fresh_seed(seed, self.train) & 0xFFFFFFFF
        dev = self.knowledgeBase.device
        self.params = params if params is not None else GenericParams(device=dev)
        self.none = torch.zeros((self.batchSize, 1), dtype=torch.float32, device=dev)
        self.iteration = 0
        self._plan = self._exec = None

    def g(self, name):
        return get(self.config, name)

    @property
    def state_size(self):
        return MACCellTuple(self.g("ctrlDim"), self.g("memDim"))

    @property
    def output_size(self):
        return 1

    def plan(self):
        """the compiled plan of this option set (first call: compiles it and creates the variables it names, in its order --
        the reference's creation order -- unless a checkpoint already put them into `params`)"""
        if self._plan is None:
            from . import plan as _plan
            self._plan = _plan.compile_cell(self.config, self.netLength, kb_lengths=self.kb_lengths is not None)
            for name, spec in self._plan.variables.items():
                self.params.ensure(name, spec.shape, spec.init)
        return self._plan

    def _segment(self, seg, feeds):
        from . import plan as _plan
        if self._exec is None:
            self._exec = _plan._Exec(self.seed, self.b0, self.dropouts, self.train, self.batchSize, self.knowledgeBase.device,
                                     mask_word=self.mask_word)
        return _plan.run_segment(seg, self._exec, feeds, self.params)

    # histories as the reference exposes them: [B, steps + 1, d] (mac_cell.py:472-474, 549-551)
    controls = property(lambda self: torch.stack(self._hist["control"], dim=1))
    memories = property(lambda self: torch.stack(self._hist["memory"], dim=1))
    infos = property(lambda self: torch.stack(self._hist["info"], dim=1))

    # ---- zero_state (mac_cell.py:539-592)
    def zero_state(self, batchSize=None, dtype=torch.float32):
        if batchSize is not None and int(batchSize) != self.batchSize:
            raise ValueError("zero_state(%d) on a cell built for batchSize %d" % (batchSize, self.batchSize))
        words = _dev(self.questionCntxWords if self.g("controlContextual") else self.questionWords, "question words")
        out = self._segment(self.plan().init, {"vecQuestions": self.vecQuestions, "words": words})
        self._carry = {k: out[k] for k in ("in_words", "out_words", "mem_mask") if k in out}
        self._carry["cont_control"] = out["control"]
        self._hist = {"control": [out["control"]], "memory": [out["memory"]], "info": [out["memory"]]}
        self.attentions = {"kb": [], "question": [], "self": [], "gate": []}
        self.contControl = out["control"]
        self.iteration = 0
        return MACCellTuple(out["control"], out["memory"])

    # ---- one step (mac_cell.py:420-480)
    def __call__(self, inputs, state, scope=None):
        if scope not in (None, "MACCell"):
            raise UnsupportedOptions("the plan names the cell's variables under MACnetwork/MACCell (model.py:453-458 passes no scope)")
        seg = self.plan().steps[int(self.iteration)]
        have = {"vecQuestions": self.vecQuestions, "knowledgeBase": self.knowledgeBase, "lengths": self.questionLengths,
                "kb_lengths": self.kb_lengths, "control": state.control, "memory": state.memory, **self._carry}
        if "controls" in seg.feeds:
            have["controls"], have["memories"] = self.controls, self.memories
        out = self._segment(seg, {k: have[k] for k in seg.feeds})
        self._carry["cont_control"] = self.contControl = out["cont_control"]
        for key, name in (("question", "att_question"), ("kb", "att_kb"), ("self", "att_self"), ("gate", "att_gate")):
            if name in out:
                self.attentions[key].append(out[name])
        for key in ("control", "memory", "info"):
            self._hist[key].append(out[key])
        return self.none, MACCellTuple(out["control"], out["memory"])

    # ---- the units on their own, with the reference's method signatures (mac_cell.py:133, 209, 305): each call compiles (once)
    #      and runs the unit's segment of the plan for the current `iteration`; attentions are appended like in a step
    def _unit(self, which, feeds):
        from . import plan as _plan
        key = (which, int(self.iteration))
        cache = self.__dict__.setdefault("_unit_plans", {})
        if key not in cache:
            cache[key] = _plan.compile_unit(self.config, which, int(self.iteration))
            for name, spec in cache[key].variables.items():
                self.params.ensure(name, spec.shape, spec.init)
        seg = cache[key].init
        have = dict(feeds, lengths=self.questionLengths, **getattr(self, "_carry", {}))
        if "controls" in seg.feeds:
            have["controls"], have["memories"] = self.controls, self.memories
        out = self._segment(seg, {k: have[k] for k in seg.feeds})
        for k, name in (("question", "att_question"), ("kb", "att_kb"), ("self", "att_self"), ("gate", "att_gate")):
            if name in out:
                self.attentions[k].append(out[name])
        return out

    def control(self, controlInput, inWords, outWords, questionLengths, control, contControl=None, name=""):
        out = self._unit("control", {"control_input": controlInput, "in_words": inWords, "out_words": outWords, "control": control,
                                     "cont_control": contControl})
        return out["control"], out["cont_control"]

    def read(self, knowledgeBase, memory, control, name=""):
        return self._unit("read", {"knowledgeBase": knowledgeBase, "memory": memory, "control": control})["info"]

    def write(self, memory, info, control, contControl=None, name=""):
        return self._unit("write", {"memory": memory, "info": info, "control": control, "cont_control": contControl})["memory"]

    inWords = property(lambda self: self._carry["in_words"])
    outWords = property(lambda self: self._carry["out_words"])

    # ---- MACCell's run-status interface: this path has one kernel per op and no hand-offs inside a launch, so nothing can time out
    def status(self):
        return (0, -1)

    def check(self):
        return None

    def reset_status(self):
        return None

    # ---- the loop of model.py:453-458
    def run(self):
        state = self.zero_state(self.batchSize)
        for i in range(self.netLength):
            self.iteration = i
            _, state = self(self.none, state)
        return state
