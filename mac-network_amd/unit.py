"""What the three fused units around the cell share (stem.Stem, encoder.QuestionEncoder, output.OutputClassifier): the argument
validators, the fused-or-generic construction, the reference-name dictionaries, and the ONE autograd node around a unit's pair
of `_w` ABI calls (include/macx.h).  A leaf: it imports _lib and options only.

A unit declares, as class attributes: FIELDS (its _lib.*_FIELDS) and REF_NAMES, ABI ("stem" | "encoder" | "output" |
"rnn_encoder" -- encoder.RecurrentQuestionEncoder, whose FIELDS / REF_NAMES / PARAMS / GRADS depend on the cell and so belong to the
instance: the exports
macx_<ABI>_saved_floats / _ws_floats / _forward_w / _backward_w), SHAPES / PARAMS / GRADS (its three ctypes structs), GENERIC (the
class built for the option sets check_fused refuses), check_fused and SIZE_ERROR (the ValueError text of a `saved` size of 0).
Its forward() validates, builds the shapes struct and hands over to self._call; two hooks say what differs between the units:

    _outputs(sh, inputs)   -> (outputs, X): the tensors the forward call writes, and the ones the backward call reads behind
                              the params struct (the stem reads its OUTPUT there, the other two their inputs)
    _backward(sh, X, d_outs) -> (d, extra, d_inputs): the incoming gradients in front of the grads struct, the tensors behind
                              it, and the gradient returned for each input

so that the two argument lists are
    forward:   (shapes, *scalars, seed, params) + inputs + outputs + (saved, n_saved, word, stream)
    backward:  (shapes, *scalars, seed, params) + X + (saved, n_saved, ws, n_ws) + d + (grads,) + extra + (word, stream)
tests/test_unit_contract_host.py holds both to the header's prototypes, position by position."""
import ctypes as C
import math

import torch

from . import _lib
from .options import UnsupportedOptions, fresh_seed


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the HIP device: the MAC cell has no CPU path" % name)
    return t.contiguous()


def _kb_lengths(t, batch):
    """kb_lengths: None, or an integer tensor [batch] on the device -> contiguous int32 (what questionLengths goes through)"""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("kb_lengths must be an integer tensor")
    if not t.is_cuda:
        raise RuntimeError("kb_lengths must live on the HIP device: the MAC cell has no CPU path")
    if t.shape != (batch,):
        raise ValueError("kb_lengths must be [batchSize]")
    return t.to(torch.int32).contiguous()


def _mask_word(t, like):
    """macx_dropout.mask_word: one 32-bit word in device memory (an int32 / uint32 tensor with one element), or None."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.numel() != 1 or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
        raise TypeError("mask_word must be a 1-element int32 tensor on the HIP device (the kernels read it when they run)")
    if t.device != like.device:
        raise ValueError("mask_word lives on %s, the cell on %s" % (t.device, like.device))
    return t


def require_device(t, what):
    """the fused units' one device check; what: "the stem" | "the question encoder" | "the output unit" """
    if not t.is_cuda:
        raise RuntimeError("%s has no CPU path" % what)


def refuse_mask_word(mask_word, unit, call, generic=None):
    """what a generic module's forward() does first, before any device check: only the fused units take a run's mask word"""
    if mask_word is not None:
        raise UnsupportedOptions("%s: a run's mask word is taken by the fused %s only (%s); the generic %s has no such path"
                                 % (unit, unit, call, generic or unit))


def xavier_uniform(shape, fan_sum, generator=None):
    """xavier-uniform (ops.py:18-33) drawn in fp64: U(-1, 1) * sqrt(6 / (fan_in + fan_out)), as float32"""
    return ((torch.rand(shape, generator=generator, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / fan_sum)).float()


class _FusedCall(torch.autograd.Function):
    """macx_<ABI>_forward_w / macx_<ABI>_backward_w of one fused unit.  scalars: the calls' scalar head behind the shapes struct
    (act, keep | keep_input, keep_question); word: the run's mask word (1-element int32 device tensor) or None == NULL == word 0;
    tensors: the unit's inputs, then its parameters in FIELDS order."""

    @staticmethod
    def forward(ctx, mod, sh, scalars, seed, word, *tensors):
        L = _lib.lib()
        n_in = len(tensors) - len(mod.FIELDS)
        inputs, params = tuple(t.contiguous() for t in tensors[:n_in]), tensors[n_in:]
        saved_floats, _, forward_w, _ = mod.EXPORTS
        n_saved = getattr(L, saved_floats)(C.byref(sh))
        if n_saved == 0:
            raise ValueError(mod.SIZE_ERROR)
        dev = inputs[0].device
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev)
        outputs, X = mod._outputs(sh, inputs)
        ps = mod.PARAMS(*[p.data_ptr() for p in params])
        _lib.check(getattr(L, forward_w)(C.byref(sh), *scalars, seed & 0xFFFFFFFF, C.byref(ps), *[t.data_ptr() for t in inputs + outputs],
                                         saved.data_ptr(), n_saved, _lib.ptr(word), _lib.stream_of(dev)), forward_w)
        ctx.stuff = (mod, sh, scalars, seed, word, X, params, saved, n_saved)
        if torch.cuda.is_current_stream_capturing():
            # under no_grad nothing holds `saved` once this call returns; inside a capture its block must not go back to the graph's
            # pool, where a later buffer that is written from OUTSIDE the graph (the cell's sticky status words) could land on it
            mod._capture_keep = saved
        return outputs[0] if len(outputs) == 1 else outputs

    @staticmethod
    def backward(ctx, *d_outs):
        mod, sh, scalars, seed, word, X, params, saved, n_saved = ctx.stuff
        L = _lib.lib()
        _, ws_floats, _, backward_w = mod.EXPORTS
        dev = saved.device
        n_ws = getattr(L, ws_floats)(C.byref(sh))
        ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        grads = [torch.empty_like(p) for p in params]
        gs = mod.GRADS(*[g.data_ptr() for g in grads])
        ps = mod.PARAMS(*[p.data_ptr() for p in params])
        d, extra, d_inputs = mod._backward(sh, X, d_outs)
        _lib.check(getattr(L, backward_w)(C.byref(sh), *scalars, seed & 0xFFFFFFFF, C.byref(ps), *[t.data_ptr() for t in X], saved.data_ptr(),
                                          n_saved, ws.data_ptr(), n_ws, *[t.data_ptr() for t in d], C.byref(gs),
                                          *[t.data_ptr() for t in extra], _lib.ptr(word), _lib.stream_of(dev)),    # (the forward pass's word)
                   backward_w)
        grads = mod._param_grads(grads)
        return (None,) * (len(ctx.needs_input_grad) - len(d_inputs) - len(grads)) + tuple(d_inputs) + tuple(grads)


class FusedUnit(torch.nn.Module):
    """Base of Stem, QuestionEncoder and OutputClassifier (the contract: this module's docstring).  Constructing a unit for an
    option set its check_fused refuses returns its GENERIC class: the same interface on one HIP kernel per reference op."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        if "ABI" in vars(cls):
            cls.EXPORTS = tuple("macx_%s_%s" % (cls.ABI, s) for s in ("saved_floats", "ws_floats", "forward_w", "backward_w"))

    def __new__(cls, config=None, *args, **kw):
        if "ABI" in vars(cls) and config is not None:          # (the fused class itself, not a class derived from it)
            try:
                cls.check_fused(config)
            except UnsupportedOptions:
                return cls.GENERIC(config, *args, **kw)
        return super().__new__(cls)

    def tensors(self):
        return [getattr(self, f) for f in self.FIELDS]

    def to_reference_dict(self):
        return {self.REF_NAMES[f]: getattr(self, f).detach().clone() for f in self.FIELDS}

    def load_reference_dict(self, d):
        with torch.no_grad():
            for f in self.FIELDS:
                getattr(self, f).copy_(torch.as_tensor(d[self.REF_NAMES[f]]))

    def _call(self, sh, scalars, seed, train, mask_word, *inputs):
        return _FusedCall.apply(self, sh, scalars, fresh_seed(seed, train), _mask_word(mask_word, inputs[0]), *inputs, *self.tensors())

    def _param_grads(self, grads):
        return grads
