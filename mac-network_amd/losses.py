"""Losses on a run's attention maps as ONE launch (macx_att_loss, include/macx.h): attention supervision against a target
distribution over the knowledge-base cells or the question words, and entropy regularisers on the maps.

    att = cell.state_tensor("att_kb")                                     # [p, B, N] with the autograd edge (cell.MACCell)
    rows = macx.losses.attention_loss(att, target, lengths=kb_lengths, row_weights=supervised, scale=lam / (p * B))
    (ce + rows.sum()).backward()

The kernel writes the loss rows [p, B] and the gradient d_att [p, B, n] together; the backward pass hands d_att, times the incoming
row gradient, to the cell's own backward pass (macx_cell_backward_x).  Lengths and weights are device tensors the kernel reads when
it runs, so the call is capturable: the captured training steps of graph.py issue it between their forward and backward launches
(`att_loss=`).  No CPU path: a tensor that is not on the HIP device raises."""
import math

import torch

from . import _lib

KINDS = _lib.ATT_LOSS_KINDS


def _device_f32(t, name, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("%s must be a float32 tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the HIP device: the attention loss has no CPU path" % name)
    if shape is not None and tuple(t.shape) not in shape:
        raise ValueError("%s must be %s, got %s" % (name, " or ".join(str(list(s)) for s in shape), list(t.shape)))
    return t.detach().contiguous()


def check_scalars(kind, eps, scale):
    """the by-value arguments, validated as the export validates them (and before anything asks for the device)"""
    if kind not in KINDS:
        raise ValueError("kind = %r: the attention loss is one of %s" % (kind, sorted(KINDS)))
    eps, scale = float(eps), float(scale)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError("eps = %r: the loss takes log(a + eps), eps must be positive and finite" % (eps,))
    if not math.isfinite(scale):
        raise ValueError("scale = %r must be finite" % (scale,))
    return KINDS[kind], eps, scale


def launch(att, target, lengths, step_weights, row_weights, kind, eps, scale, rows, d_att):
    """macx_att_loss on torch's current stream.  Every tensor is a contiguous device tensor of the export's layout (or None where the
    export takes NULL); kind is the export's integer.  What graph.CapturedDPTrainStep captures, and the body of attention_loss."""
    p, B, n = att.shape
    ptr = _lib.ptr
    code = _lib.lib().macx_att_loss(ptr(att), ptr(target), ptr(lengths), ptr(step_weights), ptr(row_weights), p, B, n, int(kind),
                                    int(target is not None and target.dim() == 3), float(eps), float(scale), ptr(rows), ptr(d_att),
                                    _lib.stream_of(att))
    _lib.check(code, "macx_att_loss")


class _AttentionLoss(torch.autograd.Function):
    """macx_att_loss: rows and d_att from one launch; the backward pass returns the stored d_att times the incoming row gradient
    (output._AnswerLoss's pattern).  rows_out: None, or a [p, B] tensor the rows are written INTO -- the function returns a tensor of
    its own on that memory (cell._Run.segment's alias), so a caller's static buffer never becomes an autograd result itself."""

    @staticmethod
    def forward(ctx, att, target, lengths, step_weights, row_weights, kind, eps, scale, rows_out):
        a = _device_f32(att, "att", None)
        p, B, n = a.shape
        if rows_out is None:
            rows = torch.empty(p, B, dtype=torch.float32, device=a.device)
        else:
            rows = torch.empty(0, dtype=torch.float32, device=a.device).set_(rows_out.untyped_storage(), rows_out.storage_offset(), (p, B))
        d_att = torch.empty_like(a)
        launch(a, target, lengths, step_weights, row_weights, kind, eps, scale, rows, d_att)
        ctx.save_for_backward(d_att)
        return rows

    @staticmethod
    def backward(ctx, g_rows):
        (d_att,) = ctx.saved_tensors
        return (d_att * g_rows.unsqueeze(-1),) + (None,) * 8


def attention_loss(att, target=None, lengths=None, step_weights=None, row_weights=None, kind="ce", eps=1e-8, scale=1.0, _rows_out=None):
    """Loss rows [p, B] of a stacked attention map `att` [p, B, n] (MACCell.state_tensor("att_kb" | "att_question")), differentiable
    with respect to att.  With w = scale * step_weights[i] * row_weights[b] and L = lengths[b] clamped to [1, n]:
      kind "ce"       rows[i, b] = -w sum_{j<L} target[j] log(att[j] + eps); target [B, n] (every step) or [p, B, n] (per step)
      kind "entropy"  rows[i, b] =  w sum_{j<L} att[j] log(att[j] + eps): the negative entropy (scale's sign chooses); no target
    lengths: None (all n) or a [B] integer device tensor (the cell's kb_lengths / questionLengths): cells j >= L are not read and
    receive a zero gradient.  step_weights [p], row_weights [B]: None (1) or float32 device tensors; a row_weights[b] of 0 makes
    question b unsupervised -- an exactly zero row and gradient, whatever its target holds.  target, lengths and the weights are
    data: no gradient flows to them.  No CPU path."""
    code, eps, scale = check_scalars(kind, eps, scale)
    if not torch.is_tensor(att) or att.dim() != 3:
        raise ValueError("att must be a [p, B, n] tensor (MACCell.state_tensor)")
    if not att.is_cuda:
        raise RuntimeError("att must live on the HIP device: the attention loss has no CPU path")
    p, B, n = att.shape
    if (target is None) != (kind != "ce"):
        raise TypeError('kind "ce" needs a target distribution' if target is None else 'kind "entropy" takes no target')
    if target is not None:
        target = _device_f32(target, "target", ((B, n), (p, B, n)))
    if lengths is not None:
        if not torch.is_tensor(lengths) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool or tuple(lengths.shape) != (B,):
            raise ValueError("lengths must be a [%d] integer tensor" % B)
        if not lengths.is_cuda:
            raise RuntimeError("lengths must live on the HIP device: the attention loss has no CPU path")
        lengths = lengths.to(torch.int32).contiguous()
    if step_weights is not None:
        step_weights = _device_f32(step_weights, "step_weights", ((p,),))
    if row_weights is not None:
        row_weights = _device_f32(row_weights, "row_weights", ((B,),))
    return _AttentionLoss.apply(att, target, lengths, step_weights, row_weights, code, eps, scale, _rows_out)
