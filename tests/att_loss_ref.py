"""Shared by tests/test_att_loss_host.py and tests/test_gpu_att_loss.py: the two attention losses of macx_att_loss (include/macx.h)
and their gradients in fp64 torch, written from the header's formulas.

    w = scale * step_weights[i] * row_weights[b],   live cells j < clamp(lengths[b], 1, n)
    ce       rows[i, b] = -w sum_j t[j] log(a[j] + eps)        d_att[i, b, j] = -w t[j] / (a[j] + eps)
    entropy  rows[i, b] =  w sum_j a[j] log(a[j] + eps)        d_att[i, b, j] =  w (log(a[j] + eps) + a[j] / (a[j] + eps))

Cells j >= L are taken out by INDEX (torch.where on the mask, never a multiplication): whatever att and target hold there -- NaN in
the tests -- reaches nothing.  eps and scale arrive as Python floats and are taken at their fp32 values, which is what the export
receives."""
import numpy as np
import torch

DT = torch.float64


def f32(x):
    """a Python float at the value the export's `float` parameter receives"""
    return float(np.float32(x))


def live_mask(lengths, B, n):
    """[B, n] bool: j < clamp(lengths[b], 1, n); lengths None: every cell"""
    if lengths is None:
        return torch.ones(B, n, dtype=torch.bool)
    L = torch.as_tensor(lengths).to(torch.int64).clamp(1, n)
    return torch.arange(n).unsqueeze(0) < L.unsqueeze(1)


def weights(p, B, step_weights, row_weights, scale):
    sw = torch.ones(p, dtype=DT) if step_weights is None else step_weights.to(DT)
    rw = torch.ones(B, dtype=DT) if row_weights is None else row_weights.to(DT)
    return f32(scale) * sw.unsqueeze(1) * rw.unsqueeze(0)                      # [p, B]


def terms(att, target, lengths, step_weights, row_weights, kind, eps, scale):
    """[p, B, n] fp64: the weighted summands of the loss rows (0 at j >= L and in rows of weight 0); att may carry an autograd edge"""
    p, B, n = att.shape
    a = att.to(DT)
    live = live_mask(lengths, B, n).unsqueeze(0).expand(p, B, n)
    w = weights(p, B, step_weights, row_weights, scale).unsqueeze(-1).expand(p, B, n)
    live = live & (w != 0)                                                     # an unsupervised row reads nothing
    safe = torch.where(live, a, torch.ones_like(a))                            # (index, not product: NaN behind the mask stays out)
    lg = torch.log(safe + f32(eps))
    if kind == "ce":
        t = target.to(DT)
        t = (t if t.dim() == 3 else t.unsqueeze(0)).expand(p, B, n)
        x = -w * torch.where(live, t, torch.zeros_like(t)) * lg
    elif kind == "entropy":
        x = w * safe * lg
    else:
        raise ValueError(kind)
    return torch.where(live, x, torch.zeros_like(x))


def rows(att, target=None, lengths=None, step_weights=None, row_weights=None, kind="ce", eps=1e-8, scale=1.0):
    """loss rows [p, B] fp64"""
    return terms(att, target, lengths, step_weights, row_weights, kind, eps, scale).sum(dim=-1)


def abs_term_sums(att, target=None, lengths=None, step_weights=None, row_weights=None, kind="ce", eps=1e-8, scale=1.0):
    """sum_j |term_j| per row [p, B]: what an fp32 summation's error bound is relative to"""
    return terms(att, target, lengths, step_weights, row_weights, kind, eps, scale).abs().sum(dim=-1)


def d_att(att, target=None, lengths=None, step_weights=None, row_weights=None, kind="ce", eps=1e-8, scale=1.0):
    """the closed-form gradient of rows.sum() with respect to att, [p, B, n] fp64; exactly 0 at j >= L and in rows of weight 0"""
    p, B, n = att.shape
    a = att.detach().to(DT)
    live = live_mask(lengths, B, n).unsqueeze(0).expand(p, B, n)
    w = weights(p, B, step_weights, row_weights, scale).unsqueeze(-1).expand(p, B, n)
    live = live & (w != 0)
    safe = torch.where(live, a, torch.ones_like(a))
    ae = safe + f32(eps)
    if kind == "ce":
        t = target.to(DT)
        t = (t if t.dim() == 3 else t.unsqueeze(0)).expand(p, B, n)
        g = -w * torch.where(live, t, torch.zeros_like(t)) / ae
    elif kind == "entropy":
        g = w * (torch.log(ae) + safe / ae)
    else:
        raise ValueError(kind)
    return torch.where(live, g, torch.zeros_like(g))


def draw(p, B, n, lengths, seed, nan=True):
    """(att [p,B,n], target [p,B,n]) fp32: softmax of N(0,1) over each question's live cells; with nan: NaN at every j >= L"""
    g = torch.Generator().manual_seed(seed)
    live = live_mask(lengths, B, n).unsqueeze(0).expand(p, B, n)
    out = []
    for _ in range(2):
        x = torch.softmax(torch.randn(p, B, n, generator=g, dtype=DT).masked_fill(~live, float("-inf")), dim=-1).to(torch.float32)
        out.append(torch.where(live, x, torch.full_like(x, float("nan"))) if nan else x)
    return out
