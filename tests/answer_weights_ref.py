"""The weighted answer loss (macx_answer_loss_weighted, include/macx.h) restated in fp64 torch, and the padding rule of a short batch
on the captured tower classes as a pure function.  Shared by tests/test_answer_weights_host.py and tests/test_gpu_answer_weights.py."""
import torch


def live(weights, B):
    """[B] bool: question b counts iff weights[b] > 0 (0, negative and NaN weights are weight 0); None = all ones"""
    return torch.ones(B, dtype=torch.bool) if weights is None else weights > 0


def effective(weights, B):
    """[B] fp64 weights with every dead question at exactly 0"""
    w = torch.ones(B, dtype=torch.float64) if weights is None else weights.to(torch.float64)
    return torch.where(live(weights, B), w, torch.zeros_like(w))


def reference(logits, answers, weights=None, grad_scale=1.0):
    """fp64: dict(rows [B], pred [B] int64, dlogits [B, A], loss, sums = (sum w l, sum w [pred == answer], W)) of the contract.
    Dead rows are masked BEFORE anything is computed from them, as the kernel leaves before it loads them: they may hold NaN logits
    and labels out of range.  Live labels must be in range."""
    B, A = logits.shape
    on = live(weights, B)
    w = effective(weights, B)
    x = torch.where(on.unsqueeze(1), logits.to(torch.float64), torch.zeros(B, A, dtype=torch.float64))
    ans = torch.where(on, answers.long(), torch.zeros(B, dtype=torch.long))
    logp = torch.log_softmax(x, dim=1)
    rows = torch.where(on, -logp.gather(1, ans.unsqueeze(1)).squeeze(1), torch.zeros(B, dtype=torch.float64))
    pred = torch.where(on, x.argmax(dim=1), torch.full((B,), -1, dtype=torch.long))
    W = w.sum()
    share = w / W if float(W) > 0 else torch.zeros_like(w)
    onehot = torch.nn.functional.one_hot(ans, A).to(torch.float64)
    dlogits = grad_scale * share.unsqueeze(1) * (torch.softmax(x, dim=1) - onehot)
    loss = (w * rows).sum() / W if float(W) > 0 else torch.zeros((), dtype=torch.float64)
    hit = (w * (pred == ans).to(torch.float64)).sum()
    return dict(rows=rows, pred=pred, dlogits=dlogits, loss=loss, sums=(float((w * rows).sum()), float(hit), float(W)))


def sums_of(rows, pred, answers, weights):
    """the three totals of ONE call, formed in fp64 from what the call returned in fp32 / int32 (rows, pred) and read (answers,
    weights): every product w * row is exact in fp64"""
    B = rows.shape[0]
    w = effective(weights, B)
    hit = (pred.long() == answers.long()) & live(weights, B)
    return float((w * rows.to(torch.float64)).sum()), float((w * hit.to(torch.float64)).sum()), float(w.sum())


def pad_slots(t, n, B, axis=0):
    """The padding rule: a static tensor of B slots along `axis` loaded with the n <= B entries of `t` -- slots 0 .. n-1 are t, slots
    n .. B-1 copies of slot 0 (finite and in range, whatever the batch holds)."""
    assert 1 <= n <= B and t.shape[axis] == n
    first = t.narrow(axis, 0, 1)
    shape = list(t.shape)
    shape[axis] = B - n
    return torch.cat([t, first.expand(shape)], dim=axis)


def pad_weights(weights, n, B):
    """... and the static weights: the caller's (None = ones) for the n questions, 0 behind them"""
    w = torch.ones(n) if weights is None else weights.to(torch.float32)
    return torch.cat([w, torch.zeros(B - n)])
