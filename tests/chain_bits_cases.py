"""The cases of tests/test_gpu_chain_segments.py and of its fixture generator tests/golden/make_chain_bits.py: the full cell, forward
and backward, at the smallest shapes where the chain kernels' per-question (segment) logic can go wrong.

A 64-row tile of the flat [B * N] row axis touches one, two or (N < 64) three questions; stage B0 and the dy sums of chain_bwd keep
one accumulator set per question of the tile, and the launcher picks the two-question kernel when N >= 64.

    d128_N70    tiles of 64 rows (any size, d != 512); question boundaries at row offsets 6, 12, .. inside 8-row blocks; last tile 30 rows
    d128_N64    boundaries exactly on tile edges: the N = tile rows edge of the two-question rule
    d128_N40    up to three questions per tile: the general kernel
    d512_N196   8 428 rows, the fewest that select 64-row tiles at d = 512: the flagship instantiation with its dKB fillers
The first shape also runs without read dropout (the keep bits' stand-in), with the plain ReLU as readCtrlAct (relu = STD) and with
kb_lengths that leave one live cell in one question.
"""
import hashlib

import torch

from helpers import make_case

#        id                 (B, S, N, d, p)        config overrides            kb_lengths
CASES = {
    "d128_N70":            ((5, 7, 70, 128, 2),    {},                         None),
    "d128_N70_nodrop":     ((5, 7, 70, 128, 2),    {"readDropout": 1.0},       None),
    "d128_N70_relu":       ((5, 7, 70, 128, 2),    {"relu": "STD"},            None),
    "d128_N70_lengths":    ((5, 7, 70, 128, 2),    {},                         [70, 1, 33, 70, 70]),
    "d128_N64":            ((4, 7, 64, 128, 2),    {},                         None),
    "d128_N40":            ((7, 7, 40, 128, 2),    {},                         None),
    "d512_N196":           ((43, 7, 196, 512, 2),  {},                         None),
}


def case_inputs(name):
    (B, S, N, d, p), over, kb_lengths = CASES[name]
    cfg, vq, words, lengths, kb = make_case("args", B, S, N, d, p, **over)
    if kb_lengths is not None:
        kb = kb.clone()
        for b, n in enumerate(kb_lengths):
            kb[b, n:] = 0.0
    g = torch.Generator().manual_seed(9)
    dmem, dctl = torch.randn(B, d, generator=g) / B, torch.randn(B, d, generator=g) / B
    return cfg, vq, words, lengths, kb, kb_lengths, dmem, dctl


def run_case(macx, dev, name):
    """-> (outputs {name: cpu tensor}, what the oracle needs to repeat the run)"""
    cfg, vq, words, lengths, kb, kb_lengths, dmem, dctl = case_inputs(name)
    p = cfg.netLength
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(5)).to(dev)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for f in params.fields:                      # non-zero biases: the bias paths take part
            t = getattr(params, f)
            if f.endswith("_b"):
                t.copy_((torch.rand(t.shape, generator=g) - 0.5) * 0.2)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (vq, words, kb)]
    kw = {} if kb_lengths is None else {"kb_lengths": torch.as_tensor(kb_lengths, dtype=torch.int64).to(dev)}
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=lengths.to(dev), knowledgeBase=kbd,
                        memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout,
                        batchSize=vq.shape[0], train=True, config=cfg, params=params, seed=5, **kw)
    state = cell.run()
    ((state.memory * dmem.to(dev)).sum() + (state.control * dctl.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert cell.status() == (0, -1)
    out = {"memory": state.memory, "control": state.control}
    for i in range(p):
        out["att_kb_%d" % i] = cell.attentions["kb"][i]
        out["att_question_%d" % i] = cell.attentions["question"][i]
    out["grad_vecQuestions"], out["grad_words"], out["grad_knowledgeBase"] = vqd.grad, wd.grad, kbd.grad
    for f in params.fields:
        out["grad_" + f] = getattr(params, f).grad
    out = {k: v.detach().cpu().contiguous() for k, v in out.items()}
    return out, dict(cfg=cfg, params=params, vq=vq, words=words, lengths=lengths, kb=kb, kb_lengths=kb_lengths, dmem=dmem, dctl=dctl)


def digest(t):
    """what a fixture keeps of one fp32 tensor: SHA-256 of its bytes, shape, largest magnitude (NaN counts as such)"""
    t = t.detach().cpu().contiguous().float()
    a = t.abs()
    return {"sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest(), "shape": list(t.shape),
            "max_abs": float(a.max()) if bool(torch.isfinite(a).all()) else float("nan")}
