#!/usr/bin/env python3
"""What attention supervision costs on the replayed path, and what the fused launch returns against the route of before.

    python tools/att_loss_ab.py [--out profiles/att_loss_ab.txt] [--json FILE]

One process, the metric's shape (B = 64, S = 50, N = 196, d = 512, p = 12, train-mode dropouts), three legs on the same inputs:

    (a) captured step             macx.CapturedTrainStep.replay()                              -- the step without supervision
    (b) captured step + att_loss  the same class with att_loss=dict(on="kb", kind="ce")        -- macx_att_loss inside the graph
    (c) eager step + torch loss   MACCell.run(), cross-entropy written in torch ops over cell.attentions["kb"][i], one backward
                                  -- the only route to attention supervision before att_loss=

Untimed steps first, then 5 rounds; a round times one block of 20 steps of EACH leg, one after the other, each block between two
synchronisations, so that a drift of the machine falls on all three legs.  Reported per leg: the median block and the spread,
milliseconds per step; then (b) - (a), the price of supervision on the replayed path, and (c) / (b), what the feature returns."""
import argparse
import json
import os
import statistics
import sys
import time

BLOCKS, STEPS, WARM = 5, 20, 5


def interleaved_ms(torch, legs):
    """{name: one(i)} -> {name: figures}: WARM untimed steps of each, then BLOCKS rounds of one STEPS-step block per leg"""
    for one in legs.values():
        for i in range(WARM):
            one(i)
    times, i = {k: [] for k in legs}, WARM
    for _ in range(BLOCKS):
        for name, one in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(STEPS):
                one(i + k)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
        i += STEPS
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "blocks_ms": [round(x, 4) for x in v]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
    ap.add_argument("--out", default=None, help="the report (default: profiles/att_loss_ab.txt of this checkout)")
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    import macx
    if not torch.cuda.is_available():
        sys.exit("tools/att_loss_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    B, S, N, D, P, seed, lam, eps = 64, 50, 196, 512, 12, 1234, 0.1, 1e-8
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D)
    vq, words, lengths, kb = [t.to(dev) for t in macx.configs.synthetic_inputs(B, S, N, D, seed=seed)]
    g = torch.Generator().manual_seed(seed)
    gm = (torch.randn(B, D, generator=g) / B).to(dev)
    target = torch.softmax(torch.randn(B, N, generator=g), dim=-1).to(dev)
    row_w = (torch.rand(B, generator=g) < 0.8).float().to(dev)                  # four questions in five are supervised
    step_w = torch.ones(P, device=dev)

    def params():
        return macx.MACCellParams(cfg, P, generator=torch.Generator().manual_seed(seed)).to(dev)

    plain = macx.CapturedTrainStep(cfg, params(), B, S, N, seed=seed)
    plain.load(vq, words, lengths, kb, gm)
    fused = macx.CapturedTrainStep(cfg, params(), B, S, N, seed=seed, att_loss=dict(on="kb", kind="ce", weight=lam, eps=eps))
    fused.load(vq, words, lengths, kb, gm, att_target=target, att_row_weights=row_w, att_step_weights=step_w)

    eager_params = params()
    vq_e, words_e, kb_e = [t.clone().requires_grad_(True) for t in (vq, words, kb)]
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    scale = lam / (P * B)

    def eager_step(i):
        for t in [vq_e, words_e, kb_e] + eager_params.tensors():
            t.grad = None
        cell = macx.MACCell(vecQuestions=vq_e, questionWords=words_e, questionCntxWords=words_e, questionLengths=lengths, knowledgeBase=kb_e,
                            memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout, batchSize=B,
                            train=True, config=cfg, params=eager_params, seed=seed, mask_word=word)
        state = cell.run()
        aux = 0
        for k in range(P):
            a = cell.attentions["kb"][k]
            aux = aux - (step_w[k] * scale) * (row_w.unsqueeze(1) * target * torch.log(a + eps)).sum()
        torch.autograd.backward([state.memory, aux], [gm, None])

    res = interleaved_ms(torch, {"captured": lambda i: plain.replay(), "captured_att_loss": lambda i: fused.replay(),
                                 "eager_torch_loss": eager_step})
    plain.check()
    fused.check()
    res["graph_replay"] = {"captured": bool(plain.captured), "captured_att_loss": bool(fused.captured)}
    fused_aux = float(fused.aux_rows.sum())
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    a, b, c = res["captured"], res["captured_att_loss"], res["eager_torch_loss"]
    lines = ["attention supervision on the replayed training step (tools/att_loss_ab.py)",
             "cell only, B=%d S=%d N=%d d=%d p=%d, train-mode dropouts, CE on att_kb (weight %.2f); %s; torch %s"
             % (B, S, N, D, P, lam, torch.cuda.get_device_name(0), torch.__version__),
             "%d untimed steps per leg, then %d rounds of one %d-step block per leg, interleaved; ms per step: median block "
             "(fastest .. slowest block)" % (WARM, BLOCKS, STEPS), ""]
    for key, name in (("captured", "(a) captured step"), ("captured_att_loss", "(b) captured step + att_loss"),
                      ("eager_torch_loss", "(c) eager step + torch-op loss")):
        r = res[key]
        note = "" if res["graph_replay"].get(key, True) else "   [self-check failed in this process: EAGER launches behind the class]"
        lines.append("%-34s %8.3f  (%.3f .. %.3f)%s" % (name, r["median_ms"], r["min_ms"], r["max_ms"], note))
    lines += ["",
              "(b) - (a), the price of supervision on the replayed path: %+.3f ms per step (medians; block spread of (a): %.3f ms)"
              % (b["median_ms"] - a["median_ms"], a["max_ms"] - a["min_ms"]),
              "(c) / (b), the route of before against the fused launch:  %.2fx" % (c["median_ms"] / b["median_ms"]),
              "auxiliary loss of the last fused step: %.6f" % fused_aux]
    out = args.out or os.path.join(args.root, "profiles", "att_loss_ab.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
