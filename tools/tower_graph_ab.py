#!/usr/bin/env python3
"""A/B of the whole tower's step and evaluation forward: eager ctypes launches against ONE replayed HIP graph, in one process.

    python tools/tower_graph_ab.py [--out profiles/tower_graph_ab.txt] [--parent-bench-json FILE] [--parent-eager-json FILE]

The workload and the inputs are bench.py:model_level's (question ids + lengths, 14 x 14 x 1024 features, answers; B = 64, S = 50,
d = 512, p = 12, train-mode dropouts; clip + Adam + EMA).  Four legs:

    eager train step      net(...) -> loss -> backward -> TowerBuckets gather (copy_) -> FlatAdamEMA.step       (model_level's `one`)
    captured train step   macx.CapturedTowerTrainStep.replay(iteration=i)   (inputs stay loaded, as in the eager leg)
    eager eval forward    net(..., train=False) under no_grad
    captured eval forward macx.CapturedTowerForward.replay()

Each leg: 5 untimed steps, then 5 blocks of 20 steps, each block between two synchronisations; reported: the median block and
the spread (fastest .. slowest block), milliseconds per step.  `--eager-only --json FILE` runs the two eager legs alone and needs
nothing this commit added, so the same file measures a checkout of the parent commit (`--root DIR`) in the same GPU visit; that
figure and the parent's own `bench.py` model_level.ms_per_step are recorded in the output as the baseline."""
import argparse
import json
import os
import statistics
import sys
import time

BLOCKS, STEPS, WARM = 5, 20, 5


def blocks_ms(torch, one):
    for i in range(WARM):
        one(i)
    out, i = [], WARM
    for _ in range(BLOCKS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            one(i)
            i += 1
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / STEPS * 1e3)
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4),
            "blocks_ms": [round(x, 4) for x in out]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
    ap.add_argument("--out", default=None, help="the report (default: profiles/tower_graph_ab.txt of this checkout)")
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    ap.add_argument("--eager-only", action="store_true")
    ap.add_argument("--parent-bench-json", default=None, help="the parent commit's bench.py output (its JSON result line)")
    ap.add_argument("--parent-eager-json", default=None, help="--eager-only --json output measured on the parent commit's checkout")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    import macx
    dev = torch.device("cuda:0")
    B, S, N, D, P, VOCAB, seed = 64, 50, 196, 512, 12, 90, 1234
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D)

    def tower(**bucket_kw):
        net = macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(seed)).to(dev)
        bucket = macx.dp.TowerBuckets(net, **bucket_kw)
        return net, bucket, macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4, clip_norm=8.0, ema_decay=0.999)

    g = torch.Generator().manual_seed(seed)                            # bench.py:model_level's inputs
    _, _, lengths, _ = macx.configs.synthetic_inputs(B, S, 1, 8, seed=seed)
    img = torch.relu(torch.randn(B, N, 1024, generator=g)).to(dev)
    qs = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32)
    qs = (qs * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)).to(dev)
    lengths = lengths.to(dev)
    ans = torch.randint(0, 28, (B,), generator=g).to(dev)

    net, bucket, opt = tower()

    def eager_step(i):
        for t in net.tensors():
            t.grad = None
        logits = net(img, qs, lengths, train=True, seed=seed + i, check_ids=False)
        loss, _ = net.loss_and_pred(logits, ans)
        bucket.begin_step(B, B)
        loss.backward()
        bucket.allreduce_(B, B)
        opt.step(flat_grad=bucket.flat)

    def eager_fwd(i):
        with torch.no_grad():
            net(img, qs, lengths, train=False, check_ids=False)

    res = {"eager_train_step": blocks_ms(torch, eager_step), "eager_eval_forward": blocks_ms(torch, eager_fwd)}
    if not args.eager_only:
        cnet, cbucket, copt = tower(fused_gather=True)
        step = macx.CapturedTowerTrainStep(cnet, copt, cbucket, B, S, H=14, W=14, imageInDim=1024, seed=seed)
        step.load(img, qs, lengths, ans.to(torch.int32))
        res["captured_train_step"] = dict(blocks_ms(torch, lambda i: step.replay(iteration=i)), graph_replay=bool(step.captured))
        step.check()
        fwd = macx.CapturedTowerForward(cnet, B, S)
        fwd.load(img, qs, lengths)
        res["captured_eval_forward"] = dict(blocks_ms(torch, lambda i: fwd.replay()), graph_replay=bool(fwd.captured))
        fwd.check()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    if args.eager_only:
        print(json.dumps(res))
        return
    lines = ["whole tower, eager launches against one replayed HIP graph (tools/tower_graph_ab.py)",
             "B=%d S=%d 14x14x1024 d=%d p=%d, train-mode dropouts, clip + Adam + EMA; %s; torch %s" %
             (B, S, D, P, torch.cuda.get_device_name(0), torch.__version__),
             "per leg: %d untimed steps, then %d blocks of %d steps; ms per step: median block (fastest .. slowest block)" % (WARM, BLOCKS, STEPS), ""]
    for k in ("eager_train_step", "captured_train_step", "eager_eval_forward", "captured_eval_forward"):
        r = res[k]
        note = "" if r.get("graph_replay", True) else "   [self-check failed in this process: EAGER launches behind the class]"
        lines.append("%-24s %8.3f  (%.3f .. %.3f)%s" % (k, r["median_ms"], r["min_ms"], r["max_ms"], note))
    lines.append("")
    if args.parent_eager_json and os.path.exists(args.parent_eager_json):
        pe = json.load(open(args.parent_eager_json))
        for k in ("eager_train_step", "eager_eval_forward"):
            r = pe[k]
            lines.append("parent commit, %-18s %8.3f  (%.3f .. %.3f)   same tool, same GPU visit" % (k, r["median_ms"], r["min_ms"], r["max_ms"]))
        a, b = res["eager_train_step"], pe["eager_train_step"]
        inside = b["min_ms"] <= a["median_ms"] <= b["max_ms"] or a["median_ms"] <= b["median_ms"]
        lines.append("this commit's eager train step (median %.3f) %s the parent's block spread (%.3f .. %.3f)"
                     % (a["median_ms"], "lies within or below" if inside else "lies ABOVE", b["min_ms"], b["max_ms"]))
    if args.parent_bench_json and os.path.exists(args.parent_bench_json):
        ml = None
        for ln in open(args.parent_bench_json):
            ln = ln.strip()
            if ln.startswith("{"):
                try:
                    ml = json.loads(ln).get("model_level", ml)
                except ValueError:
                    pass
        if ml:
            lines.append("parent commit, bench.py model_level.ms_per_step: %s  (%s questions/s; fastest of its 3 blocks of 6 steps) -- the "
                         "baseline the README quotes against" % (ml["ms_per_step"], ml["value"]))
    out = args.out or os.path.join(args.root, "profiles", "tower_graph_ab.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
