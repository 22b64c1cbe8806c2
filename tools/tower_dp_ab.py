#!/usr/bin/env python3
"""What cutting the whole tower's training step at its collectives costs and buys, in ONE process (no collective is issued):

    python tools/tower_dp_ab.py [--out profiles/tower_dp_ab.txt]

The tower is the metric's (14 x 14 x 1024 features, S = 50, d = 512, p = 12, train-mode dropouts, clip + Adam + EMA), the inputs random.

    (a) B = 64 of a global 64: macx.CapturedDPTowerTrainStep -- two graphs, and three with weights=True -- against
        macx.CapturedTowerTrainStep's one graph: the price of cutting the graph.
    (b) a shard of 8 of a global 64: the replayed parts against the eager data-parallel step (net, loss_and_pred, TowerBuckets
        begin_step / allreduce_, FlatAdamEMA.step): the launch-bound case the class exists for.

Per comparison: 5 untimed steps of every leg, then 5 rounds in which the legs take turns at a block of 20 steps between two
synchronisations (interleaved, so drift hits every leg alike); reported: the median block and the spread, milliseconds per step.
Nothing here says anything about more than one GPU: an all-reduce is not part of any leg."""
import argparse
import os
import statistics
import sys
import time

BLOCKS, STEPS, WARM = 5, 20, 5


def interleaved_ms(torch, legs):
    """legs: {name: one(i)} -> {name: (median, fastest, slowest) ms per step}"""
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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "tower_dp_ab.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    dev = torch.device("cuda:0")
    GLOBAL, S, N, D, P, VOCAB, seed = 64, 50, 196, 512, 12, 90, 1234
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D)
    g = torch.Generator().manual_seed(seed)

    def tower(**bucket_kw):
        net = macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(seed)).to(dev)
        bucket = macx.dp.TowerBuckets(net, **bucket_kw)
        return net, bucket, macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4, clip_norm=8.0, ema_decay=0.999)

    def batch(B):
        lengths = torch.randint(3, S + 1, (B,), generator=g, dtype=torch.int32)
        qs = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32)
        qs = qs * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)
        img = torch.relu(torch.randn(B, N, 1024, generator=g))
        return img.to(dev), qs.to(dev), lengths.to(dev), torch.randint(0, 28, (B,), generator=g, dtype=torch.int32).to(dev)

    def dp_step(B, x, **kw):
        net, bucket, opt = tower(fused_gather=True, exchange=False)
        step = macx.CapturedDPTowerTrainStep(net, opt, bucket, B=B, S=S, global_batch=GLOBAL, b0=0, seed=seed, **kw)
        step.load(*x)
        return step

    notes = []

    def leg(step, run):
        if not step.captured:
            notes.append("%s: the self-check failed in this process, EAGER launches behind the class" % type(step).__name__)
        return run

    # (a) the price of the cut, B = 64
    x = batch(GLOBAL)
    net, bucket, opt = tower(fused_gather=True)
    one = macx.CapturedTowerTrainStep(net, opt, bucket, GLOBAL, S, seed=seed)
    one.load(*x)
    two, three = dp_step(GLOBAL, x), dp_step(GLOBAL, x, weights=True)
    a = interleaved_ms(torch, {"CapturedTowerTrainStep, one graph": leg(one, lambda i: one.replay(iteration=i)),
                               "CapturedDPTowerTrainStep, graphs A + B": leg(two, lambda i: two.step(iteration=i)),
                               "... weights=True, graphs Q + A + B": leg(three, lambda i: three.step(iteration=i))})
    for s in (one, two, three):
        s.check()
    del one, two, three, net, bucket, opt
    # (b) the launch-bound shard: 8 of 64
    B = 8
    x = batch(B)
    parts = dp_step(B, x)
    enet, ebucket, eopt = tower()
    img, qs, lengths, ans = x

    def eager(i):
        for t in enet.tensors():
            t.grad = None
        logits = enet(img, qs, lengths, train=True, seed=seed + i, b0=0, check_ids=False)
        loss, _ = enet.loss_and_pred(logits, ans)
        ebucket.begin_step(B, GLOBAL)
        loss.backward()
        ebucket.allreduce_(B, GLOBAL)
        eopt.step(flat_grad=ebucket.flat)

    b = interleaved_ms(torch, {"eager TowerBuckets step": eager,
                               "CapturedDPTowerTrainStep, graphs A + B": leg(parts, lambda i: parts.step(iteration=i))})
    parts.check()
    lines = ["whole tower, the training step cut at its collectives (tools/tower_dp_ab.py); ONE process, no collective in any leg",
             "14x14x1024 S=%d d=%d p=%d, train-mode dropouts, clip + Adam + EMA, random inputs; %s; torch %s"
             % (S, D, P, torch.cuda.get_device_name(0), torch.__version__),
             "%d untimed steps per leg, then %d rounds of interleaved blocks of %d steps; ms per step: median block (fastest .. slowest)"
             % (WARM, BLOCKS, STEPS), "", "(a) B = 64 of a global 64: the price of cutting the graph"]
    lines += ["    %-44s %8.3f  (%.3f .. %.3f)" % ((k,) + v) for k, v in a.items()]
    lines += ["", "(b) a shard of 8 of a global 64: replayed parts against eager launches"]
    lines += ["    %-44s %8.3f  (%.3f .. %.3f)" % ((k,) + v) for k, v in b.items()]
    lines += [""] + notes + ["no kernel was added for this class, and nothing was measured on more than one GPU"]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
