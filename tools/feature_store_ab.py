#!/usr/bin/env python3
"""A/B of feeding the tower's captured graphs image features from the host against naming rows of a macx.FeatureStore, in one process.

    python tools/feature_store_ab.py [--out profiles/feature_store_ab.txt] [--json FILE]

bench.py:model_level's inputs (B = 64, S = 50, 14 x 14 x 1024 features, d = 512).  Three classes -- CapturedTowerForward at p = 12 and
p = 4, CapturedTowerTrainStep at p = 12 -- and three legs per class:

    upload   the class as it was: load() of the [64, 196, 1024] fp32 batch from pinned host memory + replay (51.4 MB per batch)
    fp16     the class built with features= on an fp16 store: load(image_ids=) + replay; the gather runs inside the graph
    fp32     the same on an fp32 store (the gather is macx_kb_gather's copy kernel)

The stores hold 2 048 images (0.8 GB in fp16, 1.6 GB in fp32: beyond the 256 MiB cache); rows 0 .. 63 are the upload leg's batch,
and every timed call names the next of 16 id vectors that together cover 1 024 distinct rows, so a gather reads from HBM.  Before
anything is timed the three legs run on the same images once: fp32 logits must equal the upload leg's bit for bit, the largest
fp16 - fp32 difference is recorded for information.  Timing: 5 untimed calls per leg, then 5 rounds; a round times one block of 20
calls of each leg, one after the other (interleaved), each block between two synchronisations.  Reported: the median block and the
spread, milliseconds per batch.  The gather alone is timed the same way (200 calls per block) against macx_kb_gather on the same
output bytes."""
import argparse
import json
import os
import statistics
import sys
import time

BLOCKS, STEPS, WARM = 5, 20, 5
B, S, HW, CIN, D, VOCAB, ROWS, VECTORS, SEED = 64, 50, 14, 1024, 512, 90, 2048, 16, 1234


def interleaved_ms(torch, legs, steps=STEPS):
    """legs: {name: callable}; returns {name: figures}"""
    for one in legs.values():
        for _ in range(WARM):
            one()
    out = {k: [] for k in legs}
    for _ in range(BLOCKS):
        for k, one in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "blocks_ms": [round(x, 4) for x in v]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "feature_store_ab.txt"))
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("feature_store_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    N = HW * HW
    g = torch.Generator().manual_seed(SEED)                                   # bench.py:model_level's draws, in its order
    _, _, lengths, _ = macx.configs.synthetic_inputs(B, S, 1, 8, seed=SEED)
    img = torch.relu(torch.randn(B, N, CIN, generator=g)).pin_memory()
    qs = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32)
    qs = (qs * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)).pin_memory()
    lengths = lengths.to(torch.int32).pin_memory()
    ans = torch.randint(0, 28, (B,), generator=g).to(torch.int32).pin_memory()

    stores = {}
    dg = torch.Generator(device=dev).manual_seed(SEED)
    rest = [torch.relu(torch.randn(256, N, CIN, generator=dg, device=dev)) for _ in range(ROWS // 256)]
    rest[0][:B] = img.to(dev)
    for name, dt in (("fp16", torch.float16), ("fp32", torch.float32)):
        st = macx.FeatureStore(ROWS, HW, HW, CIN, dtype=dt, device=dev)
        for i, chunk in enumerate(rest):
            st.write(256 * i, chunk)
        stores[name] = st.check()
    del rest
    first = torch.arange(B, dtype=torch.int32).pin_memory()                   # the upload leg's images
    perm = torch.randperm(ROWS, generator=g)[:VECTORS * B].to(torch.int32).reshape(VECTORS, B)
    vectors = [perm[i].clone().pin_memory() for i in range(VECTORS)]
    turn = {"i": 0}

    def next_ids():
        turn["i"] = (turn["i"] + 1) % VECTORS
        return vectors[turn["i"]]

    res = {"stores": {k: {"rows": ROWS, "nbytes": s.nbytes} for k, s in stores.items()},
           "h2d_bytes": {"upload": B * N * CIN * 4 + B * S * 4 + B * 4, "ids": B * 4 + B * S * 4 + B * 4}}
    lines = ["image batch uploaded per step against rows of a device-resident FeatureStore named by id, one process (tools/feature_store_ab.py)",
             "B=%d S=%d %dx%dx%d d=%d; stores of %d images: fp16 %.1f MB, fp32 %.1f MB; %s; torch %s"
             % (B, S, HW, HW, CIN, D, ROWS, stores["fp16"].nbytes / 1e6, stores["fp32"].nbytes / 1e6, torch.cuda.get_device_name(0),
                torch.__version__),
             "per leg: %d untimed calls, then %d interleaved blocks of %d; ms per batch: median block (fastest .. slowest block)"
             % (WARM, BLOCKS, STEPS),
             "every leg is load() + replay(): upload = the fp32 batch from pinned host memory, fp16 / fp32 = 64 row ids", ""]

    def make_net(p):
        cfg = macx.configs.flag_file_config("args", netLength=p, memDim=D, ctrlDim=D, attDim=D)
        return macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(SEED)).to(dev)

    def report(title, caps, fig, note):
        lines.append("%s   (%s)" % (title, note))
        for k in ("upload", "fp16", "fp32"):
            f = fig[k]
            eager = "" if caps[k].captured else "   [self-check failed in this process: EAGER launches behind the class]"
            lines.append("  %-8s %8.3f  (%.3f .. %.3f)   upload / this = %.3f%s"
                         % (k, f["median_ms"], f["min_ms"], f["max_ms"], fig["upload"]["median_ms"] / f["median_ms"], eager))
        lines.append("")

    for p in (12, 4):                                                       # ---- evaluation forward
        net = make_net(p)
        caps = {"upload": macx.CapturedTowerForward(net, B, S)}
        for k, st in stores.items():
            caps[k] = macx.CapturedTowerForward(net, B, S, features=st)
        logits = {"upload": caps["upload"](img, qs, lengths, check_ids=False).clone()}
        for k in stores:
            logits[k] = caps[k](None, qs, lengths, check_ids=False, image_ids=first).clone()
        torch.cuda.synchronize()
        same32 = bool(torch.equal(logits["upload"].view(torch.int32), logits["fp32"].view(torch.int32)))
        diff16 = float((logits["fp16"] - logits["fp32"]).abs().max())
        legs = {"upload": lambda: caps["upload"](img, qs, lengths, check_ids=False)}
        for k in stores:
            legs[k] = (lambda c: lambda: c(None, qs, lengths, check_ids=False, image_ids=next_ids()))(caps[k])
        fig = interleaved_ms(torch, legs)
        for c in caps.values():
            c.check()
        res["forward_p%d" % p] = {"load_and_replay": fig, "fp32_logits_equal_upload": same32, "max_abs_logits_difference_fp16_fp32": diff16,
                                  "graph_replay": {k: bool(c.captured) for k, c in caps.items()}}
        report("evaluation forward, p = %d" % p, caps, fig,
               "fp32 store against upload: logits %s; fp16 against fp32 store: largest logit difference %.3e"
               % ("bit-identical" if same32 else "DIFFER", diff16))
        del caps, legs, net

    caps, nets = {}, {}                                                       # ---- training step, p = 12: a net per leg
    for k in ("upload", "fp16", "fp32"):
        nets[k] = make_net(12)
        bucket = macx.dp.TowerBuckets(nets[k], fused_gather=True)
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4, clip_norm=8.0, ema_decay=0.999)
        caps[k] = macx.CapturedTowerTrainStep(nets[k], opt, bucket, B, S, seed=SEED, **({} if k == "upload" else {"features": stores[k]}))
    caps["upload"].load(img, qs, lengths, ans, check_ids=False)
    for k in stores:
        caps[k].load(None, qs, lengths, ans, check_ids=False, image_ids=first)
    losses = {k: float(c.replay(iteration=0)) for k, c in caps.items()}
    same32 = losses["upload"] == losses["fp32"]

    def train_leg(c, upload):
        def one():
            if upload:
                c.load(img, qs, lengths, ans, check_ids=False)
            else:
                c.load(None, qs, lengths, ans, check_ids=False, image_ids=next_ids())
            c.replay()
        return one
    fig = interleaved_ms(torch, {k: train_leg(c, k == "upload") for k, c in caps.items()})
    for c in caps.values():
        c.check()
    res["train_p12"] = {"load_and_replay": fig, "first_step_loss": losses, "fp32_loss_equals_upload": same32,
                        "graph_replay": {k: bool(c.captured) for k, c in caps.items()}}
    report("training step, p = 12", caps, fig, "first step's loss: upload %.6f, fp32 store %.6f (%s), fp16 store %.6f"
           % (losses["upload"], losses["fp32"], "equal" if same32 else "DIFFERENT", losses["fp16"]))
    del caps, nets

    # ---- the gather alone: 64 rows into a [64, 196, 1024] fp32 batch
    out = torch.empty(B, N, CIN, device=dev)
    dvec = [v.to(dev) for v in vectors]
    L, p_ = macx._lib.lib(), macx._lib.ptr
    f32 = stores["fp32"]

    def kb_gather():
        macx._lib.check(L.macx_kb_gather(p_(f32.table), p_(dvec[turn["i"]]), ROWS, B, N, CIN, p_(out), macx._lib.stream_of(out)), "macx_kb_gather")
        next_ids()

    def store_gather(st):
        def one():
            st.gather_into(dvec[turn["i"]], out)
            next_ids()
        return one
    fig = interleaved_ms(torch, {"fp16": store_gather(stores["fp16"]), "fp32": store_gather(f32), "macx_kb_gather": kb_gather}, steps=200)
    res["gather_alone"] = fig
    wrote = B * N * CIN * 4
    lines.append("the gather alone, %d rows -> %.1f MB of fp32 output, blocks of 200 calls: microseconds per call, bytes moved (read + written) per second"
                 % (B, wrote / 1e6))
    for k, read in (("fp16", wrote // 2), ("fp32", wrote), ("macx_kb_gather", wrote)):
        f = fig[k]
        lines.append("  %-15s %8.1f us  (%.1f .. %.1f)   %.2f TB/s" % (k, f["median_ms"] * 1e3, f["min_ms"] * 1e3, f["max_ms"] * 1e3,
                                                                       (read + wrote) / (f["median_ms"] * 1e-3) / 1e12))
    lines += ["", "host-to-device bytes per batch: upload %d (images + question ids + lengths), ids %d (row ids + question ids + lengths)"
              % (res["h2d_bytes"]["upload"], res["h2d_bytes"]["ids"])]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
