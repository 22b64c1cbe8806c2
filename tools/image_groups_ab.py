#!/usr/bin/env python3
"""A/B of the evaluation forward for a batch whose questions share images: 64 duplicated images against 7 images + an index, both
replayed from a captured HIP graph (macx.CapturedTowerForward), in one process.

    python tools/image_groups_ab.py [--out profiles/image_groups_ab.txt] [--json FILE]

The workload's shape: B = 64 questions, S = 50, 14 x 14 x 1024 features, d = 512, at p = 12 and p = 4.  Two legs per net length:

    duplicated   CapturedTowerForward(net, 64, 50): every question brings its own copy of its image (the only route before
                 `images=` existed, hence the baseline); the stem runs on 64 images
    grouped      CapturedTowerForward(net, 64, 50, images=7) with image_index = b // 10 (CLEVR's 10 questions per image): the stem
                 runs on 7 images, macx_kb_gather copies each question's block

Both legs see the same questions and, through the index, the same images; their logits are compared once (largest difference,
argmax agreement) before anything is timed.  Timing: 5 untimed replays per leg, then 5 rounds; a round times one block of 20
replays of each leg, one after the other (interleaved), each block between two synchronisations.  Reported: the median block and
the spread, milliseconds per batch, and questions per second from the median.  Inputs stay loaded while a leg is timed; what a
caller uploads per batch is reported as bytes, computed from the shapes.  A second pair of figures times load() from pinned host
memory + replay(), the same way."""
import argparse
import json
import os
import statistics
import sys
import time

BLOCKS, STEPS, WARM = 5, 20, 5
B, S, HW, CIN, D, VOCAB, G, PER_IMAGE = 64, 50, 14, 1024, 512, 90, 7, 10


def interleaved_ms(torch, legs):
    """legs: {name: callable}; returns {name: figures}"""
    for one in legs.values():
        for _ in range(WARM):
            one()
    out = {k: [] for k in legs}
    for _ in range(BLOCKS):
        for k, one in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                one()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / STEPS * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "questions_per_s": round(B / statistics.median(v) * 1e3, 1), "blocks_ms": [round(x, 4) for x in v]}
            for k, v in out.items()}


def h2d_bytes(images):
    """what load() copies to the device per batch: image features, question ids, lengths (+ the index)"""
    n = images * HW * HW * CIN * 4 + B * S * 4 + B * 4
    return n + (B * 4 if images != B else 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "image_groups_ab.txt"))
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("image_groups_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    images7 = torch.relu(torch.randn(G, HW * HW, CIN, generator=g)).pin_memory()
    index = (torch.arange(B, dtype=torch.int32) // PER_IMAGE).pin_memory()
    assert int(index.max()) == G - 1
    images64 = images7[index.long()].contiguous().pin_memory()
    _, _, lengths, _ = macx.configs.synthetic_inputs(B, S, 1, 8, seed=1234)
    qs = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32)
    qs = (qs * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)).pin_memory()
    lengths = lengths.to(torch.int32).pin_memory()

    res = {"h2d_bytes": {"duplicated": h2d_bytes(B), "grouped": h2d_bytes(G)}}
    lines = ["evaluation forward, 64 duplicated images against 7 images + index, both from one replayed HIP graph (tools/image_groups_ab.py)",
             "B=%d S=%d %dx%dx%d d=%d, %d images, image_index = b // %d; %s; torch %s"
             % (B, S, HW, HW, CIN, D, G, PER_IMAGE, torch.cuda.get_device_name(0), torch.__version__),
             "per leg: %d untimed replays, then %d interleaved blocks of %d; ms per batch: median block (fastest .. slowest block)"
             % (WARM, BLOCKS, STEPS), ""]
    for p in (12, 4):
        cfg = macx.configs.flag_file_config("args", netLength=p, memDim=D, ctrlDim=D, attDim=D)
        net = macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(1234)).to(dev)
        dup = macx.CapturedTowerForward(net, B, S)
        grp = macx.CapturedTowerForward(net, B, S, images=G)
        dup.load(images64, qs, lengths)
        grp.load(images7, qs, lengths, image_index=index)
        a, b = dup.replay().clone(), grp.replay().clone()
        torch.cuda.synchronize()
        diff = float((a - b).abs().max())
        same_pred = bool(torch.equal(a.argmax(1), b.argmax(1)))
        r = interleaved_ms(torch, {"duplicated": dup.replay, "grouped": grp.replay})
        rl = interleaved_ms(torch, {"duplicated": lambda: dup(images64, qs, lengths, check_ids=False),
                                    "grouped": lambda: grp(images7, qs, lengths, check_ids=False, image_index=index)})
        dup.check()
        grp.check()
        res["p%d" % p] = {"replay": r, "load_and_replay": rl, "max_abs_logits_difference": diff, "same_argmax": same_pred,
                          "graph_replay": {"duplicated": bool(dup.captured), "grouped": bool(grp.captured)}}
        lines.append("p = %d   (logits of the two legs: largest difference %.3e, argmax %s)" % (p, diff, "identical" if same_pred else "DIFFERS"))
        for what, fig in (("replay", r), ("load (pinned host) + replay", rl)):
            for k, cap in (("duplicated", dup), ("grouped", grp)):
                f = fig[k]
                note = "" if cap.captured else "   [self-check failed in this process: EAGER launches behind the class]"
                lines.append("  %-28s %-11s %8.3f  (%.3f .. %.3f)  %9.1f questions/s%s"
                             % (what, k, f["median_ms"], f["min_ms"], f["max_ms"], f["questions_per_s"], note))
            lines.append("  %-28s duplicated / grouped = %.3f" % (what, fig["duplicated"]["median_ms"] / fig["grouped"]["median_ms"]))
        lines.append("")
        del dup, grp, net
    lines.append("host-to-device bytes per batch (image features + question ids + lengths [+ index]): duplicated %d, grouped %d"
                 % (res["h2d_bytes"]["duplicated"], res["h2d_bytes"]["grouped"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
