#!/usr/bin/env python3
"""A/B of feeding the tower's captured graphs their questions from the host against naming rows of a macx.QuestionStore, in one process.

    python tools/question_store_ab.py [--out profiles/question_store_ab.txt] [--json FILE]

B = 64, S = 50, 14 x 14 x 1024 features in an fp16 macx.FeatureStore of 1 024 images, d = 512; 8 192 questions, 8 per image in the
store's own order.  Three workloads -- CapturedTowerForward at p = 12 and p = 4, CapturedTowerTrainStep at p = 12 -- each built twice,
with features= alone and with features= and questions=, and timed as

    load          the class without questions=: the batch sliced from the host arrays (questions, lengths, answers, image rows) and
                  load(..., check_ids=False) + replay -- the way before the QuestionStore, without its validation
    load checked  the same with load()'s default check_ids=True: the range checks of the batch on top (here on host tensors; on
                  device tensors they are two synchronisations per step)
    load_ids      the class with questions=: load_ids(a [64] host id vector) + replay
    next_batch    the same class: next_batch(order) + replay -- a device-to-device slice of a macx.EpochOrder

Every leg walks the same 128 batches of a random permutation.  Before anything is timed the two classes run one batch each: the logits
(forward) / the first step's loss (training) must be equal bit for bit.  The evaluation forward is also timed with images=8 on the
store's own order, where the 64 questions of a batch ask about 8 images (grouped on the device by the gather), against the
questions= class without images= on the same order (the stem on 64 images).
Timing: 5 untimed calls per leg, then 5 rounds; a round times one block of 20 calls of each leg, one after the other (interleaved),
each block between two synchronisations.  Reported: the median block and the spread, milliseconds per batch."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feature_store_ab import BLOCKS, STEPS, WARM, interleaved_ms       # noqa: E402  (the same timing loop)

B, S, HW, CIN, D, VOCAB, ANSWERS, ROWS, QN, PER_IMAGE, SEED = 64, 50, 14, 1024, 512, 90, 28, 1024, 8192, 8, 1234


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "question_store_ab.txt"))
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("question_store_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(SEED)
    lengths = torch.randint(1, S + 1, (QN,), generator=g, dtype=torch.int32)
    words = torch.randint(1, VOCAB + 1, (QN, S), generator=g, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    answers = torch.randint(0, ANSWERS, (QN,), generator=g, dtype=torch.int32)
    rows = (torch.arange(QN, dtype=torch.int32) // PER_IMAGE) % ROWS              # 8 consecutive questions per image
    feats = macx.FeatureStore(ROWS, HW, HW, CIN, dtype=torch.float16, device=dev)
    dg = torch.Generator(device=dev).manual_seed(SEED)
    for r in range(0, ROWS, 256):
        feats.write(r, torch.relu(torch.randn(256, HW * HW, CIN, generator=dg, device=dev)))
    feats.check()
    qstore = macx.QuestionStore(words, lengths, answers, image_rows=rows, device=dev)
    perm = torch.randperm(QN, generator=g).to(torch.int32)
    vectors = [perm[i:i + B].clone() for i in range(0, QN, B)]                 # the permutation's batches, as host id vectors
    turn = {"i": -1}

    def next_ids():
        turn["i"] = (turn["i"] + 1) % len(vectors)
        return vectors[turn["i"]]

    def sliced(ids):
        ids = ids.long()
        return words[ids], lengths[ids], answers[ids], rows[ids]

    def advance(c, order):
        if order.remaining == 0:
            order.rewind(perm if order is shuffled else None)
        return c.next_batch(order)

    shuffled, in_order = macx.EpochOrder(qstore, B, order=perm), macx.EpochOrder(qstore, B)
    res = {"questions": {"count": QN, "nbytes": qstore.nbytes}, "features": {"rows": ROWS, "nbytes": feats.nbytes}}
    lines = ["questions sliced on the host per step against rows of a device-resident QuestionStore named by id, one process (tools/question_store_ab.py)",
             "B=%d S=%d %dx%dx%d d=%d; %d questions (%.1f MB) about %d images (fp16 FeatureStore, %.1f MB); %s; torch %s"
             % (B, S, HW, HW, CIN, D, QN, qstore.nbytes / 1e6, ROWS, feats.nbytes / 1e6, torch.cuda.get_device_name(0), torch.__version__),
             "per leg: %d untimed calls, then %d interleaved blocks of %d; ms per batch: median block (fastest .. slowest block)"
             % (WARM, BLOCKS, STEPS), ""]

    def make_net(p):
        cfg = macx.configs.flag_file_config("args", netLength=p, memDim=D, ctrlDim=D, attDim=D)
        return macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(SEED)).to(dev)

    def report(title, caps, fig, note, base="load"):
        lines.append("%s   (%s)" % (title, note))
        for k, f in fig.items():
            eager = "" if caps[k].captured else "   [self-check failed in this process: EAGER launches behind the class]"
            lines.append("  %-22s %8.3f  (%.3f .. %.3f)   %s / this = %.3f%s"
                         % (k, f["median_ms"], f["min_ms"], f["max_ms"], base, fig[base]["median_ms"] / f["median_ms"], eager))
        lines.append("")

    for p in (12, 4):                                                       # ---- evaluation forward
        net = make_net(p)
        old = macx.CapturedTowerForward(net, B, S, features=feats)
        new = macx.CapturedTowerForward(net, B, S, features=feats, questions=qstore)
        ids = vectors[0]
        q, ln, _, r = sliced(ids)
        a = old(None, q, ln, check_ids=False, image_ids=r).clone()
        new.load_ids(ids)
        same = bool(torch.equal(a.view(torch.int32), new.replay().view(torch.int32)))

        def load_leg(check):
            def one():
                q, ln, _, r = sliced(next_ids())
                old(None, q, ln, check_ids=check, image_ids=r)
            return one

        def ids_leg():
            new.load_ids(next_ids())
            new.replay()

        def order_leg():
            advance(new, shuffled)
            new.replay()
        fig = interleaved_ms(torch, {"load": load_leg(False), "load checked": load_leg(True), "load_ids": ids_leg, "next_batch": order_leg})
        caps = {"load": old, "load checked": old, "load_ids": new, "next_batch": new}
        res["forward_p%d" % p] = {"legs": fig, "logits_equal": same, "graph_replay": {k: bool(c.captured) for k, c in caps.items()}}
        report("evaluation forward, p = %d" % p, caps, fig, "load_ids against load on the same batch: logits %s" % ("bit-identical" if same else "DIFFER"))
        # shared images: the store's own order asks 8 questions per image
        grouped = macx.CapturedTowerForward(net, B, S, features=feats, questions=qstore, images=B // PER_IMAGE)
        in_order.rewind()
        new.next_batch(in_order)
        a = new.replay().clone()
        in_order.rewind()
        grouped.next_batch(in_order)
        same = bool(torch.equal(a.view(torch.int32), grouped.replay().view(torch.int32)))

        def shared_leg(c):
            def one():
                advance(c, in_order)
                c.replay()
            return one
        fig = interleaved_ms(torch, {"one image per question": shared_leg(new), "images=8": shared_leg(grouped)})
        caps = {"one image per question": new, "images=8": grouped}
        res["forward_p%d_shared" % p] = {"legs": fig, "logits_equal": same, "graph_replay": {k: bool(c.captured) for k, c in caps.items()}}
        report("evaluation forward, p = %d, next_batch on the store's own order (8 questions per image)" % p, caps, fig,
               "logits of the two on the same batch: %s" % ("bit-identical" if same else "differ (the stem's batch differs)"),
               base="one image per question")
        qstore.check()
        for c in (old, new, grouped):
            c.check()
        del old, new, grouped, net

    steps = {}                                                              # ---- training step, p = 12: a net per class
    for k in ("old", "new"):
        net = make_net(12)
        bucket = macx.dp.TowerBuckets(net, fused_gather=True)
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4, clip_norm=8.0, ema_decay=0.999)
        steps[k] = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, seed=SEED, features=feats, **({} if k == "old" else {"questions": qstore}))
    old, new = steps["old"], steps["new"]
    q, ln, an, r = sliced(vectors[0])
    old.load(None, q, ln, an, check_ids=False, image_ids=r)
    new.load_ids(vectors[0])
    losses = {"load": float(old.replay(iteration=0)), "load_ids": float(new.replay(iteration=0))}
    same = losses["load"] == losses["load_ids"]

    def train_load(check):
        def one():
            q, ln, an, r = sliced(next_ids())
            old.load(None, q, ln, an, check_ids=check, image_ids=r)
            old.replay()
        return one

    def train_ids():
        new.load_ids(next_ids())
        new.replay()

    def train_order():
        advance(new, shuffled)
        new.replay()
    fig = interleaved_ms(torch, {"load": train_load(False), "load checked": train_load(True), "load_ids": train_ids, "next_batch": train_order})
    caps = {"load": old, "load checked": old, "load_ids": new, "next_batch": new}
    qstore.check()
    for c in (old, new):
        c.check()
    res["train_p12"] = {"legs": fig, "first_step_loss": losses, "loss_equal": same, "graph_replay": {k: bool(c.captured) for k, c in caps.items()}}
    report("training step, p = 12", caps, fig, "first step's loss: load %.6f, load_ids %.6f (%s)"
           % (losses["load"], losses["load_ids"], "equal" if same else "DIFFERENT"))
    lines.append("host-to-device bytes per batch: load %d (question ids + lengths + answers + image rows), load_ids %d, next_batch 0"
                 % (B * S * 4 + 3 * B * 4, B * 4))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
