#!/usr/bin/env python3
"""A/B of filing an evaluation epoch's attention maps and logits by question id inside the captured graph (macx.EvalRecords,
macx_records_scatter) against not keeping them, and against what a caller had to do before: copy them out after every replay.

    python tools/eval_records_ab.py [--out profiles/eval_records_ab.txt] [--json FILE]

The protocol of tools/question_store_ab.py: one process, B = 64, S = 50, 14 x 14 x 1024 features in an fp16 macx.FeatureStore of
1 024 images, d = 512; 8 192 questions in a macx.QuestionStore, walked by a random permutation with next_batch + replay.
CapturedTowerForward(score=True, predictions=table) at p = 12 and p = 4, built four times in the same run and timed as

    records=None        the class as it was: predictions filed, maps and logits overwritten by the next replay
    records fp16        records=rec with the kb and word maps in fp16 and the logits (fp32): one more launch in the graph
    records fp32        the same with fp32 maps
    .cpu() per batch    records=None, and after every replay a copy of fwd.attentions' kb and word maps and of the logits to the
                        host (torch.stack(...).cpu(): a synchronisation and a device-to-host copy per batch)

Before anything is timed each class runs the same batch: the logits must be equal bit for bit, and the filed rows must equal the
views' contents (fp16: after .half()).
Timing: 5 untimed calls per leg, then 5 rounds; a round times one block of 20 calls of each leg, one after the other (interleaved),
each block between two synchronisations.  Reported: the median block and the spread, milliseconds per batch."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feature_store_ab import BLOCKS, STEPS, WARM, interleaved_ms       # noqa: E402  (the same timing loop)

B, S, HW, CIN, D, VOCAB, ANSWERS, ROWS, QN, PER_IMAGE, SEED = 64, 50, 14, 1024, 512, 90, 28, 1024, 8192, 8, 1234
MAPS = ("kb", "question")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "eval_records_ab.txt"))
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("eval_records_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(SEED)
    lengths = torch.randint(1, S + 1, (QN,), generator=g, dtype=torch.int32)
    words = torch.randint(1, VOCAB + 1, (QN, S), generator=g, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    answers = torch.randint(0, ANSWERS, (QN,), generator=g, dtype=torch.int32)
    rows = (torch.arange(QN, dtype=torch.int32) // PER_IMAGE) % ROWS
    feats = macx.FeatureStore(ROWS, HW, HW, CIN, dtype=torch.float16, device=dev)
    dg = torch.Generator(device=dev).manual_seed(SEED)
    for r in range(0, ROWS, 256):
        feats.write(r, torch.relu(torch.randn(256, HW * HW, CIN, generator=dg, device=dev)))
    feats.check()
    qstore = macx.QuestionStore(words, lengths, answers, image_rows=rows, device=dev)
    perm = torch.randperm(QN, generator=g).to(torch.int32)
    order = macx.EpochOrder(qstore, B, order=perm)
    res = {"questions": {"count": QN, "nbytes": qstore.nbytes}, "features": {"rows": ROWS, "nbytes": feats.nbytes}}
    lines = ["an evaluation epoch's attention maps and logits filed by question id inside the captured graph, one process (tools/eval_records_ab.py)",
             "B=%d S=%d %dx%dx%d d=%d; %d questions about %d images (fp16 FeatureStore); %s; torch %s"
             % (B, S, HW, HW, CIN, D, QN, ROWS, torch.cuda.get_device_name(0), torch.__version__),
             "per leg: %d untimed calls, then %d interleaved blocks of %d; ms per batch (next_batch + replay): median block (fastest .. slowest block)"
             % (WARM, BLOCKS, STEPS), ""]

    def advance(c):
        if order.remaining == 0:
            order.rewind(perm)
        return c.next_batch(order)

    for p in (12, 4):
        cfg = macx.configs.flag_file_config("args", netLength=p, memDim=D, ctrlDim=D, attDim=D)
        net = macx.MACNet(cfg, vocab=VOCAB, generator=torch.Generator().manual_seed(SEED)).to(dev)
        recs = {"records fp16": macx.EvalRecords(qstore, p=p, N=HW * HW, S=S, answers=ANSWERS, maps=MAPS, dtype=torch.float16),
                "records fp32": macx.EvalRecords(qstore, p=p, N=HW * HW, S=S, answers=ANSWERS, maps=MAPS, dtype=torch.float32)}
        make = lambda rec: macx.CapturedTowerForward(net, B, S, features=feats, questions=qstore, score=True,
                                                     predictions=qstore.predictions(), records=rec)
        caps = {"records=None": make(None), "records fp16": make(recs["records fp16"]), "records fp32": make(recs["records fp32"]),
                ".cpu() per batch": make(None)}
        ids = perm[:B].to(dev)
        base, same, filed = None, True, True
        for k, c in caps.items():
            c.load_ids(ids, check_ids=False)
            logits = c.replay().clone()
            base = logits if base is None else base
            same = same and bool(torch.equal(base.view(torch.int32), logits.view(torch.int32)))
            if k in recs:
                for m in MAPS:
                    want = torch.stack(list(c.attentions[m])).transpose(0, 1).to(recs[k].dtype)
                    filed = filed and bool(torch.equal(recs[k].tables[m][ids.long()].view(torch.int16 if recs[k].dtype == torch.float16 else torch.int32),
                                                       want.contiguous().view(torch.int16 if recs[k].dtype == torch.float16 else torch.int32)))
                filed = filed and bool(torch.equal(recs[k].tables["logits"][ids.long(), 0], logits))

        def leg(c, copy_out):
            def one():
                advance(c)
                c.replay()
                if copy_out:
                    return [torch.stack(list(c.attentions[m])).cpu() for m in MAPS] + [c.logits.cpu()]
            return one
        fig = interleaved_ms(torch, {k: leg(c, k == ".cpu() per batch") for k, c in caps.items()})
        qstore.check()
        for c in caps.values():
            c.check()
        per_replay = B * p * (HW * HW + S)
        res["forward_p%d" % p] = {"legs": fig, "logits_equal": same, "filed_rows_equal": filed,
                                  "graph_replay": {k: bool(c.captured) for k, c in caps.items()},
                                  "table_nbytes": {k: r.nbytes for k, r in recs.items()}}
        lines.append("evaluation forward, p = %d   (logits of the four classes on one batch: %s; filed rows against the views: %s)"
                     % (p, "bit-identical" if same else "DIFFER", "bit-identical" if filed else "DIFFER"))
        for k, f in fig.items():
            eager = "" if caps[k].captured else "   [self-check failed in this process: EAGER launches behind the class]"
            lines.append("  %-22s %8.3f  (%.3f .. %.3f)   records=None / this = %.3f%s"
                         % (k, f["median_ms"], f["min_ms"], f["max_ms"], fig["records=None"]["median_ms"] / f["median_ms"], eager))
        lines.append("  filed per replay: %.2f MB read (fp32 maps + logits), %.2f MB written in fp16 / %.2f MB in fp32; tables of %d questions: "
                     "%.1f MB fp16, %.1f MB fp32"
                     % ((per_replay + B * ANSWERS) * 4 / 1e6, (per_replay * 2 + B * ANSWERS * 4) / 1e6, (per_replay + B * ANSWERS) * 4 / 1e6, QN,
                        recs["records fp16"].nbytes / 1e6, recs["records fp32"].nbytes / 1e6))
        lines.append("")
        del caps, recs, net
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
