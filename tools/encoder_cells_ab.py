#!/usr/bin/env python3
"""A/B of the question encoder's fused recurrent path (macx.RecurrentQuestionEncoder: encType RNN | GRU | LSTM, one direction or
two, macx_rnn_encoder_forward_w / _backward_w) against the two classes that ran an encoder before it.

    python tools/encoder_cells_ab.py [--out profiles/encoder_cells_ab.txt] [--json FILE]

One process, B = 64, S = 50 (lengths 1 .. 50, question 0 full), wrdEmbDim 300, encDim 512, vocabulary 90; train mode, one call =
forward + backward of the encoder alone (random gradients for both outputs), eager launches from Python as a training step
outside a captured graph makes them.  Legs:

    LSTM 1 dir, generic       macx.GenericQuestionEncoder: one HIP kernel per reference op, about 14 launches per word from Python
    LSTM 1 dir, recurrent     the new class on the same option set (the parser's default: no --encBi, h = 512)
    LSTM 2 dir, fused         macx.QuestionEncoder (h = 256 per direction): what every flag file runs
    LSTM 2 dir, recurrent     the new class on it: the same launches, so the same time within the noise
    GRU / RNN, 1 and 2 dir    the new class; nothing ran these before

Before anything is timed, the two LSTM pairs run the same batch on the same weights: the one-directional pair must agree to 1e-5
(two different summation orders), the bidirectional pair bit for bit.
Timing: 5 untimed calls per leg, then 5 rounds; a round times one block of 20 calls of each leg, one after the other (interleaved),
each block between two synchronisations.  Reported: the median block and the spread, milliseconds per call."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feature_store_ab import BLOCKS, STEPS, WARM, interleaved_ms       # noqa: E402  (the same timing loop)

B, S, E, ENC, VOCAB, SEED = 64, 50, 300, 512, 90, 1234


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "encoder_cells_ab.txt"))
    ap.add_argument("--json", default=None, help="also write the figures as JSON")
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("encoder_cells_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(SEED)
    lengths = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
    lengths[0] = S
    q = torch.randint(1, VOCAB + 1, (B, S), generator=g, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    q, lengths = q.to(dev), lengths.to(dev)
    d_words, d_vec = torch.randn(B, S, ENC, generator=g).to(dev) / B, torch.randn(B, ENC, generator=g).to(dev) / B

    def config(cell, bi):
        return macx.configs.flag_file_config("args", encType=cell, encBi=bi, encDim=ENC, ctrlDim=ENC, wrdEmbDim=E)

    def build(cls, cell, bi):
        return cls(config(cell, bi), VOCAB, generator=torch.Generator().manual_seed(SEED)).to(dev)

    encs = {"LSTM 1 dir, generic": build(macx.QuestionEncoder, "LSTM", False),
            "LSTM 1 dir, recurrent": build(macx.RecurrentQuestionEncoder, "LSTM", False),
            "LSTM 2 dir, fused": build(macx.QuestionEncoder, "LSTM", True),
            "LSTM 2 dir, recurrent": build(macx.RecurrentQuestionEncoder, "LSTM", True)}
    for cell in ("GRU", "RNN"):
        for bi in (False, True):
            encs["%s %d dir, recurrent" % (cell, 2 if bi else 1)] = build(macx.RecurrentQuestionEncoder, cell, bi)
    assert type(encs["LSTM 1 dir, generic"]) is macx.GenericQuestionEncoder and type(encs["LSTM 2 dir, fused"]) is macx.QuestionEncoder
    for a, b in (("LSTM 1 dir, generic", "LSTM 1 dir, recurrent"), ("LSTM 2 dir, fused", "LSTM 2 dir, recurrent")):
        encs[b].load_reference_dict(encs[a].to_reference_dict())

    def call(enc):
        def one():
            for t in enc.tensors():
                t.grad = None
            words, vec = enc(q, lengths, train=True, seed=SEED, check_ids=False)
            torch.autograd.backward([words, vec], [d_words, d_vec])
            return words, vec
        return one

    def results(enc):
        words, vec = call(enc)()
        torch.cuda.synchronize()
        return [words.detach(), vec.detach()] + [t.grad for t in enc.tensors()]

    def worst(a, b):
        return max(float((x.double() - y.double()).abs().max() / max(float(y.double().abs().max()), 1e-7)) for x, y in zip(a, b))

    uni = worst(results(encs["LSTM 1 dir, recurrent"]), results(encs["LSTM 1 dir, generic"]))
    bi_equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                   for x, y in zip(results(encs["LSTM 2 dir, recurrent"]), results(encs["LSTM 2 dir, fused"])))
    fig = interleaved_ms(torch, {k: call(e) for k, e in encs.items()})
    res = {"legs": fig, "lstm_1dir_worst_relative_difference": uni, "lstm_2dir_bit_identical": bi_equal}
    lines = ["the question encoder alone, forward + backward in train mode, eager launches, one process (tools/encoder_cells_ab.py)",
             "B=%d S=%d wrdEmbDim=%d encDim=%d vocabulary %d; %s; torch %s" % (B, S, E, ENC, VOCAB, torch.cuda.get_device_name(0), torch.__version__),
             "per leg: %d untimed calls, then %d interleaved blocks of %d; ms per call: median block (fastest .. slowest block)" % (WARM, BLOCKS, STEPS),
             "one batch on the same weights first: LSTM 1 dir recurrent against generic, outputs and gradients, worst relative difference %.2e; "
             "LSTM 2 dir recurrent against fused: %s" % (uni, "bit-identical" if bi_equal else "DIFFER"), ""]
    for k, f in fig.items():
        lines.append("  %-24s %8.3f  (%.3f .. %.3f)" % (k, f["median_ms"], f["min_ms"], f["max_ms"]))
    ratio = lambda a, b: fig[a]["median_ms"] / fig[b]["median_ms"]
    lines += ["", "  LSTM 1 dir: generic / recurrent = %.2f" % ratio("LSTM 1 dir, generic", "LSTM 1 dir, recurrent"),
              "  LSTM 2 dir: fused / recurrent   = %.3f" % ratio("LSTM 2 dir, fused", "LSTM 2 dir, recurrent")]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
