"""Records tests/golden/eval_records/preds_list.json: what the reference's own MACnet.buildPredsList (model.py:693-710), unmodified,
returns for a small batch -- the fixture tests/test_eval_records_host.py holds macx.EvalRecords.instances(trim=False) to.

    MACX_REFERENCE_DIR=<upstream checkout> python tools/record_preds_list.py

The reference is imported by tests/ref_exec.py's route (MACX_REFERENCE_DIR, against tests/tf1_shim); `self` is a stand-in whose
answerDict.decodeId is a list lookup.  Inputs: B = 3 questions, p = 2 steps, N = 4 cells, S = 5 words, with self-attention; fp32 maps
drawn from a seeded generator (rows normalised like attention, zeros behind each question's length / knowledge-base size and
behind entry i of self-attention row i, whole rows of p entries as the run's buffer holds them).  The file
holds lists, strings and numbers only: the inputs (so that the test can replay them without the reference) and the returned list."""
import copy
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "eval_records", "preds_list.json")
B, P, N, S = 3, 2, 4, 5
ANSWERS = ["no", "yes", "cube", "sphere", "2"]
LENGTHS, KB_LENGTHS = [5, 2, 3], [4, 3, 1]


def attention(rng, width, lengths):
    """[P][B, width] float32: positive rows that sum to one over each question's live columns, exact zeros behind them.
    lengths: [B], or a function of the step (self-attention: step i looks at i + 1 entries)"""
    out = []
    for i in range(P):
        live = np.asarray(lengths(i) if callable(lengths) else lengths)
        a = rng.random((B, width)).astype(np.float32) + np.float32(0.05)
        a *= (np.arange(width)[None, :] < live[:, None]).astype(np.float32)
        out.append((a / a.sum(axis=1, keepdims=True)).astype(np.float32))
    return out


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_exec
    if not ref_exec.available():
        raise SystemExit("MACX_REFERENCE_DIR must name a checkout of the reference")
    model = ref_exec.load()["model"]
    rng = np.random.default_rng(20240607)
    maps = {"kb": attention(rng, N, KB_LENGTHS), "question": attention(rng, S, LENGTHS), "self": attention(rng, P, lambda i: [i + 1] * B)}
    instances = [{"index": 10 + b, "question": "q%d" % b, "imageId": "CLEVR_val_%06d" % (b // 2), "answer": ANSWERS[b]} for b in range(B)]
    predictions = [1, 4, 2]
    stand_in = SimpleNamespace(answerDict=SimpleNamespace(decodeId=lambda i: ANSWERS[i]))
    preds_list = model.MACnet.buildPredsList(stand_in, {"instances": copy.deepcopy(instances)}, np.asarray(predictions), maps)
    record = {"B": B, "p": P, "N": N, "S": S, "answers": ANSWERS, "lengths": LENGTHS, "kb_lengths": KB_LENGTHS, "instances": instances,
              "predictions": predictions, "maps": {k: [step.tolist() for step in v] for k, v in maps.items()}, "preds_list": preds_list}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
