#!/usr/bin/env python3
"""Records tests/golden/chain_bits/<case>.json: a SHA-256, the shape and the largest magnitude of every output tensor (final state,
attention maps, every gradient) of the cases of tests/chain_bits_cases.py, as the checkout it is run from computes them.

Run on an MI355X FROM A CHECKOUT OF THE COMMIT WHOSE BITS ARE THE REFERENCE -- for tests/test_gpu_chain_segments.py that is the
parent of the change that took the per-value selects out of the chain kernels (33b8871) -- with this file and
tests/chain_bits_cases.py copied into it:

    python tests/golden/make_chain_bits.py [--out DIR] [case ...]

The fixtures hold no arrays: the test recomputes the tensors and compares digests.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import macx
    import chain_bits_cases as cb
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "chain_bits"))
    ap.add_argument("cases", nargs="*", default=list(cb.CASES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the fixtures are what the GPU kernels compute"
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    for name in args.cases:
        out, _ = cb.run_case(macx, dev, name)
        again, _ = cb.run_case(macx, dev, name)              # a reference that is not reproducible is no reference
        rec = {k: cb.digest(v) for k, v in out.items()}
        for k, v in again.items():
            assert cb.digest(v)["sha256"] == rec[k]["sha256"], "%s: %s differs between two runs" % (name, k)
        with open(os.path.join(args.out, name + ".json"), "w") as fh:
            json.dump({"case": name, "tensors": rec}, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("%-20s %d tensors, memory max |value| %.4g" % (name, len(rec), rec["memory"]["max_abs"]))


if __name__ == "__main__":
    main()
