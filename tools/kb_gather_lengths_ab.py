#!/usr/bin/env python3
"""A/B of the length-aware gather (macx_kb_gather_l / macx_kb_gather_bwd_l) against the plain one, same process, same buffers.

    python tools/kb_gather_lengths_ab.py [--out profiles/kb_gather_lengths_ab.txt]

The workload's block: B = 64 questions over G = 7 images (index b // 10), N = 196 cells, d = 512 -- 25.7 MB written forward, 2.8 MB
backward.  Legs, forward and backward each: the plain call; the `_l` call with every size N (the same bytes through the new kernel);
the `_l` call with sizes drawn uniformly from [1, N] (about half the reads, every write).  Results of the full-size `_l` legs are
compared with the plain ones bit for bit before anything is timed.  Timing: 20 untimed calls per leg, then 5 rounds; a round times
one block of 200 calls of each leg, one after the other (interleaved), each block between two synchronisations.  Reported:
microseconds per call, median block and spread.  Nothing here prices the cell: it computes the padded rows whatever the gather does."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

BLOCKS, CALLS, WARM = 5, 200, 20
B, G, N, D, PER_IMAGE = 64, 7, 196, 512, 10


def interleaved_us(torch, legs):
    for one in legs.values():
        for _ in range(WARM):
            one()
    out = {k: [] for k in legs}
    for _ in range(BLOCKS):
        for k, one in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                one()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / CALLS * 1e6)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--out", default=os.path.join(root, "profiles", "kb_gather_lengths_ab.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    import torch
    import macx
    if not torch.cuda.is_available():
        raise SystemExit("kb_gather_lengths_ab.py measures on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    L = macx._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator().manual_seed(1234)
    src, dkb = torch.randn(G, N, D, generator=g).to(dev), torch.randn(B, N, D, generator=g).to(dev)
    index = (torch.arange(B, dtype=torch.int32) // PER_IMAGE).to(dev)
    full = torch.full((G,), N, dtype=torch.int32, device=dev)
    drawn = torch.randint(1, N + 1, (G,), generator=g, dtype=torch.int32)
    short = drawn.to(dev)
    kb, kb_l, lens = torch.empty(B, N, D, device=dev), torch.empty(B, N, D, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    out, out_l = torch.empty(G, N, D, device=dev), torch.empty(G, N, D, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def ok(rc):
        macx._lib.check(rc, "gather")

    fwd = lambda: ok(L.macx_kb_gather(p(src), p(index), G, B, N, D, p(kb), st))
    fwd_l = lambda sizes: (lambda: ok(L.macx_kb_gather_l(p(src), p(index), p(sizes), G, B, N, D, p(kb_l), p(lens), st)))
    bwd = lambda: ok(L.macx_kb_gather_bwd(p(dkb), p(index), G, B, N, D, p(out), st))
    bwd_l = lambda sizes: (lambda: ok(L.macx_kb_gather_bwd_l(p(dkb), p(index), p(sizes), G, B, N, D, p(out_l), st)))
    fwd(), fwd_l(full)(), bwd(), bwd_l(full)()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((kb, kb_l), (out, out_l)))
    figs = interleaved_us(torch, {"forward  plain": fwd, "forward  _l, sizes N": fwd_l(full), "forward  _l, sizes drawn": fwd_l(short),
                                  "backward plain": bwd, "backward _l, sizes N": bwd_l(full), "backward _l, sizes drawn": bwd_l(short)})
    lines = ["macx_kb_gather_l / _bwd_l against macx_kb_gather / _bwd, one process (tools/kb_gather_lengths_ab.py)",
             "B=%d G=%d N=%d d=%d, image_index = b // %d; %s; torch %s" % (B, G, N, D, PER_IMAGE, torch.cuda.get_device_name(0), torch.__version__),
             "sizes drawn: %s (live share of the rows a question copies: %.2f)" % (drawn.tolist(), float(drawn[index.cpu().long()].float().mean()) / N),
             "_l with every size N against the plain call, forward and backward: %s" % ("bit-identical" if same else "DIFFERENT"),
             "per leg: %d untimed calls, then %d interleaved blocks of %d calls; us per call: median block (fastest .. slowest block)"
             % (WARM, BLOCKS, CALLS), ""]
    for k, (med, lo, hi) in figs.items():
        lines.append("  %-26s %8.2f  (%.2f .. %.2f)" % (k, med, lo, hi))
    lines += ["", "A call this short is about what the host takes to issue one: the figures bound each kernel from above, they do not rank them.",
              "The cell computes the padded rows whatever the gather does: no step time is claimed from these figures."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
