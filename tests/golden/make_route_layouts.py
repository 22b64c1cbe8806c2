#!/usr/bin/env python3
"""Records tests/golden/route_layouts.json: what the sizing exports (macx_saved_floats, macx_ws_floats(.., 1), macx_saved_segment of
every MACX_SEG_*) answer over the grid of tests/route_cases.py -- flag file x kernel family x keep x tuning key x shape -- as the
checkout it is run from computes them.  Integers only; no GPU is needed.

Run FROM A CHECKOUT OF THE COMMIT WHOSE LAYOUTS ARE THE REFERENCE -- for tests/test_route_host.py that is the parent of the change
that gave the fused cell one route plan -- with this file and tests/route_cases.py copied into it:

    python tests/golden/make_route_layouts.py [--out FILE]

Format: "shapes" the grid's shapes; "heads"[flag file][shape index] the (offset, count) of the segments in front of the status
words, which depend on neither family, keep nor tuning table (asserted here); "points"["flag file|family|keep|tune"][shape index] =
[saved floats, workspace floats, the status segment's (offset, count)] -- or the error code in the last place and zeros before it
where macx_check refuses the combination (a d_logical cell off the H2 family).
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
    import macx
    import route_cases as rc
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "route_layouts.json"))
    args = ap.parse_args()
    shapes = rc.layout_shapes()
    heads = {f: [None] * len(shapes) for f in rc.FLAG_FILES}
    points = {}
    for flags in rc.FLAG_FILES:
        for family in rc.FAMILIES:
            for tune in rc.TUNES:
                for keep in (0, 1):
                    rows = []
                    for k, shape in enumerate(shapes):
                        opts, sh = rc.frozen(macx, flags, shape, family, tune)
                        lay = rc.layout(macx, opts, sh, keep)
                        head, status = lay[2:-1], lay[-1]
                        if isinstance(status, list):
                            assert heads[flags][k] in (None, head), (flags, family, tune, keep, shape)
                            heads[flags][k] = head
                        else:
                            assert lay[:2] == [0, 0] and all(h == status for h in head), (flags, family, tune, keep, shape)
                        rows.append([lay[0], lay[1], status])
                    points["%s|%s|%d|%s" % (flags, family, keep, rc.tune_id(tune))] = rows
    with open(args.out, "w") as fh:
        json.dump({"shapes": shapes, "heads": heads, "points": points}, fh, separators=(",", ":"))
        fh.write("\n")
    print("%s: %d points, %d bytes" % (args.out, sum(len(r) for r in points.values()), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
