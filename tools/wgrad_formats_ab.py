#!/usr/bin/env python3
"""Bit equality and timing of the producer/consumer weight-gradient kernels (wgrad_split_kernel in macx_wgrad6.hip.h: the bf16x3 and
fp16x2 operand formats) between two trees, one process per tree, fixed seeds.

    python tools/wgrad_formats_ab.py --json THIS_TREE.json [--no-timing]
    python tools/wgrad_formats_ab.py --compare PARENT.json NEW.json [--repeat PARENT_AGAIN.json]

Run it once in each tree (the file copied into the other one); it uses nothing but the C ABI and the Python layer, which the two
trees share.  Cases, each hashed (SHA-256 of every output buffer's bytes):

    wgrad/f<1|2>/<M>x<Kd>x<Jd>   macx_wgrad in families 1 and 2: M=64 128x128 (one tile, JW=1), M=64 128x256 (JW=2), M=257 256x384
                                 (JW=1, ragged last 32-row chunk), M=1001 128x256 (macx_wgrad_splits > 1: slabs + slab_reduce)
    cell/d<128|256>              one fused-cell backward, B=3, p=2: the [B,d] linears' gradients through the TnList launch
    stem/f<1|2>/<B>x<H>x<W>      Stem forward + backward with channels (128, 256, 384): JW=2 for layer 0, JW=1 for layer 1; B=2 with a
                                 13 x 16 map and B=1 with a 15 x 15 map.  Family 2 runs the fp16x2 format, family 1 the bf16x3 one.

Timing (feature_store_ab.py's interleaved block timer: 5 untimed calls per leg, then 5 rounds of one block per leg, each block between two
synchronisations): the four macx_wgrad shapes in both families, 200 calls per block, and the stem's forward + backward at the workload's
B=64, 14 x 14, 1024 -> 512 -> 512 in both families, 10 calls per block.

--compare: every hash of the two files must be equal (exit status 1 otherwise).  Timings are printed side by side; with --repeat (a
second run of the first tree) each leg's noise figure is the larger max - min of the block medians of the first tree's two runs, and a
leg passes when the second tree's median is no slower than the first tree's slower median plus that figure."""
import argparse
import hashlib
import json
import os
import sys

SEED = 1234
WGRAD_SHAPES = [(64, 128, 128), (64, 128, 256), (257, 256, 384), (1001, 128, 256)]     # the last: nsplit > 1
STEM_CH = (128, 256, 384)
STEM_GEOMETRY = [(2, 13, 16), (1, 15, 15)]
STEM_TIMED = (64, 14, 14, (1024, 512, 512))
CELL = dict(name="args", B=3, S=9, N=49, p=2)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def wgrad_call(macx, torch, dev, M, Kd, Jd):
    """(callable, out): macx_wgrad on contiguous N(0,1) operands; asserts nothing about nsplit"""
    L, ptr = macx._lib.lib(), macx._lib.ptr
    g = torch.Generator().manual_seed(M * 131 + Kd + Jd)
    A = torch.randn(M, Kd, generator=g).to(dev)
    G = torch.randn(M, Jd, generator=g).to(dev)
    ns = L.macx_wgrad_splits(M, Kd, Jd)
    assert ns >= 1, ns
    out = torch.zeros(Kd, Jd, device=dev)
    ws = torch.zeros(ns * Kd * Jd, device=dev)

    def one():
        macx._lib.check(L.macx_wgrad(ptr(A), Kd, ptr(G), Jd, M, Kd, Jd, ptr(out), ptr(ws), macx._lib.stream_of(out)), "macx_wgrad")
    one.keep = (A, G, ws)
    return one, out, ns


def stem_call(macx, torch, dev, B, H, W, ch):
    """(callable -> {name: tensor}): Stem forward + backward on relu(randn) images and a randn / B cotangent, training mode"""
    cfg = macx.configs.flag_file_config("args", memDim=ch[2], ctrlDim=ch[2], attDim=ch[2])
    cfg.stemDim = ch[1]
    stem = macx.Stem(cfg, H=H, W=W, inDim=ch[0], generator=torch.Generator().manual_seed(1)).to(dev)
    g = torch.Generator().manual_seed(2)
    img = torch.relu(torch.randn(B, H * W, ch[0], generator=g)).to(dev)
    dout = (torch.randn(B, H * W, ch[2], generator=g) / B).to(dev)

    def one():
        for p in stem.parameters():
            p.grad = None
        kb = stem(img, train=True, seed=5, b0=1)
        (kb * dout).sum().backward()
        return dict([("kb", kb)] + [(f, getattr(stem, f).grad) for f in stem.FIELDS])
    return one


def cell_case(macx, torch, dev, d):
    c = CELL
    cfg = macx.configs.flag_file_config(c["name"], netLength=c["p"], memDim=d, ctrlDim=d, attDim=d)
    vq, words, lengths, kb = macx.configs.synthetic_inputs(c["B"], c["S"], c["N"], d, seed=SEED)
    params = macx.MACCellParams(cfg, c["p"], generator=torch.Generator().manual_seed(5)).to(dev)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (vq, words, kb)]
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=lengths.to(dev), knowledgeBase=kbd,
                        memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout,
                        batchSize=c["B"], train=True, config=cfg, params=params, seed=5)
    g = torch.Generator().manual_seed(9)
    dmem = (torch.randn(c["B"], d, generator=g) / c["B"]).to(dev)
    dctl = (torch.randn(c["B"], d, generator=g) / c["B"]).to(dev)
    state = cell.run()
    ((state.memory * dmem).sum() + (state.control * dctl).sum()).backward()
    torch.cuda.synchronize()
    out = {"memory": state.memory, "d_vecQuestions": vqd.grad, "d_words": wd.grad, "d_knowledgeBase": kbd.grad}
    for f in params.fields:
        out["d_" + f] = getattr(params, f).grad
    return {k: sha(v) for k, v in out.items()}


def run(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import torch
    import macx
    from feature_store_ab import interleaved_ms
    if not torch.cuda.is_available():
        raise SystemExit("wgrad_formats_ab.py runs on the HIP device; there is none here")
    dev = torch.device("cuda:0")
    L = macx._lib.lib()
    default = L.macx_gemm_mode(-1)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "default_family": default, "hashes": {}, "nsplit": {},
           "timing": {}}
    legs_wgrad, legs_stem = {}, {}
    try:
        for fam in (1, 2):
            assert L.macx_gemm_mode(fam) == fam
            for M, Kd, Jd in WGRAD_SHAPES:
                key = "wgrad/f%d/%dx%dx%d" % (fam, M, Kd, Jd)
                one, out, ns = wgrad_call(macx, torch, dev, M, Kd, Jd)
                one()
                torch.cuda.synchronize()
                res["hashes"][key] = {"out": sha(out)}
                res["nsplit"][key] = ns
                legs_wgrad[key] = (fam, one)
            assert res["nsplit"]["wgrad/f%d/%dx%dx%d" % ((fam,) + WGRAD_SHAPES[-1])] > 1, "the slab case runs on one slab"
            for B, H, W in STEM_GEOMETRY:
                got = stem_call(macx, torch, dev, B, H, W, STEM_CH)()
                torch.cuda.synchronize()
                res["hashes"]["stem/f%d/%dx%dx%d" % (fam, B, H, W)] = {k: sha(v) for k, v in got.items()}
        L.macx_gemm_mode(default)
        for d in (128, 256):
            res["hashes"]["cell/d%d" % d] = cell_case(macx, torch, dev, d)
        if not args.no_timing:
            def in_family(fam, one):
                def leg():
                    L.macx_gemm_mode(fam)
                    one()
                return leg
            res["timing"].update(interleaved_ms(torch, {k: in_family(f, one) for k, (f, one) in legs_wgrad.items()}, steps=200))
            B, H, W, ch = STEM_TIMED
            one = stem_call(macx, torch, dev, B, H, W, ch)
            for fam in (1, 2):
                legs_stem["stem_fwd_bwd/f%d/%dx%dx%d-%d-%d-%d" % ((fam, B, H, W) + ch)] = in_family(fam, one)
            res["timing"].update(interleaved_ms(torch, legs_stem, steps=10))
    finally:
        L.macx_gemm_mode(default)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("%d hashed cases, %d timed legs -> %s" % (len(res["hashes"]), len(res["timing"]), args.json))
    for k, v in sorted(res["timing"].items()):
        print("  %-44s %9.4f ms  (%.4f .. %.4f)" % (k, v["median_ms"], v["min_ms"], v["max_ms"]))


def compare(a_path, b_path, repeat_path):
    load = lambda p: json.load(open(p))
    a, b = load(a_path), load(b_path)
    a2 = load(repeat_path) if repeat_path else None
    bad = []
    keys = sorted(set(a["hashes"]) | set(b["hashes"]))
    nbuf = 0
    for k in keys:
        ha, hb = a["hashes"].get(k, {}), b["hashes"].get(k, {})
        for name in sorted(set(ha) | set(hb)):
            nbuf += 1
            if ha.get(name) is None or ha.get(name) != hb.get(name):
                bad.append("%s %s: %s != %s" % (k, name, str(ha.get(name))[:16], str(hb.get(name))[:16]))
    if a2 is not None and a2["hashes"] != a["hashes"]:
        bad.append("the first tree's two runs differ from each other")
    print("A = %s, B = %s%s" % (a_path, b_path, ", A again = %s" % repeat_path if a2 else ""))
    print("hashes: %d cases, %d buffers, %d differ" % (len(keys), nbuf, len(bad)))
    for line in bad:
        print("  DIFFERS " + line)
    missed = []
    if a["timing"] and b["timing"]:
        print("timing, ms per call: median block (fastest .. slowest block)")
        for k in sorted(a["timing"]):
            ta, tb = a["timing"][k], b["timing"].get(k)
            if tb is None:
                continue
            text = "  %-44s A %9.4f (%.4f .. %.4f)" % (k, ta["median_ms"], ta["min_ms"], ta["max_ms"])
            if a2 is not None:
                tr = a2["timing"][k]
                noise = max(ta["max_ms"] - ta["min_ms"], tr["max_ms"] - tr["min_ms"])
                bound = max(ta["median_ms"], tr["median_ms"]) + noise
                ok = tb["median_ms"] <= bound
                text += "  A again %9.4f (%.4f .. %.4f)  noise %.4f" % (tr["median_ms"], tr["min_ms"], tr["max_ms"], noise)
                text += "  B %9.4f (%.4f .. %.4f)  bound %.4f  %s" % (tb["median_ms"], tb["min_ms"], tb["max_ms"], bound,
                                                                       "pass" if ok else "MISS")
                if not ok:
                    missed.append(k)
            else:
                text += "  B %9.4f (%.4f .. %.4f)  B / A %.3f" % (tb["median_ms"], tb["min_ms"], tb["max_ms"],
                                                                  tb["median_ms"] / ta["median_ms"])
            print(text)
        if a2 is not None:
            print("legs past their bound: %s" % (", ".join(missed) or "none"))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="run the cases in this tree and write hashes and timings here")
    ap.add_argument("--no-timing", action="store_true", help="hashes only")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--repeat", help="with --compare: a second run of tree A, for the noise figures")
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(args.compare[0], args.compare[1], args.repeat))
    if not args.json:
        ap.error("--json FILE or --compare A.json B.json")
    run(args)


if __name__ == "__main__":
    main()
