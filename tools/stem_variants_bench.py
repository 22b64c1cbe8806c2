#!/usr/bin/env python3
"""Forward + backward time of the generic stem (GenericStem on macx_conv2d_*) at B = 64 on 14 x 14 x 1024 features, training
mode, for a few stem option sets, next to the fused Stem on the default shape.  Prints one JSON line: ms per forward + backward
and the achieved TF/s (convolution FLOPs of the forward, backward-data where it runs, and kernel gradient) against the
157 TF/s fp32-MFMA peak of the MI355X.

    python tools/stem_variants_bench.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import macx  # noqa: E402

PEAK_TF = 157.0
CASES = {
    "default_generic": {},
    "three_layers": dict(stemNumLayers=3),
    "strides_2_1": dict(stemStrideSizes=[2, 1]),
    "location_PE": dict(locationAware=True, locationType="PE"),
    "default_fused": {},
}


def conv_flops(stem, B, H, W):
    """2 * MACs of each layer's forward; backward = kernel gradient (same) + backward-data (same, except layer 0: images are
    inputs and get no gradient)"""
    total, hh, ww = 0.0, H, W
    layers = stem.layers if isinstance(stem, macx.GenericStem) else [(3, 1, stem.inDim, stem.midDim), (3, 1, stem.midDim, stem.outDim)]
    for i, (k, s, cin, cout) in enumerate(layers):
        hh, ww = -(-hh // s), -(-ww // s)
        f = 2.0 * B * hh * ww * k * k * cin * cout
        total += f * (3 if i > 0 else 2)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, Cin = 64, 14, 14, 1024
    img = torch.relu(torch.randn(B, H * W, Cin, generator=torch.Generator().manual_seed(0))).to(dev)
    out = {"metric": "generic stem fwd+bwd, B=64, 14x14x1024 -> 512 -> 512 (train mode)", "unit": "ms", "peak_tf": PEAK_TF, "cases": {}}
    for name, flags in CASES.items():
        cfg = SimpleNamespace(memDim=512, stemDim=512, stemDropout=0.82, relu="STD", **flags)
        cls = macx.Stem if name == "default_fused" else macx.GenericStem
        stem = cls(cfg, H=H, W=W, inDim=Cin, generator=torch.Generator().manual_seed(1)).to(dev)
        d = None

        def step(i):
            nonlocal d
            kb = stem(img, train=True, seed=i)
            if d is None:
                d = torch.randn(kb.shape, generator=torch.Generator().manual_seed(2)).to(dev)
            (kb * d).sum().backward()

        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.iters):
            step(i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.iters * 1e3
        tf = conv_flops(stem, B, H, W) / (ms * 1e-3) / 1e12
        out["cases"][name] = {"ms": round(ms, 3), "tflops": round(tf, 1), "pct_peak": round(100 * tf / PEAK_TF, 1),
                              "kb_cells": stem.out_hw[0] * stem.out_hw[1]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
