#!/usr/bin/env python3
"""Static instruction counts per stage of a chain kernel (CPU only: needs hipcc, no GPU).

    python tools/stage_insts.py --tu macx_chain_bwd.hip --kernel "chain_bwd_kernel<512,4,3,64>"
    python tools/stage_insts.py --tu macx_chain_fwd.hip --kernel "chain_fwd_kernel<512,4,64>" [--csrc DIR] [--asm FILE]

Compiles one translation unit of mac-network_amd/csrc to gfx950 assembly (hipcc -S --cuda-device-only -DMACX_STAGE_MARKS) and
counts instruction CLASSES between the assembler comments `; MACX_STAGE <name>` that the kernels emit under that define
(MACX_MARK, macx_common.hip.h; the product build has none).  A stage is what lies between two consecutive markers in the
listing: it holds every variant of a run-time switch (all five activations where a stage switches on one) and whatever
blocks the compiler laid out there, so the figures are per wave and static -- a yardstick for the vector work of a
stage, not a cycle count.

Classes: VALU (v_* without the matrix and accumulator-move instructions), selects (v_cndmask, split into the e32 form that
reads VCC and the e64 / other forms), compares (v_cmp*), DPP (any *_dpp), s_nop (instructions, and the wait states they
stand for), LDS (ds_*), global (global_* / buffer_* / flat_*), MFMA, scalar (every other s_*).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-network_amd", "csrc")

STAGE_NAMES = {
    ("bwd 0", "bwd 1"): "B0",
    ("bwd 1", "bwd 2"): "B1 product",
    ("bwd 2", "bwd 3"): "B1 epilogue + emit",
    ("bwd 3", "bwd 4"): "B2 first product",
    ("bwd 4", "bwd 5"): "dy sums + (.)y",
    ("bwd 5", "bwd 6"): "B2 second product",
    ("bwd 6", "bwd 7"): "last epilogue",
    ("fwd 0", "fwd 1"): "X product",
    ("fwd 1", "fwd 2"): "X epilogue",
    ("fwd 2", "fwd 3"): "X W1b product",
    ("fwd 3", "fwd 4"): "X(.)y conversion",
    ("fwd 4", "fwd 5"): "(X(.)y) W1a product",
    ("fwd 5", "fwd 6"): "H1 epilogue",
    ("fwd 6", "fwd 7"): "H1 W2 product",
    ("fwd 7", "fwd 8"): "I2 epilogue + logits",
}
COLUMNS = ("VALU", "cnd_e32", "cnd_e64", "v_cmp", "DPP", "s_nop", "nop_states", "LDS", "global", "MFMA", "scalar")


def mangled_fragment(kernel):
    """'chain_bwd_kernel<512,4,3,64>' -> 'chain_bwd_kernelILi512ELi4ELi3ELi64EEE' (Itanium: integer template arguments)"""
    m = re.fullmatch(r"\s*(\w+)\s*(?:<([^>]*)>)?\s*", kernel)
    if not m:
        raise SystemExit("cannot read kernel name %r" % kernel)
    name, args = m.group(1), m.group(2)
    if args is None:
        return name
    out = "%d%sI" % (len(name), name)
    for a in args.split(","):
        if a.strip() in ("true", "false"):
            out += "Lb%dE" % (a.strip() == "true")
            continue
        v = int(a)
        out += "Li%s%dE" % ("n" if v < 0 else "", abs(v))
    return out + "E"


def compile_asm(tu, csrc, defines):
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed", "-Wno-inline-asm",
           "-DMACX_STAGE_MARKS", "-I", os.path.join(ROOT, "include"), os.path.join(csrc, tu), "-o", out]
    cmd += ["-D" + d for d in defines]
    subprocess.run(cmd, check=True)
    return out


def kernel_body(lines, frag):
    """the lines between the kernel's label and its function-end label"""
    start = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_][\w$.]*:", l) and frag in l.split(":")[0] and not l.startswith(".")]
    if not start:
        names = sorted({l.split(":")[0] for l in lines if l.startswith("_Z") and ":" in l and "kernel" in l})
        raise SystemExit("no kernel matches %r; the listing has:\n  %s" % (frag, "\n  ".join(names)))
    if len(start) > 1:
        raise SystemExit("%r matches %d kernels: %s" % (frag, len(start), [lines[i].split(":")[0] for i in start]))
    i = start[0]
    for j in range(i + 1, len(lines)):
        if lines[j].startswith(".Lfunc_end"):
            return lines[i + 1:j]
    return lines[i + 1:]


def classify(mn, operands, row):
    if mn.startswith("v_mfma") or mn.startswith("v_smfmac"):
        row["MFMA"] += 1
    elif mn.startswith("v_accvgpr"):
        pass
    elif mn.startswith("v_"):
        row["VALU"] += 1
        if mn.startswith("v_cndmask"):
            row["cnd_e32" if mn.endswith("_e32") else "cnd_e64"] += 1
        elif mn.startswith("v_cmp"):
            row["v_cmp"] += 1
        if mn.endswith("_dpp") or "row_" in operands or "quad_perm" in operands:
            row["DPP"] += 1
    elif mn == "s_nop":
        row["s_nop"] += 1
        row["nop_states"] += int(operands.strip() or "0", 0) + 1
    elif mn.startswith("ds_"):
        row["LDS"] += 1
    elif mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        row["global"] += 1
    elif mn.startswith("s_") and not mn.startswith("s_waitcnt"):
        row["scalar"] += 1


def count(body):
    stages, cur = [], "(entry)"
    row = dict.fromkeys(COLUMNS, 0)
    for l in body:
        t = l.strip()
        m = re.match(r";\s*MACX_STAGE\s+(.*\S)", t)
        if m:
            stages.append((cur, row))
            cur, row = m.group(1), dict.fromkeys(COLUMNS, 0)
            continue
        if not t or t.startswith((";", ".", "//")) or re.match(r"^[\w$.]+:", t):
            continue
        t = t.split(";")[0].strip()
        if not t:
            continue
        parts = t.split(None, 1)
        classify(parts[0], parts[1] if len(parts) > 1 else "", row)
    stages.append((cur, row))
    return stages


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tu", default="macx_chain_bwd.hip", help="translation unit under csrc/")
    ap.add_argument("--kernel", default="chain_bwd_kernel<512,4,3,64>", help="kernel name with its integer template arguments")
    ap.add_argument("--csrc", default=CSRC, help="source directory (default: this tree's)")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--keep", help="keep the listing under this name")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="further build defines")
    args = ap.parse_args()
    path = args.asm or compile_asm(args.tu, args.csrc, args.defines)
    with open(path) as fh:
        lines = fh.read().splitlines()
    if args.keep:
        os.replace(path, args.keep)
    elif not args.asm:
        os.unlink(path)
    stages = count(kernel_body(lines, mangled_fragment(args.kernel)))
    print("# %s (%s): static instructions per wave between stage markers" % (args.kernel, args.tu))
    print("%-34s" % "stage" + "".join("%11s" % c for c in COLUMNS))
    total = dict.fromkeys(COLUMNS, 0)
    for k, (name, row) in enumerate(stages):
        nxt = stages[k + 1][0] if k + 1 < len(stages) else "(end)"
        label = "%s .. %s" % (name, nxt)
        human = STAGE_NAMES.get((name, nxt))
        if human:
            label = "%s [%s]" % (human, name.split()[-1] + "-" + nxt.split()[-1])
        print("%-34s" % label + "".join("%11d" % row[c] for c in COLUMNS))
        for c in COLUMNS:
            total[c] += row[c]
    print("%-34s" % "whole kernel" + "".join("%11d" % total[c] for c in COLUMNS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
