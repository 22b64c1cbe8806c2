"""-m gpu: the chain kernels' per-question (segment) logic, bit for bit against the commit before its selects became row masks.

tests/golden/chain_bits/<case>.json (tests/golden/make_chain_bits.py, run on an MI355X from a checkout of 33b8871) holds a SHA-256 per
output tensor of the full cell -- final memory and control, the attention maps of every step, every gradient.  The change that
introduced the two-question chain_bwd kernel, the bit-mask forms of its per-question sums and keep factor, and the side-by-side
column reductions is an exact rewrite: every digest must match.  Where one does not, the failure also says how far the tensor is
from the fp64 oracle at the tolerances of tests/test_gpu_cell.py (FWD_TOL 2e-5, GRAD_TOL 2e-4, attention 2e-6 absolute), so that a
mismatch reads as "rounds differently" or as "wrong".

Cases and why these shapes: tests/chain_bits_cases.py.
"""
import json
import os

import pytest

import chain_bits_cases as cb
from helpers import oracle_run, rel_err, max_abs

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5     # tests/test_gpu_cell.py
GRAD_TOL = 2e-4
ATT_TOL = 2e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_bits")


def _oracle_errors(macx, ctx, out):
    """{tensor: (error against the fp64 oracle, its tolerance)} for a run of cb.run_case"""
    import contextlib
    cfg, params = ctx["cfg"], ctx["params"]
    p = cfg.netLength
    masked = contextlib.nullcontext()
    if ctx["kb_lengths"] is not None:
        from kb_lengths_ref import masked_kb_attention
        masked = masked_kb_attention(ctx["kb_lengths"], ctx["kb"].shape[1])
    with masked:
        ref = oracle_run(cfg, params.to_reference_dict(), ctx["vq"], ctx["words"], ctx["lengths"], ctx["kb"], train=True, seed=5,
                         need_grad=True, d_memory=ctx["dmem"], d_control=ctx["dctl"])
    rc = ref["cell"]
    errs = {"memory": (rel_err(out["memory"], ref["memory"]), FWD_TOL), "control": (rel_err(out["control"], ref["control"]), FWD_TOL)}
    for i in range(p):
        errs["att_kb_%d" % i] = (max_abs(out["att_kb_%d" % i], rc.attentions["kb"][i]), ATT_TOL)
        errs["att_question_%d" % i] = (max_abs(out["att_question_%d" % i], rc.attentions["question"][i]), ATT_TOL)
    for name, r in zip(("vecQuestions", "words", "knowledgeBase"), ref["inputs"]):
        errs["grad_" + name] = (rel_err(out["grad_" + name], r.grad), GRAD_TOL)
    names = macx.params.reference_names(cfg, p)
    for f in params.fields:
        worst = 0.0
        for refname, idx in names[f]:
            rg = ref["params"][refname].grad
            got = out["grad_" + f] if idx is None else out["grad_" + f][idx]
            floor = 5e-2 if refname.endswith("linearLayerlogits/biases/bias") else 1e-6      # analytically zero: absolute
            worst = max(worst, rel_err(got.reshape(rg.shape), rg, floor=floor))
        errs["grad_" + f] = (worst, GRAD_TOL)
    return errs


@pytest.mark.parametrize("name", list(cb.CASES))
def test_cell_bits_match_the_parent(macx, dev, name):
    with open(os.path.join(GOLDEN, name + ".json")) as fh:
        want = json.load(fh)["tensors"]
    out, ctx = cb.run_case(macx, dev, name)
    assert sorted(out) == sorted(want), "the fixture lists other tensors: regenerate it only from the reference commit"
    got = {k: cb.digest(v) for k, v in out.items()}
    for k in want:
        assert got[k]["shape"] == want[k]["shape"], k
    bad = sorted(k for k in want if got[k]["sha256"] != want[k]["sha256"])
    print("\nCHAINBITS %s: %d tensors, %d differ from the recorded bits" % (name, len(want), len(bad)))
    if bad:
        errs = _oracle_errors(macx, ctx, out)
        lines = ["%s: max |value| %.6g (recorded %.6g); against the fp64 oracle %.3e (tolerance %.0e: %s)"
                 % (k, got[k]["max_abs"], want[k]["max_abs"], errs[k][0], errs[k][1], "within" if errs[k][0] < errs[k][1] else "OUTSIDE")
                 for k in bad]
        pytest.fail("%s: %d of %d tensors are not bit-identical to the reference commit:\n  %s" % (name, len(bad), len(want), "\n  ".join(lines)))
