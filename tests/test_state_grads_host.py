"""No GPU: the ABI of the state-gradient exports and the condition that keeps the GPU tests from passing vacuously.

1. macx_state_grads: field order and size in include/macx.h and in the ctypes mirror (_lib.MacxStateGrads) agree.
2. macx_cell_backward_x / macx_cell_backward_phase_x are declared in the header, listed in _lib.EXPORTS, and take the plain
   exports' arguments with the struct behind the input gradients.
3. For every single-output loss of tests/test_gpu_state_grads.py the fp64 oracle's gradients are non-zero at every input the loss
   must reach (tests/state_grads_ref.REACHED) and at some parameter: a comparison against them is a comparison of numbers far above
   helpers.rel_err's 1e-6 floor."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import mac_oracle as mo
import state_grads_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["d_controls", "d_memories", "d_att_question", "d_att_kb", "d_att_self", "d_att_gate"]


def _header():
    return open(os.path.join(ROOT, "include", "macx.h")).read()


def test_state_grads_struct_matches_the_header():
    import macx
    names = [f[0] for f in macx._lib.MacxStateGrads._fields_]
    assert names == FIELDS == list(macx._lib.STATE_GRAD_FIELDS)
    body = re.search(r"typedef struct macx_state_grads \{(.*?)\} macx_state_grads;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [part.strip() for part in body.split(";") if part.strip()]
    assert [re.search(r"(\w+)\s*$", d).group(1) for d in decls] == names
    assert all(d.startswith("const float*") for d in decls)                        # six device pointers, nothing else
    assert C.sizeof(macx._lib.MacxStateGrads) == len(names) * C.sizeof(C.c_void_p)
    sg = macx._lib.MacxStateGrads()
    assert all(getattr(sg, n) is None for n in names)                               # the default: all NULL == the plain call


def test_exports_are_declared_and_listed():
    import macx
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {}
    for name in ("macx_cell_backward", "macx_cell_backward_x", "macx_cell_backward_phase", "macx_cell_backward_phase_x"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, re.S)
        assert m, "%s is not declared in include/macx.h" % name
        protos[name] = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert name in macx._lib.EXPORTS
    for plain, ext in (("macx_cell_backward", "macx_cell_backward_x"), ("macx_cell_backward_phase", "macx_cell_backward_phase_x")):
        a, b = protos[plain], protos[ext]
        at = b.index("const macx_state_grads*")
        assert b[at - 1] == "const macx_input_grads*"
        assert b[:at] + b[at + 1:] == a, "%s is not %s + the struct" % (ext, plain)
    assert "FINITE" in _header()[_header().index("typedef struct macx_state_grads") - 1500: _header().index("typedef struct macx_state_grads")]


@pytest.mark.parametrize("kind,idx,name", sr.SINGLE_CASES)
def test_oracle_single_output_gradients_are_nonzero(kind, idx, name):
    sh, p = sr.SINGLE_SHAPE, sr.steps_of(name)
    B, S, N, d = sh["B"], sh["S"], sh["N"], sh["d"]
    cfg = mo.flag_file_config(name, netLength=p, memDim=d, ctrlDim=d, attDim=d)
    vq, words, lengths, kb = mo.synthetic_inputs(B, S, N, d, seed=1234)
    vs = mo.VarStore(generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    mo.mac_network(cfg, vs, vq.double(), words.double(), words.double(), lengths, kb.double())      # creates the variables
    Gs = sr.incoming([(kind, idx)], B, S, N, d, p)
    ref = sr.oracle_aux(cfg, vs.params, vq, words, lengths, kb, Gs, train=True, seed=5)
    t = sr.target_tensor(ref["cell"], None, kind, idx)
    assert t.requires_grad and tuple(t.shape) == sr.target_shape(kind, idx, B, S, N, d, p)
    largest = {}
    for n, x in zip(("vecQuestions", "words", "knowledgeBase"), ref["inputs"]):
        largest[n] = 0.0 if x.grad is None else float(x.grad.abs().max())
    for n in sr.REACHED[kind]:
        assert largest[n] > 1e-4, (n, largest)                                      # rel_err's floor is 1e-6
    assert max(float(v.grad.abs().max()) for v in ref["params"].values() if v.grad is not None) > 1e-4
