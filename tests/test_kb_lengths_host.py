"""No GPU: the reference the kb_lengths GPU tests compare against, and the ABI field.

1. tests/kb_lengths_ref.masked_kb_attention is right: at fp64, for every question b of a padded batch, the masked oracle gives
   what the UNPATCHED oracle gives on that question alone with its knowledge base cut to its live cells, kb[b:b+1, :L_b] -- final
   memory and control and every step's attention over the knowledge base to 1e-12, and the parameter gradients of the batch are
   the sum of the single-question runs' (1e-11 of each gradient's largest entry: the two sides add the same fp64 terms in
   different orders).  The padded rows hold large finite junk, so a leak would show.
2. macx_inputs ends with kbLengths, in the header and in the ctypes mirror."""
import os
import re

import pytest
import torch

from oracle import mac_oracle as mo
from helpers import oracle_run, rel_err, max_abs
from kb_lengths_ref import masked_kb_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, N, d, p = 3, 6, 12, 16, 3
LENGTHS = [12, 1, 7]


def _case(name):
    cfg = mo.flag_file_config(name, netLength=p, memDim=d, ctrlDim=d, attDim=d)
    vq, words, lengths, kb = mo.synthetic_inputs(B, S, N, d, seed=21)
    kb = kb.double()
    g = torch.Generator().manual_seed(4)
    for b, L in enumerate(LENGTHS):
        kb[b, L:] = 50.0 * torch.randn(N - L, d, generator=g, dtype=torch.float64)       # padding: finite junk
    vs = mo.VarStore(generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    mo.mac_network(cfg, vs, vq.double(), words.double(), words.double(), lengths, kb)       # creates the variables
    params = {k: v.detach().clone() for k, v in vs.params.items()}
    g = torch.Generator().manual_seed(9)
    for k, v in params.items():
        if "bias" in k:                                                                       # non-zero biases: bias paths count
            v.copy_((torch.rand(v.shape, generator=g, dtype=torch.float64) - 0.5) * 0.2)
    dmem = torch.randn(B, d, generator=g, dtype=torch.float64)
    dctl = torch.randn(B, d, generator=g, dtype=torch.float64)
    return cfg, params, vq.double(), words.double(), lengths, kb, dmem, dctl


@pytest.mark.parametrize("name", ["args", "args3"])
def test_masked_oracle_is_the_oracle_on_the_cut_knowledge_base(name):
    cfg, params, vq, words, lengths, kb, dmem, dctl = _case(name)
    orig = mo.Ops.inter2att
    with masked_kb_attention(torch.tensor(LENGTHS), N):
        assert mo.Ops.inter2att is not orig
        full = oracle_run(cfg, params, vq, words, lengths, kb, train=False, need_grad=True, d_memory=dmem, d_control=dctl)
    assert mo.Ops.inter2att is orig                                                           # restored
    summed = {k: torch.zeros_like(v) for k, v in params.items()}
    for b, L in enumerate(LENGTHS):
        sl = slice(b, b + 1)
        one = oracle_run(cfg, params, vq[sl], words[sl], lengths[sl], kb[sl, :L], train=False, need_grad=True,
                         d_memory=dmem[sl], d_control=dctl[sl])
        assert max_abs(full["memory"][sl], one["memory"]) < 1e-12
        assert max_abs(full["control"][sl], one["control"]) < 1e-12
        for i in range(p):
            att = full["cell"].attentions["kb"][i][b]
            assert max_abs(att[:L], one["cell"].attentions["kb"][i][0]) < 1e-12
            assert bool((att[L:] == 0).all())
        assert bool((full["inputs"][2].grad[b, L:] == 0).all())                               # padded rows get no gradient
        assert rel_err(full["inputs"][2].grad[b, :L], one["inputs"][2].grad[0]) < 1e-11
        for k in summed:
            if one["params"][k].grad is not None:
                summed[k] += one["params"][k].grad
    for k, v in summed.items():
        got = full["params"][k].grad
        if got is None:
            assert float(v.abs().max()) == 0.0, k
            continue
        assert rel_err(got, v, floor=1e-3) < 1e-11, k


def test_masked_oracle_restores_on_error():
    orig = mo.Ops.inter2att
    with pytest.raises(RuntimeError):
        with masked_kb_attention([1], 4):
            raise RuntimeError("boom")
    assert mo.Ops.inter2att is orig


def test_inputs_struct_ends_with_kb_lengths():
    import macx
    names = [f[0] for f in macx._lib.MacxInputs._fields_]
    assert names == ["vecQuestions", "words", "questionLengths", "knowledgeBase", "kbLengths"]
    header = open(os.path.join(ROOT, "include", "macx.h")).read()
    body = re.search(r"typedef struct macx_inputs \{(.*?)\} macx_inputs;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in body.split(";") if part.strip()]
    assert fields == names
    assert "const int32_t* kbLengths" in body
    assert macx._lib.MacxInputs().kbLengths is None                                           # the default: NULL, every cell live
