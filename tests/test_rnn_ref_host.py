"""CPU: tests/rnn_ref.py (the encoder on TF 1.x's BasicRNNCell, GRUCell and BasicLSTMCell, fp64) against its two references --
the oracle's question_encoder where both exist (the LSTM, one direction and two, eval and train with injected masks), and the
reference's own ops.RNNLayer run on these cells (tests/golden/rnn_cells/*.npz, written by tests/golden/make_rnn_cells_golden.py):
outputs, final state, every gradient to 1e-12, and the variable names in creation order."""
import os

import numpy as np
import pytest
import torch

import rnn_ref
from oracle import mac_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnn_cells")
TOL = 1e-12
PAIRS = [(cell, bi) for cell in ("RNN", "GRU", "LSTM") for bi in (False, True)]


def close(a, b):
    return float((torch.as_tensor(a) - torch.as_tensor(b)).abs().max()) <= TOL


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("bi", [False, True])
def test_lstm_agrees_with_the_oracle(bi, train):
    B, S, V, E, enc = 4, 5, 9, 6, 8
    cfg = mo.flag_file_config("args", encType="LSTM", encBi=bi, encDim=enc, ctrlDim=enc, wrdEmbDim=E)
    g = torch.Generator().manual_seed(2)
    lengths = torch.tensor([S, 1, 3, 0], dtype=torch.int32)                       # full, one word, ragged, empty
    q = torch.randint(1, V + 1, (B, S), generator=g) * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1))
    keeps = (0.8, 0.9) if train else (1.0, 1.0)
    masks = [(torch.rand(B, S, E, generator=g) < keeps[0]).double(), (torch.rand(B, enc, generator=g) < keeps[1]).double()] if train else None
    d_words, d_vec = torch.randn(B, S, enc, generator=g, dtype=torch.float64), torch.randn(B, enc, generator=g, dtype=torch.float64)
    runs = []
    for fn in (mo.question_encoder, rnn_ref.question_encoder):
        store = mo.VarStore(generator=torch.Generator().manual_seed(5), dtype=torch.float64, requires_grad=True)
        if runs:                                                                    # the second run on the first one's variables
            store = mo.VarStore(params={k: v.detach().clone().requires_grad_(True) for k, v in runs[0][2].params.items()},
                                dtype=torch.float64)
        words, vec = fn(cfg, store, q, lengths, V, keep_input=keeps[0], keep_question=keeps[1], masks=masks)
        if not runs:                                                                # zero biases test nothing: move them, run again
            with torch.no_grad():
                for k, v in store.params.items():
                    if k.endswith("bias"):
                        v.copy_(torch.rand(v.shape, generator=g, dtype=torch.float64) - 0.5)
            words, vec = fn(cfg, store, q, lengths, V, keep_input=keeps[0], keep_question=keeps[1], masks=masks)
        ((words * d_words).sum() + (vec * d_vec).sum()).backward()
        runs.append((words, vec, store))
    (w0, v0, s0), (w1, v1, s1) = runs
    assert list(s0.params) == list(s1.params) and len(s0.params) == (5 if bi else 3)
    assert close(w0, w1) and close(v0, v1)
    for k in s0.params:
        assert close(s0.params[k].grad, s1.params[k].grad), k


@pytest.mark.parametrize("cell,bi", PAIRS)
def test_agrees_with_the_recorded_reference_run(cell, bi):
    with np.load(os.path.join(GOLDEN, "%s_%s.npz" % (cell.lower(), "bi" if bi else "uni"))) as z:
        rec = {k: z[k] for k in z.files}
    names = [str(n) for n in rec["names"]]
    x = torch.from_numpy(rec["x"]).requires_grad_(True)
    B, S, E = x.shape
    assert (B, S, E) == (3, 4, 5) and rec["lengths"].tolist() == [4, 1, 2] and x.dtype == torch.float64
    cfg = mo.flag_file_config("args", encType=cell, encBi=bi, encDim=8, ctrlDim=8, wrdEmbDim=E)
    # an empty store with a generator: the restatement creates its variables itself, so their names and ORDER are its own
    store = mo.VarStore(generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    with store.scope("encoder"):
        rnn_ref.rnn_layer(cfg, store, x.detach(), rec["lengths"])
    assert list(store.params) == names
    n_dir, per_dir = (2 if bi else 1), (4 if cell == "GRU" else 2)
    assert len(names) == n_dir * per_dir
    prm = {n: torch.from_numpy(rec["var_%d" % i]).requires_grad_(True) for i, n in enumerate(names)}
    for n, v in prm.items():
        assert v.shape == store.params[n].shape, n
        if n.endswith("gates/bias"):
            assert bool((v == 1).all())                                             # GRUCell's gate bias starts at one
        elif n.endswith("bias"):
            assert bool((v == 0).all())
    store = mo.VarStore(params=prm, dtype=torch.float64)
    with store.scope("encoder"):
        out_seq, last = rnn_ref.rnn_layer(cfg, store, x, rec["lengths"])
    assert close(out_seq, rec["out_seq"]) and close(last, rec["last_state"])
    h = 8 // n_dir
    assert float(out_seq[1, 1:].abs().max()) == 0.0 and float(out_seq[2, 2:].abs().max()) == 0.0     # zero past a question's end
    assert close(last[0, :h], out_seq[0, 3, :h]) and close(last[1, :h], out_seq[1, 0, :h])             # the final forward state
    ((out_seq * torch.from_numpy(rec["d_out_seq"])).sum() + (last * torch.from_numpy(rec["d_last_state"])).sum()).backward()
    assert close(x.grad, rec["grad_x"])
    for i, n in enumerate(names):
        assert close(prm[n].grad, rec["grad_%d" % i]), n
