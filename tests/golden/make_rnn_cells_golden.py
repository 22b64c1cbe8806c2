"""Writes tests/golden/rnn_cells/<cell>_<uni|bi>.npz: the reference's own ops.RNNLayer (ops.py:940-952), unmodified, on TF 1.x's
BasicRNNCell, GRUCell and BasicLSTMCell in one direction and two.  Run by hand where the upstream project is checked out:

    MACX_REFERENCE_DIR=<upstream checkout> python tests/golden/make_rnn_cells_golden.py

The TF shim (tests/tf1_shim) carries the LSTM only; tests/rnn_ref.install_into_shim adds the other two cells and a dynamic_rnn
with a tensor state to the LOADED shim at run time -- neither the shim nor tests/ref_exec.py is edited.  Each file holds the
inputs, the variables (names in creation order), the outputs and the gradients of fixed cotangents: data only.
B = 3, S = 4, E = 5, encDim 8; lengths 4, 1, 2."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ref_exec  # noqa: E402
import rnn_ref  # noqa: E402

OUT = os.path.join(HERE, "rnn_cells")
B, S, E, ENC = 3, 4, 5, 8
LENGTHS = (4, 1, 2)


def main():
    if not ref_exec.available():
        raise SystemExit("MACX_REFERENCE_DIR must name a checkout of the upstream project")
    M = ref_exec.load()
    tf, ops = M["tf"], M["ops"]
    rnn_ref.install_into_shim(tf)
    cfg = ref_exec.parse_flags("args.txt")
    os.makedirs(OUT, exist_ok=True)
    g = torch.Generator().manual_seed(1234)
    x0 = torch.randn(B, S, E, generator=g, dtype=torch.float64)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32)
    for cell in ("RNN", "GRU", "LSTM"):
        for bi in (False, True):
            cfg.encType, cfg.encBi, cfg.encDim = cell, bi, ENC
            tf.shim_reset(dtype=torch.float64, seed=7, require_grad=True)
            x = tf.wrap(x0.clone()).requires_grad_(True)
            with tf.variable_scope("encoder"):
                out_seq, last = ops.RNNLayer(x, tf.wrap(lengths.clone()), cfg.encDim, bi=cfg.encBi, cellType=cfg.encType, dropout=1.0,
                                             varDp=None, name="rnn0")
            names = list(tf.state.variables)
            d_out = torch.randn(tuple(out_seq.shape), generator=g, dtype=torch.float64)
            d_last = torch.randn(tuple(last.shape), generator=g, dtype=torch.float64)
            leaves = [x] + [tf.state.variables[n] for n in names]
            grads = torch.autograd.grad((out_seq * d_out).sum() + (last * d_last).sum(), leaves)
            rec = {"x": x0.numpy(), "lengths": lengths.numpy(), "names": np.array(names), "out_seq": out_seq.detach().numpy(),
                   "last_state": last.detach().numpy(), "d_out_seq": d_out.numpy(), "d_last_state": d_last.numpy(),
                   "grad_x": grads[0].numpy()}
            for i, (n, gr) in enumerate(zip(names, grads[1:])):
                rec["var_%d" % i] = tf.state.variables[n].detach().numpy()
                rec["grad_%d" % i] = gr.numpy()
            path = os.path.join(OUT, "%s_%s.npz" % (cell.lower(), "bi" if bi else "uni"))
            np.savez(path, **rec)
            print(path, names)


if __name__ == "__main__":
    main()
