"""The question encoder with every cell ops.createCell builds with an activation (ops.py:749-772), restated in torch: TF 1.x's
BasicRNNCell, GRUCell and BasicLSTMCell (rnn_cell_impl.py) under tf.nn.dynamic_rnn / tf.nn.bidirectional_dynamic_rnn.  The oracle's
question_encoder (oracle/mac_oracle.py) covers the LSTM only; this one takes its arguments (a VarStore by name, masks injected)
and agrees with it there (tests/test_rnn_ref_host.py), and with the reference's own ops.RNNLayer run on these cells
(tests/golden/rnn_cells/, written by tests/golden/make_rnn_cells_golden.py).

    BasicRNNCell   h' = tanh([x, h] kernel + bias)                                   <scope>/basic_rnn_cell/{kernel,bias}
    GRUCell        r, u = split(sigmoid([x, h] gates/kernel + gates/bias))           <scope>/gru_cell/gates/{kernel,bias}   bias: ones
                   c = tanh([x, r h] candidate/kernel + candidate/bias)              <scope>/gru_cell/candidate/{kernel,bias}
                   h' = u h + (1 - u) c
    BasicLSTMCell  i, j, f, o = split([x, h] kernel + bias); c' = c sigmoid(f + 1) + sigmoid(i) tanh(j); h' = tanh(c') sigmoid(o)

The second half of the module is the same two TF cells and a dynamic_rnn with a tensor state written against the TF 1.x shim
(tests/tf1_shim), for make_rnn_cells_golden.py to install there at run time: the reference's RNNLayer then runs unmodified."""
import contextlib

import torch

CELL_SCOPE = {"RNN": "basic_rnn_cell", "GRU": "gru_cell", "LSTM": "basic_lstm_cell"}


def cell_variables(store, cell, n_in, h):
    """the cell's variables in TF's creation order, under the store's current scope: [(name below the scope, tensor)]"""
    out = []
    with store.scope(CELL_SCOPE[cell]):
        if cell == "GRU":
            for part, width, bias in (("gates", 2, "ones"), ("candidate", 1, "zeros")):
                with store.scope(part):
                    out.append((part + "/kernel", store.get("kernel", (n_in + h, width * h), "xavier")))
                    out.append((part + "/bias", store.get("bias", (width * h,), bias)))
        else:
            width = 4 if cell == "LSTM" else 1
            out.append(("kernel", store.get("kernel", (n_in + h, width * h), "xavier")))
            out.append(("bias", store.get("bias", (width * h,), "zeros")))
    return out


def cell_step(cell, variables, x, state):
    """one call of the cell: (output, new state); state is h, or (c, h) for the LSTM"""
    v = dict(variables)
    if cell == "RNN":
        hn = torch.tanh(torch.cat([x, state], dim=1) @ v["kernel"] + v["bias"])
        return hn, hn
    if cell == "GRU":
        r, u = torch.sigmoid(torch.cat([x, state], dim=1) @ v["gates/kernel"] + v["gates/bias"]).chunk(2, dim=1)
        c = torch.tanh(torch.cat([x, r * state], dim=1) @ v["candidate/kernel"] + v["candidate/bias"])
        hn = u * state + (1 - u) * c
        return hn, hn
    c, h = state
    i, j, f, o = (torch.cat([x, h], dim=1) @ v["kernel"] + v["bias"]).chunk(4, dim=1)
    cn = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    hn = torch.tanh(cn) * torch.sigmoid(o)
    return hn, (cn, hn)


def rnn_layer(config, store, x, lengths):
    """ops.RNNLayer (ops.py:940-952) -> fwRNNLayer / biRNNLayer without their input dropout, under the store's current scope
    (the reference's RNNLayer closes its own "rnnLayer<name>" scope before the layer is built): x [B,S,n_in], lengths [B] ->
    (outSeq [B,S,dirs h], lastState [B,dirs h]).  Past a question's end dynamic_rnn emits zeros and copies the state through; the
    backward direction runs over the length-reversed question and its outputs are reversed back."""
    B, S, n_in = x.shape
    bi, cell = bool(config.encBi), config.encType
    h = int(config.encDim / 2) if bi else config.encDim
    dt = x.dtype
    lengths = torch.as_tensor(lengths)
    outs, finals = [], []
    scopes = ("birnnLayer", "bidirectional_rnn") if bi else ("rnnLayer", "rnn")
    with store.scope(scopes[0]), store.scope(scopes[1]):
        for direction in (("fw", "bw") if bi else ("",)):
            with contextlib.ExitStack() as es:
                if direction:
                    es.enter_context(store.scope(direction))
                variables = cell_variables(store, cell, n_in, h)
            zeros = torch.zeros((B, h), dtype=dt)
            state = (zeros, zeros) if cell == "LSTM" else zeros
            out = torch.zeros((B, S, h), dtype=dt)
            rows = torch.arange(B)
            for tau in range(S):
                live = (tau < lengths).to(dt).unsqueeze(1)                                   # [B,1]
                pos = torch.full((B,), tau, dtype=torch.long) if direction != "bw" else (lengths.long() - 1 - tau).clamp(min=0)
                y, new = cell_step(cell, variables, x[rows, pos], state)
                if cell == "LSTM":
                    state = tuple(live * n + (1 - live) * s for n, s in zip(new, state))
                else:
                    state = live * new + (1 - live) * state
                put = torch.zeros((B, S, 1), dtype=dt)
                put[rows, pos] = live
                out = out + put * y.unsqueeze(1)
            outs.append(out)
            finals.append(state[1] if cell == "LSTM" else state)
    return torch.cat(outs, dim=-1), torch.cat(finals, dim=-1)


def question_encoder(config, store, questions, lengths, vocab, keep_input=1.0, keep_question=1.0, masks=None):
    """oracle.mac_oracle.question_encoder's arguments and results, for encType RNN | GRU | LSTM without output projections:
    qEmbeddingsOp (model.py:207-219) + encoder (model.py:279-297).  masks: [input mask [B,S,E], question mask [B,encDim]] when
    the keeps are < 1 (tf.nn.dropout: x * mask / keep)."""
    E, dt = config.wrdEmbDim, store.dtype
    with store.scope("qEmbeddings"):
        emb = store.get("emb", (vocab, E), "normal")
    x = torch.cat([torch.zeros((1, E), dtype=dt), emb], dim=0)[torch.as_tensor(questions).long()]
    if keep_input < 1.0:
        x = x * masks[0] / keep_input
    with store.scope("encoder"):
        words, vecQ = rnn_layer(config, store, x, lengths)
    if keep_question < 1.0:
        vecQ = vecQ * masks[1] / keep_question
    return words, vecQ


# ---------------------------------------------------------------------------------------------------------------------------
# the same cells against the TF 1.x shim (tests/golden/make_rnn_cells_golden.py installs them into the loaded shim)
# ---------------------------------------------------------------------------------------------------------------------------
def install_into_shim(tf):
    """tf.nn.rnn_cell.BasicRNNCell / GRUCell as rnn_cell_impl.py defines them, and a tf.nn.dynamic_rnn that carries a tensor state
    as well as an LSTMStateTuple (rnn._rnn_step: zero output and the state copied through past a sequence's end)."""
    base, state_tuple = tf.nn.rnn_cell.RNNCell, tf.nn.rnn_cell.LSTMStateTuple

    class _TensorStateCell(base):
        def __init__(self, num_units, activation=None, reuse=None, name=None):
            self._n, self._act, self._reuse, self._vars = int(num_units), activation or tf.tanh, reuse, None

        state_size = property(lambda self: self._n)
        output_size = property(lambda self: self._n)

        def zero_state(self, batch_size, dtype):
            return tf.zeros((int(batch_size), self._n))

        def __call__(self, inputs, st, scope=None):
            if self._vars is None:          # Layer.__call__: the variables are built once, in the scope of the first call
                with tf.variable_scope(scope or self.SCOPE, reuse=self._reuse):
                    self._vars = self.build(int(inputs.shape[-1]))
            out = self.call(inputs, st)
            return out, out

    class BasicRNNCell(_TensorStateCell):
        SCOPE = "basic_rnn_cell"

        def build(self, n_in):
            return (tf.get_variable("kernel", (n_in + self._n, self._n)), tf.get_variable("bias", (self._n,), tf.zeros_initializer()))

        def call(self, inputs, st):
            kernel, bias = self._vars
            return self._act(tf.matmul(tf.concat([inputs, st], 1), kernel) + bias)

    class GRUCell(_TensorStateCell):
        SCOPE = "gru_cell"

        def build(self, n_in):
            n = self._n
            with tf.variable_scope("gates"):        # "gates/kernel" etc. (rnn_cell_impl.GRUCell.build)
                gates = (tf.get_variable("kernel", (n_in + n, 2 * n)), tf.get_variable("bias", (2 * n,), tf.constant_initializer(1.0)))
            with tf.variable_scope("candidate"):
                cand = (tf.get_variable("kernel", (n_in + n, n)), tf.get_variable("bias", (n,), tf.zeros_initializer()))
            return gates + cand

        def call(self, inputs, st):
            gk, gb, ck, cb = self._vars
            value = tf.sigmoid(tf.matmul(tf.concat([inputs, st], 1), gk) + gb)
            r, u = tf.split(value, 2, axis=1)
            c = self._act(tf.matmul(tf.concat([inputs, r * st], 1), ck) + cb)
            return u * st + (1 - u) * c

    def dynamic_rnn(cell, inputs, sequence_length=None, initial_state=None, scope=None, **_ignored):
        if scope is None:
            with tf.variable_scope("rnn"):
                return dynamic_rnn(cell, inputs, sequence_length, initial_state, scope="rnn")
        B, T = inputs.shape[0], inputs.shape[1]
        st, outs = initial_state, []
        for t in range(T):
            out, new = cell(inputs[:, t], st)
            if sequence_length is not None:
                live = (t < torch.as_tensor(sequence_length).reshape(B, 1)).to(out.dtype)
                out = live * out
                if isinstance(st, state_tuple):
                    new = state_tuple(live * new[0] + (1 - live) * st[0], live * new[1] + (1 - live) * st[1])
                else:
                    new = live * new + (1 - live) * st
            st = new
            outs.append(out)
        return tf.wrap(torch.stack(outs, dim=1)), st

    def bidirectional_dynamic_rnn(cell_fw, cell_bw, inputs, sequence_length=None, initial_state_fw=None, initial_state_bw=None, **_ignored):
        with tf.variable_scope("bidirectional_rnn"):
            with tf.variable_scope("fw"):
                out_fw, st_fw = dynamic_rnn(cell_fw, inputs, sequence_length, initial_state_fw, scope="fw")
            rev = tf.reverse_sequence(inputs, sequence_length)
            with tf.variable_scope("bw"):
                tmp, st_bw = dynamic_rnn(cell_bw, rev, sequence_length, initial_state_bw, scope="bw")
            out_bw = tf.reverse_sequence(tmp, sequence_length)
        return (out_fw, out_bw), (st_fw, st_bw)

    tf.nn.rnn_cell.BasicRNNCell, tf.nn.rnn_cell.GRUCell = BasicRNNCell, GRUCell
    tf.nn.dynamic_rnn, tf.nn.bidirectional_dynamic_rnn = dynamic_rnn, bidirectional_dynamic_rnn
