"""Question input unit (model.py:207-219 qEmbeddingsOp, model.py:279-307 encoder, ops.py:859-911 biRNNLayer):
embedding lookup -> dropout(encInputDropout) -> bidirectional BasicLSTMCell(encDim/2) with per-question lengths ->
questionCntxWords [B,S,encDim], vecQuestions = dropout(concat(final h_fw, h_bw), qDropout).  Producer of the cell's
`vecQuestions` / `questionCntxWords` inputs; SURVEY.md 8f row 4.  All compute behind libmacx.so
(macx_encoder_forward / macx_encoder_backward); no CPU path.

    enc = QuestionEncoder(config, vocab=90).to(device)
    questionCntxWords, vecQuestions = enc(questions, lengths, train=True, seed=step)

RecurrentQuestionEncoder is the same unit for encType RNN | GRU | LSTM in one direction or two (macx_rnn_encoder_*), opt-in.
"""
import torch

from . import _lib, generic, unit
from .generic import B_CHANNEL, B_ROW, B_SAME, OP_ADD, OP_MUL, GenericParams, _Act, _Binary, _Dropout, _Embed, _Linear, _Ops
from .options import UnsupportedOptions, fresh_seed

REF_NAMES = {"emb": "qEmbeddings/emb",
             "fw_kernel": "encoder/birnnLayer/bidirectional_rnn/fw/basic_lstm_cell/kernel",
             "fw_bias": "encoder/birnnLayer/bidirectional_rnn/fw/basic_lstm_cell/bias",
             "bw_kernel": "encoder/birnnLayer/bidirectional_rnn/bw/basic_lstm_cell/kernel",
             "bw_bias": "encoder/birnnLayer/bidirectional_rnn/bw/basic_lstm_cell/bias"}
FUSED_H_MAX = 512       # widest direction macx_encoder_* accept (h <= 512, include/macx.h)


def _check_fused(config):
    g = lambda n, dflt: getattr(config, n, dflt)
    if g("encType", "LSTM") != "LSTM" or not g("encBi", False) or g("encNumLayers", 1) != 1:
        raise UnsupportedOptions("encoder: only the bidirectional single-layer LSTM has a fused HIP path")
    if g("encVariationalDropout", False):
        raise UnsupportedOptions("encoder: encVariationalDropout has no HIP path")
    if g("encProj", False) or g("encDim", 512) != g("ctrlDim", 512):
        raise UnsupportedOptions("encoder: output projections (encProj / encDim != ctrlDim) have no fused HIP path")
    if g("ansEmbMod", "NON") == "SHARED":
        raise UnsupportedOptions("encoder: shared question/answer embeddings have no HIP path")
    if (int(g("encDim", 512)) // 2) % 128 or int(g("encDim", 512)) % 2:
        raise UnsupportedOptions("encoder: the fused kernels need 128 k units per direction (the generic path takes any multiple of 4)")
    if int(g("encDim", 512)) // 2 > FUSED_H_MAX:
        raise UnsupportedOptions("encoder: the fused backward step holds 16 questions' gate gradients in LDS, which fits up to %d units "
                                 "per direction (macx_enc_shapes, include/macx.h); wider encoders run on the generic path" % FUSED_H_MAX)


def check_questions(questions, lengths, vocab, check_ids):
    """lengths is [batchSize]; check_ids: word ids and lengths lie in range (a host synchronisation; off in the bench loop)"""
    if lengths.shape != (questions.shape[0],):
        raise ValueError("questionLengths must be [batchSize]")
    if check_ids:
        if int(questions.max()) > vocab or int(questions.min()) < 0:
            raise IndexError("question word id outside [0, %d]" % vocab)
        # tf.reverse_sequence / dynamic_rnn reject lengths beyond the padded length (InvalidArgumentError)
        if int(lengths.max()) > questions.shape[1] or int(lengths.min()) < 0:
            raise ValueError("question length outside [0, %d]" % questions.shape[1])


RNN_CELLS = {"RNN": ("basic_rnn_cell", 1), "GRU": ("gru_cell", 2), "LSTM": ("basic_lstm_cell", 4)}   # scope, width of `kernel` / h


def _cell_matrices(cell, k):
    """(scope part, field prefix, width / h, bias initial value) of a cell's matrices in TF's creation order"""
    if cell == "GRU":
        return (("gates/", "", 2, 1.0), ("candidate/", "candidate_", 1, 0.0))
    return (("", "", k, 0.0),)


class _FusedRecurrentEncoder(unit.FusedUnit):
    """The body QuestionEncoder and RecurrentQuestionEncoder share: the embedding, a cell's matrices per direction under the
    reference's names, and the one pair of ABI calls around them.  A class built on it names its ABI and says, in _shapes, how its
    shapes struct is filled (MacxEncShapes has no cell / dirs fields)."""

    def _declare(self, config, vocab, embInit, generator, cell, bi):
        """emb, then per direction the cell's matrices: registered, and drawn from the generator, in that order (a bias draws
        nothing).  Returns the fields in ABI order and their reference names."""
        g = lambda n, dflt: getattr(config, n, dflt)
        self.cell, self.bi, self.dirs = cell, bi, 2 if bi else 1
        self.vocab, self.E, self.h = int(vocab), int(g("wrdEmbDim", 300)), int(g("encDim", 512)) // self.dirs
        self.keep_in, self.keep_q = float(g("encInputDropout", 0.85)), float(g("qDropout", 0.92))
        E, h = self.E, self.h
        if embInit is None:
            emb = torch.randn((self.vocab, E), generator=generator, dtype=torch.float64)
        else:
            emb = torch.as_tensor(embInit, dtype=torch.float64)
            if tuple(emb.shape) != (self.vocab, E):
                raise ValueError("embInit must be [%d, %d]" % (self.vocab, E))
        self.emb = torch.nn.Parameter(emb.float(), requires_grad=not g("wrdEmbFixed", False))
        scope, k = RNN_CELLS[cell]
        fields, names = ["emb"], {"emb": "qEmbeddings/emb"}
        for d in ("fw", "bw")[:self.dirs]:
            base = "encoder/%s/%s" % ("birnnLayer/bidirectional_rnn/" + d if bi else "rnnLayer/rnn", scope)
            # TF's creation order: the GRU's gates before its candidate; glorot_uniform over the whole [in + n, k n] matrix
            for part, prefix, width, bias in _cell_matrices(cell, k):
                kern = unit.xavier_uniform((E + h, width * h), E + h + width * h, generator)
                for f, t in (("%s_%skernel" % (d, prefix), kern), ("%s_%sbias" % (d, prefix), torch.full((width * h,), bias))):
                    self.register_parameter(f, torch.nn.Parameter(t))
                    fields.append(f)
                    names[f] = "%s/%s%s" % (base, part, f.rsplit("_", 1)[1])
        return tuple(fields), names

    def embed(self, questions):
        """embeddingsOp's `questionWords` (model.py:207-219, 783): the embedded question words [B,S,wrdEmbDim] WITHOUT the encoder's
        input dropout -- what the cell attends over when --controlContextual is off (mac_cell.py:570)."""
        B, S = questions.shape
        return generic._Embed.apply(questions, self.emb, self.E, 1.0, 0, 0).reshape(B, S, self.E)

    def forward(self, questions, lengths, train=False, seed=None, b0=0, check_ids=True, mask_word=None):
        """questions [B,S] int32 (0 = pad), lengths [B] int32 -> (questionCntxWords [B,S,dirs h], vecQuestions [B,dirs h]).
        mask_word: None, or the run's mask word (1-element int32 device tensor, as MACCell's): XORed into the keys of the input
        and the question dropout when the kernels run, so that one captured graph draws fresh masks per replay."""
        unit.require_device(questions, "the question encoder")
        questions = questions.to(torch.int32).contiguous()
        lengths = lengths.to(device=questions.device, dtype=torch.int32).contiguous()
        check_questions(questions, lengths, self.vocab, check_ids)
        B, S = questions.shape
        keeps = (self.keep_in, self.keep_q) if train else (1.0, 1.0)
        return self._call(self._shapes(B, S, int(b0)), keeps, seed, train, mask_word, questions, lengths)

    def _outputs(self, sh, inputs):
        dev = inputs[0].device
        words = torch.empty(sh.B, sh.S, self.dirs * sh.h, dtype=torch.float32, device=dev)
        vecQ = torch.empty(sh.B, self.dirs * sh.h, dtype=torch.float32, device=dev)
        return (words, vecQ), inputs

    def _backward(self, sh, X, d_outs):
        # an output nothing was computed from has no gradient: the kernels read zeros there
        shapes = ((sh.B, sh.S, self.dirs * sh.h), (sh.B, self.dirs * sh.h))
        d = tuple(torch.zeros(s, dtype=torch.float32, device=X[0].device) if g is None else g.contiguous() for s, g in zip(shapes, d_outs))
        return d, (), (None, None)

    def _param_grads(self, grads):
        return [grads[0] if self.emb.requires_grad else None] + grads[1:]


class QuestionEncoder(_FusedRecurrentEncoder):
    """Mirrors `MACnet.embeddingsOp` + `MACnet.encoder` for the configuration every flag file uses
    (encType LSTM, --encBi, encNumLayers 1, encDim == ctrlDim so no projections) on the fused kernels.  Constructing it for
    another LSTM configuration -- no --encBi (the parser's default), --encProj, encDim != ctrlDim -- returns a
    GenericQuestionEncoder: the same interface on one HIP kernel per reference op."""
    FIELDS, REF_NAMES, ABI = _lib.ENC_FIELDS, REF_NAMES, "encoder"
    SHAPES, PARAMS, GRADS = _lib.MacxEncShapes, _lib.MacxEncParams, _lib.MacxEncGrads
    check_fused = staticmethod(_check_fused)
    SIZE_ERROR = "encoder: encDim/2 must be a multiple of 128, at most %d" % FUSED_H_MAX

    def __init__(self, config, vocab, embInit=None, generator=None):
        super().__init__()
        _check_fused(config)
        self._declare(config, vocab, embInit, generator, "LSTM", True)

    def _shapes(self, B, S, b0):
        return self.SHAPES(B=B, S=S, V=self.vocab, E=self.E, h=self.h, b0=b0)


def _check_recurrent(config):
    """What RecurrentQuestionEncoder refuses, in the order the reference meets it: its own exceptions first (model.py:286, then
    the cell's first call, then the second layer's variables), then the option sets this class leaves to the other two."""
    g = lambda n, dflt: getattr(config, n, dflt)
    if g("encVariationalDropout", False):
        raise KeyError("stateInput")                  # model.py:286 reads a dropout that model.py:80-90 never creates
    enc_type, bi = g("encType", "LSTM"), bool(g("encBi", False))
    if enc_type in ("MiGRU", "MiLSTM"):
        # ops.createCell hands every cell activation = activations.get(None, None); mi_gru_cell.py:57 / mi_lstm_cell.py:68 call it
        raise TypeError("'NoneType' object is not callable")
    if enc_type not in RNN_CELLS:
        raise KeyError(enc_type)                      # ops.py:770 cells[cellType] (argparse admits the five above)
    if g("encNumLayers", 1) > 1:
        first = {"RNN": "kernel", "GRU": "gates/kernel", "LSTM": "kernel"}[enc_type]
        raise ValueError("Variable encoder/%s/%s%s/%s already exists, disallowed. Did you mean to set reuse=True in VarScope?"
                         % ("birnnLayer/bidirectional_rnn" if bi else "rnnLayer/rnn", "fw/" if bi else "", RNN_CELLS[enc_type][0], first))
    if g("encProj", False) or g("encDim", 512) != g("ctrlDim", 512):
        raise UnsupportedOptions("encoder: the output projections (encProj / encDim != ctrlDim) are missing from the recurrent "
                                 "encoder's fused path; the LSTM has them on GenericQuestionEncoder")
    if g("ansEmbMod", "NON") == "SHARED":
        raise UnsupportedOptions("encoder: embeddings shared with the answers (ansEmbMod SHARED) are missing from the recurrent "
                                 "encoder's fused path")
    enc = int(g("encDim", 512))
    if (bi and enc % 2) or (enc // 2 if bi else enc) % 128:
        raise UnsupportedOptions("encoder: the recurrent kernels need a multiple of 128 units per direction (encDim%s = %s); the "
                                 "LSTM runs other widths on GenericQuestionEncoder" % ("/2" if bi else "", "%g" % (enc / 2 if bi else enc)))
    if (enc // 2 if bi else enc) > FUSED_H_MAX:
        raise UnsupportedOptions("encoder: the recurrent kernels hold 16 questions' gate gradients in LDS, which fits up to %d units "
                                 "per direction (macx_rnn_shapes, include/macx.h)" % FUSED_H_MAX)


class RecurrentQuestionEncoder(_FusedRecurrentEncoder):
    """qEmbeddingsOp + encoder (model.py:207-219, 279-307 -> ops.RNNLayer, ops.py:798-952) for every cell ops.createCell builds
    with an activation -- encType RNN (BasicRNNCell), GRU (GRUCell), LSTM (BasicLSTMCell) -- in one direction (no --encBi:
    tf.nn.dynamic_rnn, h = encDim) or two (h = encDim/2), on fused kernels: macx_rnn_encoder_forward_w / _backward_w, one launch
    per time step and pass (the GRU two).  QuestionEncoder's interface; (LSTM, --encBi) returns QuestionEncoder's bits.
    Variables under the reference's names: encoder/rnnLayer/rnn/<cell>/... or encoder/birnnLayer/bidirectional_rnn/{fw,bw}/<cell>/...
    with <cell> = basic_rnn_cell/{kernel,bias} | gru_cell/{gates,candidate}/{kernel,bias} | basic_lstm_cell/{kernel,bias}; kernels
    glorot-uniform over the whole matrix, biases zero, the GRU gates' bias one (TF 1.x).
    Opt-in (MACNet(..., encoder="recurrent")): QuestionEncoder(config) builds what it built before.  MiGRU / MiLSTM,
    encVariationalDropout and encNumLayers > 1 raise what the reference raises; the output projections, shared answer
    embeddings and widths off the 128 granule are UnsupportedOptions."""
    ABI = "rnn_encoder"
    SHAPES = _lib.MacxRnnShapes
    check_fused = staticmethod(_check_recurrent)
    SIZE_ERROR = "encoder: the width per direction must be a multiple of 128, at most %d" % FUSED_H_MAX

    def __new__(cls, *args, **kw):
        return torch.nn.Module.__new__(cls)               # (no generic twin to fall back to: a refused option set raises)

    def __init__(self, config, vocab, embInit=None, generator=None):
        super().__init__()
        _check_recurrent(config)
        self.FIELDS, self.REF_NAMES = self._declare(config, vocab, embInit, generator, getattr(config, "encType", "LSTM"),
                                                    bool(getattr(config, "encBi", False)))

    def _struct(self, cls, ptrs):
        return cls(**dict(zip(self.FIELDS, ptrs)))        # (the pointers this cell does not have stay NULL)

    def PARAMS(self, *ptrs):
        return self._struct(_lib.MacxRnnParams, ptrs)

    def GRADS(self, *ptrs):
        return self._struct(_lib.MacxRnnGrads, ptrs)

    def _shapes(self, B, S, b0):
        return self.SHAPES(B=B, S=S, V=self.vocab, E=self.E, h=self.h, b0=b0, cell=_lib.RNN_CELL[self.cell], dirs=self.dirs)


class GenericQuestionEncoder(generic.ParamsUnit, torch.nn.Module):
    """qEmbeddingsOp + encoder (model.py:207-219, 279-307 -> ops.RNNLayer -> biRNNLayer / fwRNNLayer, ops.py:798-950) for the
    LSTM configurations the fused kernels refuse -- a forward-only LSTM(encDim) (no --encBi: the parser's default), the output
    projections projCW / projQ (--encProj or encDim != ctrlDim, model.py:785-787, with --encProjQAct) -- as ONE HIP KERNEL PER
    REFERENCE OP: macx_embed_lookup(+_bwd), macx_linear / macx_wgrad for [x, h] @ kernel + bias, macx_op_act / macx_op_binary
    for the gates and the sequence-length masking, macx_op_dropout for the question vector.  torch owns memory, the
    per-step slices / stack / concat, the reverse-sequence gather and the autograd tape.  Variables under the reference's
    names (encoder/rnnLayer/rnn/basic_lstm_cell/kernel, ... / birnnLayer/bidirectional_rnn/{fw,bw}/..., linearLayerprojCW, ...).
    --encNumLayers > 1 raises what the reference raises (its layers collide on one variable scope); other cell types,
    variational dropout and shared answer embeddings are refused.  Hidden width per direction: any multiple of 4 (the products
    zero-pad their operands to the kernels' 128-column granule, generic.k_matmul)."""

    def __init__(self, config, vocab, embInit=None, generator=None, device=None):
        super().__init__()
        dflt = dict(encType="LSTM", encBi=False, encNumLayers=1, encVariationalDropout=False, encProj=False, encProjQAct="NON",
                    encDim=512, ctrlDim=512, wrdEmbDim=300, encInputDropout=0.85, qDropout=0.92, wrdEmbFixed=False, ansEmbMod="NON")
        g = lambda n: getattr(config, n, dflt[n])
        if g("encType") != "LSTM":
            raise UnsupportedOptions("encoder: encType=%s has no HIP path" % g("encType"))
        if g("encVariationalDropout"):
            raise UnsupportedOptions("encoder: encVariationalDropout has no HIP path")
        if g("ansEmbMod") == "SHARED":
            raise UnsupportedOptions("encoder: shared question/answer embeddings have no HIP path")
        self.bi = bool(g("encBi"))
        self.scopes = ("birnnLayer", "bidirectional_rnn") if self.bi else ("rnnLayer", "rnn")
        if g("encNumLayers") > 1:
            # model.py:295-298 builds every layer from `questions` under one scope (ops.py:938-950 closes "rnnLayer<name>" before
            # the layer is built): the second layer asks tf.get_variable for the first one's kernel
            raise ValueError("Variable encoder/%s/%s/%sbasic_lstm_cell/kernel already exists, disallowed. Did you mean to set "
                             "reuse=True in VarScope?" % (self.scopes[0], self.scopes[1], "fw/" if self.bi else ""))
        self.config = config
        self.vocab, self.E = int(vocab), int(g("wrdEmbDim"))
        self.enc, self.ctrl = int(g("encDim")), int(g("ctrlDim"))
        self.hh = self.enc // 2 if self.bi else self.enc
        if self.hh % 4:
            raise UnsupportedOptions("encoder: the LSTM width per direction must be a multiple of 4 (got %d): 16-byte rows; widths "
                                     "off the product kernels' 128-column granule run zero-padded inside them" % self.hh)
        self.proj = g("encProj") or self.enc != self.ctrl
        self.proj_act = g("encProjQAct")
        self.keep_in, self.keep_q = float(g("encInputDropout")), float(g("qDropout"))
        self.fixed = bool(g("wrdEmbFixed"))
        self.params = GenericParams(device=device, generator=generator)
        self.ops = _Ops(config, self.params)
        self._declare(embInit)

    def _cells(self):
        return ("fw", "bw") if self.bi else ("",)

    def _declare(self, embInit):
        vs, ops = self.params, self.ops
        with vs.scope("qEmbeddings"):
            emb = vs.get("emb", (self.vocab, self.E), "normal")
        if embInit is not None:
            init = torch.as_tensor(embInit, dtype=torch.float32)
            if tuple(init.shape) != (self.vocab, self.E):
                raise ValueError("embInit must be [%d, %d]" % (self.vocab, self.E))
            with torch.no_grad():
                emb.copy_(init)
        emb.requires_grad_(not self.fixed)
        for _ in self._cell_vars():
            pass
        if self.proj:
            with vs.scope("encoder"):
                with vs.scope("linearLayerprojCW"):
                    ops.getWeight((self.enc, self.ctrl)), ops.getBias((self.ctrl,))
                with vs.scope("linearLayerprojQ"):
                    ops.getWeight((self.enc, self.ctrl)), ops.getBias((self.ctrl,))
                    if self.proj_act != "NON":
                        if self.proj_act == "RELU" and getattr(self.config, "relu", "STD") == "PRM":
                            with vs.scope("prelu", default=True):
                                vs.get("alpha", (self.ctrl,), 0.25)
                        with vs.scope("linearLayerprojQ_2"):
                            ops.getWeight((self.ctrl, self.ctrl)), ops.getBias((self.ctrl,))

    def _cell_vars(self):
        """(direction, kernel [E + hh, 4 hh], bias [4 hh]) per cell, created on first use under the reference's names."""
        vs = self.params
        with vs.scope("encoder"), vs.scope(self.scopes[0]), vs.scope(self.scopes[1]):
            for d in self._cells():
                if d:
                    with vs.scope(d), vs.scope("basic_lstm_cell"):
                        yield d, vs.get("kernel", (self.E + self.hh, 4 * self.hh), "xavier"), vs.get("bias", (4 * self.hh,), "zeros")
                else:
                    with vs.scope("basic_lstm_cell"):
                        yield d, vs.get("kernel", (self.E + self.hh, 4 * self.hh), "xavier"), vs.get("bias", (4 * self.hh,), "zeros")

    def embed(self, questions):
        """embeddingsOp's `questionWords` (model.py:207-219, 783): the embedded question words [B,S,wrdEmbDim] without the input
        dropout -- what the cell attends over when --controlContextual is off (mac_cell.py:570)."""
        B, S = questions.shape
        with self.params.scope("qEmbeddings"):
            emb = self.params.get("emb", (self.vocab, self.E), "normal")
        return _Embed.apply(questions, emb, self.E, 1.0, 0, 0).reshape(B, S, self.E)

    def forward(self, questions, lengths, train=False, seed=None, b0=0, check_ids=True, mask_word=None):
        """questions [B,S] int (0 = pad), lengths [B] -> (questionCntxWords [B,S,w], vecQuestions [B,w]), w = ctrlDim when projected."""
        unit.refuse_mask_word(mask_word, "encoder", "macx_encoder_forward_w")
        generic._require_device(questions, "questions")                 # no CPU path
        dev = questions.device
        B, S = questions.shape
        lengths = lengths.to(device=dev)
        check_questions(questions, lengths, self.vocab, check_ids)
        keep_in, keep_q = (self.keep_in, self.keep_q) if train else (1.0, 1.0)
        seed = fresh_seed(seed, train)
        E, hh = self.E, self.hh
        Ep = (E + 127) // 128 * 128
        vs = self.params
        with vs.scope("qEmbeddings"):
            emb = vs.get("emb", (self.vocab, E), "normal")
        x = _Embed.apply(questions, emb, Ep, keep_in, seed, int(b0) * S).reshape(B, S, Ep)          # zero columns [E, Ep)
        t_idx = torch.arange(S, device=dev).unsqueeze(0)                                            # host-side index bookkeeping
        L_ = lengths.long().unsqueeze(1)
        live = (t_idx < L_).to(torch.float32)                                                       # [B,S]
        rev = torch.where(t_idx < L_, L_ - 1 - t_idx, t_idx)                                        # array_ops.reverse_sequence
        ones = torch.ones(hh, dtype=torch.float32, device=dev)                                      # BasicLSTMCell forget_bias
        sig, tanh = _lib.ACT["SIGMOID"], _lib.ACT["TANH"]
        mul = lambda a, b: _Binary.apply(a.contiguous(), b.contiguous(), OP_MUL, B_SAME, 1.0)
        rowmul = lambda a, r: _Binary.apply(a.contiguous(), r.contiguous(), OP_MUL, B_ROW, 1.0)
        outs, finals = [], []
        for d, kernel, bias in self._cell_vars():
            # the kernel with zero rows under the padded embedding columns (memory op; the gradient of the padding is dropped)
            Kp = torch.cat([kernel[:E], kernel.new_zeros(Ep - E, 4 * hh), kernel[E:]], dim=0) if Ep != E else kernel
            xin = torch.gather(x, 1, rev.unsqueeze(-1).expand(B, S, Ep)) if d == "bw" else x
            h = torch.zeros(B, hh, dtype=torch.float32, device=dev)
            c = torch.zeros(B, hh, dtype=torch.float32, device=dev)
            seq = []
            for t in range(S):
                z = _Linear.apply(torch.cat([xin[:, t], h], dim=1), Kp, bias)                       # [x, h] @ kernel + bias
                i, j, f, o = [z[:, k * hh:(k + 1) * hh].contiguous() for k in range(4)]
                f1 = _Binary.apply(f, ones, OP_ADD, B_CHANNEL, 1.0)
                cn = _Binary.apply(mul(c, _Act.apply(f1, sig, None)), mul(_Act.apply(i, sig, None), _Act.apply(j, tanh, None)),
                                   OP_ADD, B_SAME, 1.0)
                hn = mul(_Act.apply(cn, tanh, None), _Act.apply(o, sig, None))
                lv, dead = live[:, t], 1.0 - live[:, t]                                             # dynamic_rnn: copy the state through
                h = _Binary.apply(rowmul(hn, lv), rowmul(h, dead), OP_ADD, B_SAME, 1.0)
                c = _Binary.apply(rowmul(cn, lv), rowmul(c, dead), OP_ADD, B_SAME, 1.0)
                seq.append(rowmul(hn, lv))                                                          # ... and emit zeros
            out = torch.stack(seq, dim=1)
            if d == "bw":
                out = torch.gather(out, 1, rev.unsqueeze(-1).expand(B, S, hh))
            outs.append(out)
            finals.append(h)
        words = torch.cat(outs, dim=-1) if len(outs) > 1 else outs[0]
        vecQ = torch.cat(finals, dim=-1) if len(finals) > 1 else finals[0]
        if keep_q < 1.0:
            vecQ = _Dropout.apply(vecQ.contiguous(), seed, 12, 0, keep_q, int(b0) * vecQ.shape[1])   # SITE_QUESTION
        if self.proj:
            with vs.scope("encoder"):
                words = self.ops.linear(words.contiguous(), self.enc, self.ctrl, name="projCW")
                vecQ = self.ops.linear(vecQ, self.enc, self.ctrl, act=self.proj_act, name="projQ")
        return words, vecQ


QuestionEncoder.GENERIC = GenericQuestionEncoder
