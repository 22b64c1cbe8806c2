"""CPU: macx.RecurrentQuestionEncoder as a class -- variables (names, order, shapes, initial values) per cell and direction count,
what it raises, how MACNet builds it, a checkpoint round trip by reference name -- and the contract of its two library calls:
every argument against the prototypes of macx_rnn_encoder_forward_w / _backward_w, position by position, with
tests/test_unit_contract_host.py's recorder in the library's place.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rnn_ref
from oracle import mac_oracle as mo
from test_tower_graph_host import small_net
from test_unit_contract_host import ENC_BWD, ENC_FWD, N_SAVED, N_WS, SEED, STREAM, Recorder, check_call, fresh_pointers, home, put, struct

PAIRS = [(cell, bi) for cell in ("RNN", "GRU", "LSTM") for bi in (False, True)]


def cfg_of(cell, bi, enc=256, E=20, ansEmbMod=None, **over):
    cfg = mo.flag_file_config("args", encType=cell, encBi=bi, encDim=enc, ctrlDim=enc, memDim=enc, attDim=enc, wrdEmbDim=E, **over)
    if ansEmbMod is not None:
        cfg.ansEmbMod = ansEmbMod                     # (a flag the modules read with a default of their own)
    return cfg


def reference_names(cell, bi):
    """the variables ops.RNNLayer creates, in TF's order (tests/golden/rnn_cells/*.npz holds the same lists, recorded)"""
    scope = {"RNN": "basic_rnn_cell", "GRU": "gru_cell", "LSTM": "basic_lstm_cell"}[cell]
    parts = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias") if cell == "GRU" else ("kernel", "bias")
    dirs = ("birnnLayer/bidirectional_rnn/fw/", "birnnLayer/bidirectional_rnn/bw/") if bi else ("rnnLayer/rnn/",)
    return ["encoder/%s%s/%s" % (d, scope, p) for d in dirs for p in parts]


@pytest.mark.parametrize("cell,bi", PAIRS)
def test_variables(macx, cell, bi):
    E, V, enc_dim = 20, 11, 256
    h = enc_dim // 2 if bi else enc_dim
    enc = macx.RecurrentQuestionEncoder(cfg_of(cell, bi), vocab=V, generator=torch.Generator().manual_seed(1))
    assert type(enc) is macx.RecurrentQuestionEncoder and enc.vocab == V and (enc.h, enc.dirs) == (h, 2 if bi else 1)
    d = enc.to_reference_dict()
    names = reference_names(cell, bi)
    assert list(d) == ["qEmbeddings/emb"] + names and len(enc.tensors()) == len(d)
    assert all(t is getattr(enc, f) for t, f in zip(enc.tensors(), enc.FIELDS))
    golden = np.load("%s/golden/rnn_cells/%s_%s.npz" % (__file__.rsplit("/", 1)[0], cell.lower(), "bi" if bi else "uni"))
    assert [str(n) for n in golden["names"]] == names                               # ... as the reference run recorded them
    width = {"RNN": 1, "LSTM": 4}
    assert tuple(d["qEmbeddings/emb"].shape) == (V, E)
    for n in names:
        k = width.get(cell) or (2 if "/gates/" in n else 1)
        if n.endswith("kernel"):
            assert tuple(d[n].shape) == (E + h, k * h), n
            lim = math.sqrt(6.0 / (E + h + k * h))                                   # glorot-uniform over the whole matrix
            assert float(d[n].abs().max()) <= lim and float(d[n].abs().max()) > 0.9 * lim and abs(float(d[n].mean())) < 0.05 * lim, n
        else:
            assert tuple(d[n].shape) == (k * h,), n
            assert bool((d[n] == (1.0 if n.endswith("gates/bias") else 0.0)).all()), n
    # the same seed draws the same values; another seed others; load_reference_dict copies bits
    a = macx.RecurrentQuestionEncoder(cfg_of(cell, bi), vocab=V, generator=torch.Generator().manual_seed(1))
    b = macx.RecurrentQuestionEncoder(cfg_of(cell, bi), vocab=V, generator=torch.Generator().manual_seed(2))
    assert all(torch.equal(x, y) for x, y in zip(enc.tensors(), a.tensors()))
    assert not torch.equal(enc.tensors()[1], b.tensors()[1])
    b.load_reference_dict(d)
    assert all(torch.equal(x, y) for x, y in zip(enc.tensors(), b.tensors()))
    # the struct of a call: this cell's pointers by name, NULL for the rest
    ps = enc.PARAMS(*range(1, len(enc.FIELDS) + 1))
    assert type(ps) is macx._lib.MacxRnnParams and type(enc.GRADS(*range(1, len(enc.FIELDS) + 1))) is macx._lib.MacxRnnGrads
    assert {f: getattr(ps, f) for f, _ in ps._fields_ if getattr(ps, f)} == {f: i + 1 for i, f in enumerate(enc.FIELDS)}
    assert set(enc.FIELDS) <= set(macx._lib.RNN_FIELDS)
    assert ("fw_candidate_kernel" in enc.FIELDS) == (cell == "GRU") and ("bw_kernel" in enc.FIELDS) == bi


def test_embedding_options(macx):
    init = torch.arange(11 * 20, dtype=torch.float32).reshape(11, 20)
    enc = macx.RecurrentQuestionEncoder(cfg_of("GRU", False, wrdEmbFixed=True), vocab=11, embInit=init)
    assert torch.equal(enc.emb, init) and not enc.emb.requires_grad and enc.fw_kernel.requires_grad
    with pytest.raises(ValueError, match=r"embInit must be \[11, 20\]"):
        macx.RecurrentQuestionEncoder(cfg_of("GRU", False), vocab=11, embInit=init[:5])
    assert (enc.keep_in, enc.keep_q) == (0.85, 0.92)


def test_raises_what_the_reference_raises(macx):
    R = macx.RecurrentQuestionEncoder
    for cell in ("MiGRU", "MiLSTM"):                  # createCell's activation = None, called by mi_gru_cell.py:57 / mi_lstm_cell.py:68
        with pytest.raises(TypeError) as e:
            R(cfg_of(cell, True), vocab=11)
        assert str(e.value) == "'NoneType' object is not callable"
    for cell, bi in PAIRS:
        with pytest.raises(KeyError) as e:           # model.py:286 reads a dropout model.py:80-90 never creates
            R(cfg_of(cell, bi, encVariationalDropout=True), vocab=11)
        assert e.value.args == ("stateInput",)
        with pytest.raises(ValueError) as e:
            R(cfg_of(cell, bi, encNumLayers=2), vocab=11)
        assert str(e.value) == ("Variable %s already exists, disallowed. Did you mean to set reuse=True in VarScope?"
                                % reference_names(cell, bi)[0])
    # for the LSTM that is GenericQuestionEncoder's text, word for word
    for bi in (False, True):
        with pytest.raises(ValueError) as g:
            macx.GenericQuestionEncoder(cfg_of("LSTM", bi, encNumLayers=2), vocab=11)
        with pytest.raises(ValueError) as e:
            R(cfg_of("LSTM", bi, encNumLayers=2), vocab=11)
        assert str(e.value) == str(g.value)
    # the reference's exceptions come before this class's own refusals
    with pytest.raises(KeyError):
        R(cfg_of("GRU", True, encVariationalDropout=True, encProj=True), vocab=11)


def test_unsupported_options_say_what_is_missing(macx):
    R = macx.RecurrentQuestionEncoder
    cases = ((cfg_of("GRU", True, encProj=True), "output projections"),
             (mo.flag_file_config("args", encType="RNN", encBi=False, encDim=256, ctrlDim=512), "output projections"),
             (cfg_of("GRU", False, ansEmbMod="SHARED"), "ansEmbMod SHARED"),
             (cfg_of("RNN", True, enc=128), "multiple of 128 units per direction"),
             (cfg_of("LSTM", False, enc=192), "multiple of 128 units per direction"),
             (cfg_of("GRU", False, enc=640), "up to 512 units"),
             (cfg_of("GRU", True, enc=1280), "up to 512 units"))
    for cfg, text in cases:
        with pytest.raises(macx.UnsupportedOptions, match=text):
            R(cfg, vocab=11)
    assert type(R(cfg_of("GRU", False, enc=512), vocab=11)) is R                    # the parser default's width
    assert type(R(cfg_of("LSTM", True, enc=1024), vocab=11)) is R


def test_constructor_dispatch_is_unchanged(macx):
    """macx.QuestionEncoder(config) returns the classes it returned, raises for GRU; the new class is opt-in"""
    assert type(macx.QuestionEncoder(cfg_of("LSTM", True), vocab=11)) is macx.QuestionEncoder
    assert type(macx.QuestionEncoder(cfg_of("LSTM", False), vocab=11)) is macx.GenericQuestionEncoder
    with pytest.raises(macx.UnsupportedOptions, match="encType=GRU has no HIP path"):
        macx.QuestionEncoder(cfg_of("GRU", True), vocab=11)
    assert not isinstance(macx.RecurrentQuestionEncoder(cfg_of("LSTM", True), vocab=11), macx.QuestionEncoder)


def test_macnet_builds_it_on_request(macx):
    gen = lambda: torch.Generator().manual_seed(0)
    before = small_net(macx)
    kw = dict(vocab=11, H=5, W=5, imageInDim=128, answerWordsNum=28)
    same = macx.MACNet(before.config, generator=gen(), encoder=None, **kw)
    assert type(same.enc) is macx.QuestionEncoder and len(same.tensors()) == len(before.tensors())
    assert all(torch.equal(a, b) for a, b in zip(before.tensors(), same.tensors()))
    assert type(small_net(macx, encBi=False).enc) is macx.GenericQuestionEncoder
    for cell, bi in PAIRS:
        cfg = small_net(macx, encType="LSTM").config
        cfg.encType, cfg.encBi = cell, bi
        net = macx.MACNet(cfg, generator=gen(), encoder="recurrent", **kw)
        assert type(net.enc) is macx.RecurrentQuestionEncoder and (net.enc.cell, net.enc.bi) == (cell, bi)
        assert net.tensors()[:len(net.enc.tensors())] == net.enc.tensors()
        # the rest of the tower draws what it drew: the encoder is built last
        n = len(before.enc.tensors())
        assert all(torch.equal(a, b) for a, b in zip(before.tensors()[n:], net.tensors()[len(net.enc.tensors()):]))
    mine = macx.RecurrentQuestionEncoder(cfg_of("GRU", True), vocab=11)
    assert macx.MACNet(before.config, generator=gen(), encoder=mine, **kw).enc is mine
    with pytest.raises(ValueError, match="encoder must be None"):
        macx.MACNet(before.config, generator=gen(), encoder="gru", **kw)
    with pytest.raises(TypeError):                                                  # what the reference raises, through MACNet too
        cfg = small_net(macx).config
        cfg.encType = "MiGRU"
        macx.MACNet(cfg, generator=gen(), encoder="recurrent", **kw)


def test_captured_tower_accepts_it_and_keeps_its_message(macx):
    graph = home(macx, "graph")        # (the package's own submodule: test_unit_contract_host.home)
    cfg = small_net(macx).config
    cfg.encType = "GRU"
    kw = dict(vocab=11, H=5, W=5, imageInDim=128, answerWordsNum=28, generator=torch.Generator().manual_seed(0))
    net = macx.MACNet(cfg, encoder="recurrent", **kw)
    with pytest.raises(RuntimeError) as e:               # past the module check: what is refused is the host device
        graph._require_fused_tower(net, "CapturedTowerForward")
    assert not isinstance(e.value, macx.UnsupportedOptions)
    with pytest.raises(macx.UnsupportedOptions) as e:
        graph._require_fused_tower(small_net(macx, encBi=False), "CapturedTowerForward")
    assert str(e.value) == ("CapturedTowerForward: net.enc is a GenericQuestionEncoder; only a tower of the fused modules "
                            "(QuestionEncoder, Stem, MACCellParams, OutputClassifier) is captured -- the generic one-kernel-per-op "
                            "modules are out of its scope")


@pytest.mark.parametrize("cell,bi", [("GRU", True), ("RNN", False), ("LSTM", False)])
def test_checkpoint_round_trip_by_reference_name(macx, tmp_path, cell, bi):
    cfg = small_net(macx).config
    cfg.encType, cfg.encBi = cell, bi
    kw = dict(vocab=11, H=5, W=5, imageInDim=128, answerWordsNum=28, encoder="recurrent")
    a = macx.MACNet(cfg, generator=torch.Generator().manual_seed(0), **kw)
    b = macx.MACNet(cfg, generator=torch.Generator().manual_seed(1), **kw)
    state = macx.checkpoint.reference_state_dict(a)
    for n in ["qEmbeddings/emb"] + reference_names(cell, bi):
        assert "macModel/" + n + ":0" in state, n
    assert list(state)[:len(a.enc.tensors())] == ["macModel/" + n + ":0" for n in a.enc.to_reference_dict()]
    assert not torch.equal(a.enc.fw_kernel, b.enc.fw_kernel)
    path = str(tmp_path / "net.npz")
    macx.checkpoint.save_npz(path, a)
    macx.checkpoint.load_npz(path, b)
    assert len(a.tensors()) == len(b.tensors()) and all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors()))
    c = macx.MACNet(cfg, generator=torch.Generator().manual_seed(2), **kw)
    assert macx.checkpoint.load_reference(c, state) == [] and all(torch.equal(x, y) for x, y in zip(a.tensors(), c.tensors()))


# ---------------------------------------------------------------------------------------------------------------------------
# the two library calls (test_unit_contract_host.py's recorder; nothing launches, the tensors live in host memory)
# ---------------------------------------------------------------------------------------------------------------------------
class RnnRecorder(Recorder):
    """the recorder, answering the sizing calls of a unit whose ABI name has two words (macx_rnn_encoder_*)"""

    def __getattr__(self, name):
        call = Recorder.__getattr__(self, name)

        def sized(*args):
            res = call(*args)
            return N_SAVED if name.endswith("_saved_floats") else N_WS if name.endswith("_ws_floats") else res
        return sized


@pytest.fixture
def rec(macx, monkeypatch):
    r = RnnRecorder()
    r.capturing = False
    monkeypatch.setattr(home(macx, "_lib"), "lib", lambda: r)
    monkeypatch.setattr(home(macx, "_lib"), "stream_of", lambda where: C.c_void_p(STREAM))
    monkeypatch.setattr(home(macx, "unit"), "require_device", lambda t, what: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: r.capturing)
    return r


def test_the_prototypes_are_the_encoders(macx):
    """macx_rnn_encoder_*_w take macx_encoder_*_w's arguments on the rnn structs: same arity, same classes, position by position"""
    T, L = macx._lib.TABLE, macx._lib
    for kind, (shapes, params, grads) in (("forward_w", (0, 4, None)), ("backward_w", (0, 4, 13))):
        old, new = T["macx_encoder_" + kind], T["macx_rnn_encoder_" + kind]
        assert old[0] is new[0] and len(old[1]) == len(new[1]) == len(ENC_FWD if kind == "forward_w" else ENC_BWD)
        swapped = {shapes: (L.MacxEncShapes, L.MacxRnnShapes), params: (L.MacxEncParams, L.MacxRnnParams), grads: (L.MacxEncGrads, L.MacxRnnGrads)}
        for i, (o, n) in enumerate(zip(old[1], new[1])):
            if i in swapped:
                assert (o._type_, n._type_) == swapped[i], (kind, i)
            else:
                assert o is n, (kind, i)
    for kind in ("saved_floats", "ws_floats"):
        assert T["macx_rnn_encoder_" + kind][0] is T["macx_encoder_" + kind][0]
        assert T["macx_rnn_encoder_" + kind][1][0]._type_ is L.MacxRnnShapes
    assert macx.RecurrentQuestionEncoder.EXPORTS == tuple("macx_rnn_encoder_" + k for k in ("saved_floats", "ws_floats", "forward_w", "backward_w"))
    assert all(n in macx._lib.EXPORTS for n in macx.RecurrentQuestionEncoder.EXPORTS) and len(macx._lib.EXPORTS) == 109
    assert L.RNN_CELL == {"RNN": 0, "GRU": 1, "LSTM": 2}
    assert [f for f, _ in L.MacxRnnShapes._fields_] == ["B", "S", "V", "E", "h", "b0", "cell", "dirs"]
    assert L.RNN_FIELDS[:5] == L.ENC_FIELDS


@pytest.mark.parametrize("cell,bi,train,capturing,fixed", [("GRU", True, True, False, False), ("RNN", False, False, True, True),
                                                           ("LSTM", False, True, False, False), ("GRU", False, True, False, True)])
def test_recurrent_encoder_calls(macx, rec, cell, bi, train, capturing, fixed):
    enc = macx.RecurrentQuestionEncoder(cfg_of(cell, bi, wrdEmbFixed=fixed), vocab=11, generator=torch.Generator().manual_seed(0))
    dirs, h = (2, 128) if bi else (1, 256)
    rec.capturing = capturing
    questions, lengths = torch.tensor([[1, 2, 3], [4, 11, 0]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    words, vecQ = enc(questions, lengths, train=train, seed=SEED, b0=3)
    fields = {f: 0 for f in macx._lib.RNN_FIELDS}
    fields.update({f: getattr(enc, f).data_ptr() for f in enc.FIELDS})
    env = dict(shapes=struct("MacxRnnShapes", B=2, S=3, V=11, E=20, h=h, b0=3, cell=macx._lib.RNN_CELL[cell], dirs=dirs),
               keep_input=0.85 if train else 1.0, keep_question=0.92 if train else 1.0, seed=0x89ABCDEF,
               params=struct("MacxRnnParams", **fields), questions=questions.data_ptr(), lengths=lengths.data_ptr(),
               words=words.data_ptr(), vecQuestions=vecQ.data_ptr(), saved=None, saved_floats=N_SAVED, mask_word=0, stream=STREAM,
               ws=None, ws_floats=N_WS, d_words=None, d_vecQuestions=None, grads=None)
    assert [n for n, _ in rec.calls] == ["macx_rnn_encoder_saved_floats", "macx_rnn_encoder_forward_w"]
    assert rec.calls[0][1] == (rec.calls[1][1][0],) and tuple(words.shape) == (2, 3, dirs * h) and tuple(vecQ.shape) == (2, dirs * h)
    check_call(macx, rec.calls[1], "macx_rnn_encoder_forward_w", ENC_FWD, env)
    env["saved"] = rec.calls[1][1][ENC_FWD.index("saved")]
    known = [questions.data_ptr(), lengths.data_ptr(), words.data_ptr(), vecQ.data_ptr()]
    fresh_pointers(rec.calls[1][1], ENC_FWD, ["saved"], known)
    assert (enc._capture_keep.data_ptr() == env["saved"]) if capturing else not hasattr(enc, "_capture_keep")
    del rec.calls[:]
    gw, gq = torch.randn(2, 3, dirs * h), torch.randn(2, dirs * h)
    env.update(d_words=gw.data_ptr(), d_vecQuestions=gq.data_ptr(), vecQuestions=None)
    seen = {}

    def on_call(name, args):
        if name.endswith("backward_w"):
            gs = args[ENC_BWD.index("grads")]
            seen["null"] = sorted(f for f, _ in gs._fields_ if not getattr(gs, f))
            for k, f in enumerate(enc.FIELDS):                 # k + 1 into the first float of the k-th gradient this cell has
                put(getattr(gs, f), float(k + 1))
    rec.on_call = on_call
    torch.autograd.backward([words, vecQ], [gw, gq])
    assert [n for n, _ in rec.calls] == ["macx_rnn_encoder_ws_floats", "macx_rnn_encoder_backward_w"]
    check_call(macx, rec.calls[1], "macx_rnn_encoder_backward_w", ENC_BWD, env)
    fresh_pointers(rec.calls[1][1], ENC_BWD, ["ws"], known + [gw.data_ptr(), gq.data_ptr(), env["saved"]])
    assert seen["null"] == sorted(set(macx._lib.RNN_FIELDS) - set(enc.FIELDS))       # the gradients this cell lacks stay NULL
    grads = [None if p.grad is None else float(p.grad.flatten()[0]) for p in enc.tensors()]
    assert grads == [None if fixed else 1.0] + [float(k + 1) for k in range(1, len(enc.FIELDS))]
    assert all(p.grad is None or p.grad.shape == p.shape for p in enc.tensors())


def test_mask_word_reaches_both_calls(macx, rec):
    enc = macx.RecurrentQuestionEncoder(cfg_of("GRU", False), vocab=11)
    word = torch.zeros(1, dtype=torch.int32)
    questions, lengths = torch.tensor([[1, 2, 3], [4, 11, 0]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    sh = enc.SHAPES(B=2, S=3, V=11, E=20, h=256, b0=0, cell=1, dirs=1)
    res = home(macx, "unit")._FusedCall.apply(enc, sh, (1.0, 1.0), 5, word, questions, lengths, *enc.tensors())
    torch.autograd.backward(list(res), [torch.ones_like(r) for r in res])
    assert [n for n, _ in rec.calls] == ["macx_rnn_encoder_" + s for s in ("saved_floats", "forward_w", "ws_floats", "backward_w")]
    for n, a in rec.calls[1::2]:
        assert len(a) == len(macx._lib.TABLE[n][1]) and a[-2:] == (word.data_ptr(), STREAM) and a[3] == 5, n


def test_reference_restatement_runs_on_the_class_variables(macx):
    """rnn_ref.question_encoder finds every variable of the class under the name the class gives it (no generator: a missing
    name would raise), which is what the GPU parity tests rely on"""
    for cell, bi in PAIRS:
        enc = macx.RecurrentQuestionEncoder(cfg_of(cell, bi), vocab=7, generator=torch.Generator().manual_seed(0))
        store = mo.VarStore(params={k: v.double() for k, v in enc.to_reference_dict().items()}, dtype=torch.float64)
        q = torch.tensor([[1, 7, 3], [2, 0, 0]])
        words, vec = rnn_ref.question_encoder(cfg_of(cell, bi), store, q, torch.tensor([3, 1]), 7)
        assert tuple(words.shape) == (2, 3, 256) and tuple(vec.shape) == (2, 256) and float(words[1, 1:].abs().max()) == 0.0
