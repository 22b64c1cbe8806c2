"""The contract of the three units around the cell (unit.FusedUnit / unit._FusedCall and their generic twins): the reference-name
dictionaries and checkpoint loading of all six modules, the exact sequence of library calls of the fused ones -- every argument
against the prototypes of include/macx.h, with a recorder in the library's place -- and the mask-word refusal.  No GPU."""
import ctypes as C
import importlib
import types

import pytest
import torch

import abi_kit
from test_tower_graph_host import small_net

GENERIC = dict(enc=dict(encBi=False), stem=dict(stemKernelSize=1), out=dict(outClassifierDims=[128, 128]))
SEED = (7 << 32) | 0x89ABCDEF            # (the library sees the low 32 bits)
STREAM = 0x5EED


def home(macx, name):
    """the package's own submodule (a `from macx.<name> import ...` anywhere in the session binds a second copy to macx.<name>)"""
    return importlib.import_module(macx.__name__ + "." + name)


def unit_of(macx, which, generic, seed=None):
    """the unit `which` of small_net (generator seed 0), or one built on its own for the same options from `seed`"""
    net = small_net(macx, **(GENERIC[which] if generic else {}))
    if seed is None:
        return getattr(net, which)
    gen = torch.Generator().manual_seed(seed)
    if which == "enc":
        return macx.QuestionEncoder(net.config, 11, generator=gen)
    if which == "stem":
        return macx.Stem(net.config, H=5, W=5, inDim=128, generator=gen)
    return macx.OutputClassifier(net.config, answerWordsNum=28, generator=gen)


def same_tensors(a, b):
    """two units hold the same tensors bit for bit"""
    ta, tb = a.tensors(), b.tensors()
    return len(ta) == len(tb) and all(abi_kit.bits_equal(x, y) for x, y in zip(ta, tb))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. names, order, loading
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("which", ["enc", "stem", "out"])
def test_reference_dict_contract(macx, which, generic):
    a, b = unit_of(macx, which, generic), unit_of(macx, which, generic, seed=1)
    assert type(a) is type(b) and type(a).__name__.startswith("Generic") == generic
    names = list(a.to_reference_dict())
    assert len(names) == len(a.tensors()) == len(set(names))
    if not generic:
        lib = home(macx, "_lib")
        mod, fields = {"enc": (home(macx, "encoder"), lib.ENC_FIELDS), "stem": (home(macx, "stem"), lib.STEM_FIELDS),
                       "out": (home(macx, "output"), lib.OUT_FIELDS)}[which]
        assert type(a).FIELDS is fields and type(a).REF_NAMES is mod.REF_NAMES
        assert names == [mod.REF_NAMES[f] for f in fields]
        assert all(t is getattr(a, f) for t, f in zip(a.tensors(), fields))
    # the dictionary follows tensors() order: number the tensors and read the numbers back in dictionary order
    c = unit_of(macx, which, generic, seed=2)
    with torch.no_grad():
        for i, t in enumerate(c.tensors()):
            t.fill_(float(i))
    assert list(c.to_reference_dict()) == names
    assert [float(v.flatten()[0]) for v in c.to_reference_dict().values()] == [float(i) for i in range(len(names))]
    # load_reference_dict: b takes a's bits
    assert not same_tensors(a, b)
    b.load_reference_dict(a.to_reference_dict())
    assert same_tensors(a, b)
    # ... and so does checkpoint.load_reference on a single component
    d = unit_of(macx, which, generic, seed=3)
    state = macx.checkpoint.reference_state_dict(a)
    assert list(state) == ["macModel/" + n + ":0" for n in names]
    assert macx.checkpoint.load_reference(d, state) == [] and same_tensors(a, d)
    # a wrong shape is a ValueError, a missing name a KeyError under strict (and reported, nothing else touched, without)
    first = next(iter(state))
    with pytest.raises(ValueError, match="shape mismatch"):
        macx.checkpoint.load_reference(d, dict(state, **{first: torch.zeros(3, 1, 2)}))
    short = {k: v for k, v in state.items() if k != first}
    with pytest.raises(KeyError, match="missing variables"):
        macx.checkpoint.load_reference(d, short)
    e = unit_of(macx, which, generic, seed=4)
    before = e.tensors()[0].detach().clone()
    assert macx.checkpoint.load_reference(e, short, strict=False) == [names[0]]
    assert torch.equal(e.tensors()[0], before) and all(torch.equal(x, y) for x, y in zip(a.tensors()[1:], e.tensors()[1:]))


@pytest.mark.parametrize("over", [{}] + list(GENERIC.values()), ids=["fused", "enc", "stem", "out"])
def test_checkpoint_restores_a_whole_net(macx, over):
    a = small_net(macx, **over)
    b = macx.MACNet(a.config, vocab=11, H=5, W=5, imageInDim=128, answerWordsNum=28, generator=torch.Generator().manual_seed(1))
    assert [type(getattr(a, m)) for m in ("enc", "stem", "out")] == [type(getattr(b, m)) for m in ("enc", "stem", "out")]
    assert not same_tensors(a, b)
    assert macx.checkpoint.load_reference(b, macx.checkpoint.reference_state_dict(a)) == []
    assert same_tensors(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the library calls of the fused units.  Four things are swapped: _lib.lib (the recorder), _lib.stream_of, unit.require_device
#    and torch.cuda.is_current_stream_capturing.  Nothing launches: the tensors live in host memory, so the recorder may also write
#    through the pointers it receives, which is how the tensors the node allocates in its backward pass are identified.
# ---------------------------------------------------------------------------------------------------------------------------
N_SAVED, N_WS = 24, 40


class Recorder:
    def __init__(self):
        self.calls, self.on_call = [], None

    def __getattr__(self, name):
        def call(*args):
            args = tuple((a.value or 0) if isinstance(a, C.c_void_p) else getattr(a, "_obj", a) for a in args)     # byref(s)._obj is s
            self.calls.append((name, args))
            if self.on_call is not None:
                self.on_call(name, args)
            return {"saved_floats": N_SAVED, "ws_floats": N_WS}.get(name.split("_", 2)[2], 0)
        return call


@pytest.fixture
def rec(macx, monkeypatch):
    r = Recorder()
    r.capturing = False
    monkeypatch.setattr(home(macx, "_lib"), "lib", lambda: r)
    monkeypatch.setattr(home(macx, "_lib"), "stream_of", lambda where: C.c_void_p(STREAM))
    monkeypatch.setattr(home(macx, "unit"), "require_device", lambda t, what: None)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: r.capturing)
    return r


def floats_at(address, n=1):
    return list((C.c_float * n).from_address(address))


def put(address, value):
    C.c_float.from_address(address).value = value


def check_call(macx, call, name, want, env):
    """one recorded call against its prototype: `want` names the header's parameters in order, env gives each name's value"""
    got_name, args = call
    assert got_name == name
    assert len(args) == len(macx._lib.TABLE[name][1]) == len(want), name
    for i, (w, a) in enumerate(zip(want, args)):
        v = env[w]
        if isinstance(v, dict):              # a struct, field by field
            assert type(a).__name__ == v["type"], (name, i, w)
            assert {f: getattr(a, f) or 0 for f, _ in a._fields_} == v["fields"], (name, i, w)
        elif v is not None:                  # (None: checked by the caller, through the memory behind the pointer)
            assert type(a) is type(v) and a == v, (name, i, w, a, v)


def struct(type_name, **fields):
    return {"type": type_name, "fields": fields}


def params_struct(type_name, mod):
    return struct(type_name, **{f: getattr(mod, f).data_ptr() for f in mod.FIELDS})


def mark_gradients(args, want, extra=()):
    """write k + 1 into the first float of the k-th field of the grads struct, 101, 102, ... behind the pointers named in extra"""
    gs = args[want.index("grads")]
    for k, (f, _) in enumerate(gs._fields_):
        put(getattr(gs, f), float(k + 1))
    for k, w in enumerate(extra):
        put(args[want.index(w)], float(101 + k))


def fresh_pointers(args, want, names, known):
    """the buffers a call allocated itself: non-NULL, distinct from each other and from every tensor the test knows"""
    ptrs = [args[want.index(n)] for n in names]
    assert all(ptrs) and len(set(ptrs) | set(known)) == len(ptrs) + len(set(known))


STEM_FWD = ["shapes", "act", "keep", "seed", "params", "images", "kb", "saved", "saved_floats", "mask_word", "stream"]
STEM_BWD = ["shapes", "act", "keep", "seed", "params", "kb", "saved", "saved_floats", "ws", "ws_floats", "d_kb", "grads", "mask_word",
            "stream"]


@pytest.mark.parametrize("train, capturing", [(True, False), (False, True)])
def test_stem_calls(macx, rec, train, capturing):
    stem = small_net(macx).stem
    rec.capturing = capturing
    images = torch.randn(2, 25, 128)
    kb = stem(images, train=train, seed=SEED, b0=3)
    env = dict(shapes=struct("MacxStemShapes", B=2, H=5, W=5, Cin=128, Cmid=512, Cout=256, b0=3), act=macx._lib.ACT["ELU"],
               keep=0.82 if train else 1.0, seed=0x89ABCDEF, params=params_struct("MacxStemParams", stem), images=images.data_ptr(),
               kb=kb.data_ptr(), saved=None, saved_floats=N_SAVED, mask_word=0, stream=STREAM, ws=None, ws_floats=N_WS, d_kb=None,
               grads=None)
    assert [n for n, _ in rec.calls] == ["macx_stem_saved_floats", "macx_stem_forward_w"]
    assert rec.calls[0][1] == (rec.calls[1][1][0],) and tuple(kb.shape) == (2, 25, 256) and kb.dtype == torch.float32
    check_call(macx, rec.calls[1], "macx_stem_forward_w", STEM_FWD, env)
    env["saved"] = rec.calls[1][1][STEM_FWD.index("saved")]
    fresh_pointers(rec.calls[1][1], STEM_FWD, ["saved"], [images.data_ptr(), kb.data_ptr()])
    if capturing:
        assert stem._capture_keep.data_ptr() == env["saved"] and stem._capture_keep.shape == (N_SAVED,)
        assert stem._capture_keep.dtype == torch.float32
    else:
        assert not hasattr(stem, "_capture_keep")
    del rec.calls[:]
    g = torch.randn(2, 25, 256)
    env["d_kb"] = g.data_ptr()
    rec.on_call = lambda name, args: name.endswith("backward_w") and mark_gradients(args, STEM_BWD)
    kb.backward(g)
    assert [n for n, _ in rec.calls] == ["macx_stem_ws_floats", "macx_stem_backward_w"]
    check_call(macx, rec.calls[1], "macx_stem_backward_w", STEM_BWD, env)
    fresh_pointers(rec.calls[1][1], STEM_BWD, ["ws"], [images.data_ptr(), kb.data_ptr(), g.data_ptr(), env["saved"]])
    assert [float(p.grad.flatten()[0]) for p in stem.tensors()] == [1.0, 2.0, 3.0, 4.0]
    assert all(p.grad.shape == p.shape for p in stem.tensors()) and images.grad is None


OUT_FWD = ["shapes", "act", "keep", "seed", "params", "memory", "vecQuestions", "logits", "saved", "saved_floats", "mask_word", "stream"]
OUT_BWD = ["shapes", "act", "keep", "seed", "params", "memory", "vecQuestions", "saved", "saved_floats", "ws", "ws_floats", "d_logits",
           "grads", "d_memory", "d_vecQuestions", "mask_word", "stream"]


@pytest.mark.parametrize("train, capturing", [(True, False), (False, True)])
def test_output_calls(macx, rec, train, capturing):
    out = small_net(macx).out
    rec.capturing = capturing
    memory, vecQ = torch.randn(2, 256, requires_grad=True), torch.randn(2, 256, requires_grad=True)
    logits = out(memory, vecQ, train=train, seed=SEED, b0=3)
    env = dict(shapes=struct("MacxOutShapes", B=2, d=256, hidden=128, answers=28, b0=3), act=macx._lib.ACT["ELU"],
               keep=0.85 if train else 1.0, seed=0x89ABCDEF, params=params_struct("MacxOutParams", out), memory=memory.data_ptr(),
               vecQuestions=vecQ.data_ptr(), logits=logits.data_ptr(), saved=None, saved_floats=N_SAVED, mask_word=0, stream=STREAM,
               ws=None, ws_floats=N_WS, d_logits=None, grads=None, d_memory=None, d_vecQuestions=None)
    assert [n for n, _ in rec.calls] == ["macx_output_saved_floats", "macx_output_forward_w"]
    assert rec.calls[0][1] == (rec.calls[1][1][0],) and tuple(logits.shape) == (2, 28) and logits.dtype == torch.float32
    check_call(macx, rec.calls[1], "macx_output_forward_w", OUT_FWD, env)
    env["saved"] = rec.calls[1][1][OUT_FWD.index("saved")]
    known = [memory.data_ptr(), vecQ.data_ptr(), logits.data_ptr()]
    fresh_pointers(rec.calls[1][1], OUT_FWD, ["saved"], known)
    assert (out._capture_keep.data_ptr() == env["saved"]) if capturing else not hasattr(out, "_capture_keep")
    del rec.calls[:]
    g = torch.randn(2, 28)
    env["d_logits"] = g.data_ptr()
    rec.on_call = lambda name, args: name.endswith("backward_w") and mark_gradients(args, OUT_BWD, ("d_memory", "d_vecQuestions"))
    logits.backward(g)
    assert [n for n, _ in rec.calls] == ["macx_output_ws_floats", "macx_output_backward_w"]
    check_call(macx, rec.calls[1], "macx_output_backward_w", OUT_BWD, env)
    fresh_pointers(rec.calls[1][1], OUT_BWD, ["ws", "d_memory", "d_vecQuestions"], known + [g.data_ptr(), env["saved"]])
    assert [float(p.grad.flatten()[0]) for p in out.tensors()] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert float(memory.grad.flatten()[0]) == 101.0 and float(vecQ.grad.flatten()[0]) == 102.0
    assert memory.grad.shape == memory.shape and vecQ.grad.shape == vecQ.shape


ENC_FWD = ["shapes", "keep_input", "keep_question", "seed", "params", "questions", "lengths", "words", "vecQuestions", "saved",
           "saved_floats", "mask_word", "stream"]
ENC_BWD = ["shapes", "keep_input", "keep_question", "seed", "params", "questions", "lengths", "saved", "saved_floats", "ws", "ws_floats",
           "d_words", "d_vecQuestions", "grads", "mask_word", "stream"]


def enc_env(macx, enc, questions, lengths, train):
    return dict(shapes=struct("MacxEncShapes", B=2, S=3, V=11, E=20, h=128, b0=3), keep_input=0.85 if train else 1.0,
                keep_question=0.92 if train else 1.0, seed=0x89ABCDEF, params=params_struct("MacxEncParams", enc),
                questions=questions.data_ptr(), lengths=lengths.data_ptr(), words=None, vecQuestions=None, saved=None,
                saved_floats=N_SAVED, mask_word=0, stream=STREAM, ws=None, ws_floats=N_WS, d_words=None, d_vecQuestions=None, grads=None)


@pytest.mark.parametrize("train, capturing, fixed", [(True, False, False), (False, True, True)])
def test_encoder_calls(macx, rec, train, capturing, fixed):
    enc = small_net(macx, wrdEmbFixed=fixed).enc
    assert enc.emb.requires_grad != fixed
    rec.capturing = capturing
    questions, lengths = torch.tensor([[1, 2, 3], [4, 11, 0]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    words, vecQ = enc(questions, lengths, train=train, seed=SEED, b0=3)
    env = enc_env(macx, enc, questions, lengths, train)
    env.update(words=words.data_ptr(), vecQuestions=vecQ.data_ptr())
    assert [n for n, _ in rec.calls] == ["macx_encoder_saved_floats", "macx_encoder_forward_w"]
    assert rec.calls[0][1] == (rec.calls[1][1][0],) and tuple(words.shape) == (2, 3, 256) and tuple(vecQ.shape) == (2, 256)
    check_call(macx, rec.calls[1], "macx_encoder_forward_w", ENC_FWD, env)
    env["saved"] = rec.calls[1][1][ENC_FWD.index("saved")]
    known = [questions.data_ptr(), lengths.data_ptr(), words.data_ptr(), vecQ.data_ptr()]
    fresh_pointers(rec.calls[1][1], ENC_FWD, ["saved"], known)
    assert (enc._capture_keep.data_ptr() == env["saved"]) if capturing else not hasattr(enc, "_capture_keep")
    del rec.calls[:]
    gw, gq = torch.randn(2, 3, 256), torch.randn(2, 256)
    env.update(d_words=gw.data_ptr(), d_vecQuestions=gq.data_ptr(), vecQuestions=None)
    rec.on_call = lambda name, args: name.endswith("backward_w") and mark_gradients(args, ENC_BWD)
    torch.autograd.backward([words, vecQ], [gw, gq])
    assert [n for n, _ in rec.calls] == ["macx_encoder_ws_floats", "macx_encoder_backward_w"]
    check_call(macx, rec.calls[1], "macx_encoder_backward_w", ENC_BWD, env)
    fresh_pointers(rec.calls[1][1], ENC_BWD, ["ws"], known + [gw.data_ptr(), gq.data_ptr(), env["saved"]])
    grads = [None if p.grad is None else float(p.grad.flatten()[0]) for p in enc.tensors()]
    assert grads == [None if fixed else 1.0, 2.0, 3.0, 4.0, 5.0]           # a fixed embedding gets no gradient


def test_encoder_backward_without_an_outputs_gradient(macx, rec):
    """the node itself, outside the autograd engine (which would materialise the zeros): a None gradient becomes a zero tensor"""
    for fixed, missing in ((False, 0), (True, 1)):
        enc = small_net(macx, wrdEmbFixed=fixed).enc
        questions, lengths = torch.tensor([[1, 2, 3], [4, 11, 0]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
        sh = enc.SHAPES(B=2, S=3, V=11, E=20, h=128, b0=3)
        args = (enc, sh, (1.0, 1.0), SEED, None, questions, lengths) + tuple(enc.tensors())
        ctx = types.SimpleNamespace(needs_input_grad=(False,) * 7 + (True,) * 5)
        home(macx, "unit")._FusedCall.forward(ctx, *args)
        given = [torch.randn(2, 3, 256), torch.randn(2, 256)]
        name, n = ("d_words", "d_vecQuestions")[missing], given[missing].numel()
        given[missing] = None
        seen = {}

        def on_call(fn, a):
            if fn.endswith("backward_w"):
                seen["zeros"] = floats_at(a[ENC_BWD.index(name)], n)
                seen["other"] = a[ENC_BWD.index(("d_words", "d_vecQuestions")[1 - missing])]
        rec.on_call = on_call
        res = home(macx, "unit")._FusedCall.backward(ctx, *given)
        assert seen["zeros"] == [0.0] * len(seen["zeros"]) and seen["other"] == given[1 - missing].data_ptr()
        # one entry per argument of forward: no gradient for the seven in front, the parameters' behind them
        assert len(res) == len(args) and res[:7] == (None,) * 7
        assert [r is None for r in res[7:]] == [fixed, False, False, False, False]
        assert all(r.shape == p.shape for r, p in zip(res[8:], enc.tensors()[1:]))
        del rec.calls[:]


def test_mask_word_reaches_both_calls(macx, rec):
    """forward() takes a device word only, so the node is applied directly: the word's address sits in front of the stream"""
    net = small_net(macx)
    word = torch.zeros(1, dtype=torch.int32)
    images = torch.randn(2, 25, 128)
    questions, lengths = torch.tensor([[1, 2, 3], [4, 11, 0]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    memory, vecQ = torch.randn(2, 256), torch.randn(2, 256)
    cases = ((net.stem, net.stem.SHAPES(B=2, H=5, W=5, Cin=128, Cmid=512, Cout=256, b0=0), (4, 1.0), (images,)),
             (net.enc, net.enc.SHAPES(B=2, S=3, V=11, E=20, h=128, b0=0), (1.0, 1.0), (questions, lengths)),
             (net.out, net.out.SHAPES(B=2, d=256, hidden=128, answers=28, b0=0), (4, 1.0), (memory, vecQ)))
    for mod, sh, scalars, inputs in cases:
        del rec.calls[:]
        res = home(macx, "unit")._FusedCall.apply(mod, sh, scalars, 5, word, *inputs, *mod.tensors())
        res = res if isinstance(res, tuple) else (res,)
        torch.autograd.backward(list(res), [torch.ones_like(r) for r in res])
        names = [n for n, _ in rec.calls]
        assert names == ["macx_%s_%s" % (mod.ABI, s) for s in ("saved_floats", "forward_w", "ws_floats", "backward_w")]
        for n, a in rec.calls[1::2]:
            assert len(a) == len(macx._lib.TABLE[n][1]) and a[-2:] == (word.data_ptr(), STREAM) and a[3] == 5, n


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the generic modules refuse a mask word before they ask for the device
# ---------------------------------------------------------------------------------------------------------------------------
def test_generic_modules_refuse_a_mask_word_before_the_device_check(macx):
    word = torch.zeros(1, dtype=torch.int32)
    calls = {
        "enc": (lambda m, **kw: m(torch.zeros(2, 3, dtype=torch.int32), torch.ones(2, dtype=torch.int32), **kw),
                "encoder: a run's mask word is taken by the fused encoder only (macx_encoder_forward_w); the generic encoder has no "
                "such path"),
        "stem": (lambda m, **kw: m(torch.zeros(2, 25, 128), **kw),
                 "stem: a run's mask word is taken by the fused stem only (macx_stem_forward_w); the generic stem has no such path"),
        "out": (lambda m, **kw: m(torch.zeros(2, 256), torch.zeros(2, 256), **kw),
                "output unit: a run's mask word is taken by the fused output unit only (macx_output_forward_w); the generic "
                "classifier has no such path")}
    for which, (call, text) in calls.items():
        mod = unit_of(macx, which, True)
        with pytest.raises(RuntimeError, match="must live on the HIP device"):       # host tensors: the device check ...
            call(mod)
        with pytest.raises(macx.UnsupportedOptions) as e:                            # ... which the refusal comes before
            call(mod, mask_word=word)
        assert str(e.value) == text
    for what in ("the stem", "the question encoder", "the output unit"):
        with pytest.raises(RuntimeError) as e:
            home(macx, "unit").require_device(torch.zeros(1), what)
        assert str(e.value) == what + " has no CPU path"
