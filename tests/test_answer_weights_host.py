"""The host side of per-question answer weights and partial batches (macx_answer_loss_weighted, `weights=` / `totals=` on
answer_loss_and_pred and MACNetCore.loss_and_pred, `weights=True` / `score=True` on the captured tower classes): the export, the
padding rule, the reference's own consistency, and every refusal -- each raised before anything asks for the device, on the
never-constructed instances tests/test_lengths_paths_host.py uses.  No GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import answer_weights_ref as ref
from test_lengths_paths_host import bare
from test_tower_graph_host import small_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, G, N = 6, 7, 3, 25
TOWER_CLASSES = ("CapturedTowerForward", "CapturedTowerTrainStep")


def test_export_is_declared_and_bound_with_matching_arguments(macx):
    name = "macx_answer_loss_weighted"
    header = open(os.path.join(ROOT, "include", "macx.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, code)
    assert m is not None, "not declared in macx.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* logits", "const int32_t* answers", "const float* weights", "int B", "int A", "float* loss_rows",
                      "int32_t* pred", "float* dlogits", "float* loss_out", "double* totals", "float grad_scale", "void* stream"]
    assert name in macx._lib.EXPORTS
    restype, argtypes = macx._lib.TABLE[name]
    v, i, f = C.c_void_p, C.c_int, C.c_float
    assert restype is C.c_int and list(argtypes) == [v, v, v, i, i, v, v, v, v, v, f, v]
    assert hasattr(macx._lib.lib(), name)
    # macx_answer_loss itself is what it was, and the ABI version did not move (a new export, no struct changed)
    assert list(macx._lib.TABLE["macx_answer_loss"][1]) == [v, v, i, i, v, v, v, f, v]
    assert macx._lib.ABI_VERSION == 5 and macx._lib.lib().macx_abi_version() == 5


def test_new_keywords_default_to_off(macx):
    for f in (macx.output.answer_loss_and_pred, macx.MACNetCore.loss_and_pred):
        sig = inspect.signature(f).parameters
        assert sig["weights"].default is None and sig["totals"].default is None, f
    sig = inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters
    assert sig["weights"].default is False and sig["totals"].default is None
    assert inspect.signature(macx.CapturedTowerForward.__init__).parameters["score"].default is False
    for name in TOWER_CLASSES:
        assert inspect.signature(getattr(macx, name).load).parameters["weights"].default is None, name
    for f in (macx.CapturedTowerForward.load, macx.CapturedTowerForward.__call__):
        assert inspect.signature(f).parameters["answers"].default is None, f
    # the cell-level classes are out of scope: their caller owns d_memory
    for name in ("CapturedForward", "CapturedTrainStep", "CapturedDPTrainStep"):
        assert "weights" not in inspect.signature(getattr(macx, name).__init__).parameters, name


# ---- the padding rule and the reference ------------------------------------------------------------------------------------------
def test_padding_rule_on_index_tensors():
    ids = torch.tensor([[3, 1, 0], [2, 2, 2], [5, 0, 0], [1, 4, 0]], dtype=torch.int32)
    out = ref.pad_slots(ids, 4, 6)
    assert out.dtype == torch.int32 and out.tolist() == ids.tolist() + [[3, 1, 0], [3, 1, 0]]
    assert ref.pad_slots(ids, 4, 4).tolist() == ids.tolist()                       # a full batch is itself
    assert ref.pad_slots(torch.tensor([7, 2]), 2, 5).tolist() == [7, 2, 7, 7, 7]
    assert ref.pad_slots(torch.tensor([9]), 1, 3).tolist() == [9, 9, 9]
    per_step = torch.arange(2 * 2 * 3).reshape(2, 2, 3)                            # a per-step target: the questions on axis 1
    assert ref.pad_slots(per_step, 2, 3, axis=1).tolist() == [[[0, 1, 2], [3, 4, 5], [0, 1, 2]], [[6, 7, 8], [9, 10, 11], [6, 7, 8]]]
    assert ref.pad_weights(None, 2, 4).tolist() == [1.0, 1.0, 0.0, 0.0]
    assert ref.pad_weights(torch.tensor([0.5, 2.0, 1.0]), 3, 4).tolist() == [0.5, 2.0, 1.0, 0.0]


def test_the_library_pads_by_the_same_rule(macx):
    g = torch.Generator().manual_seed(1)
    for shape, n, axis in (((6, 7), 4, 0), ((6,), 1, 0), ((6, 25, 8), 6, 0), ((3, 6, 25), 2, 1)):
        short = list(shape)
        short[axis] = n
        t = torch.randint(0, 9, short, generator=g, dtype=torch.int32)
        buf = torch.full(shape, -1, dtype=torch.int32)
        macx.graph._pad_slots(buf, t, n, axis=axis)
        assert torch.equal(buf, ref.pad_slots(t, n, shape[axis], axis=axis)), (shape, n, axis)


def test_reference_gradient_is_autograd_of_its_loss():
    Bq, A = 7, 5
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(Bq, A, generator=g)
    answers = torch.randint(0, A, (Bq,), generator=g)
    weights = torch.tensor([1.0, 0.5, 0.0, 2.0, -1.0, float("nan"), 0.25])
    dead = ~ref.live(weights, Bq)
    assert dead.tolist() == [False, False, True, False, True, True, False]
    logits[dead] = float("nan")
    answers[dead] = A + 7
    r = ref.reference(logits, answers, weights)
    assert bool(torch.isfinite(r["loss"])) and bool(torch.isfinite(r["dlogits"]).all())
    x = torch.where(dead.unsqueeze(1), torch.zeros(Bq, A), logits).to(torch.float64).requires_grad_(True)
    w = ref.effective(weights, Bq)
    rows = -torch.log_softmax(x, dim=1).gather(1, torch.where(dead, 0, answers).unsqueeze(1)).squeeze(1)
    loss = (w * rows).sum() / w.sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(r["loss"])) <= 1e-14
    assert float((x.grad - r["dlogits"]).abs().max()) <= 1e-15
    assert bool((r["dlogits"][dead] == 0).all()) and bool((r["rows"][dead] == 0).all()) and r["pred"][dead].tolist() == [-1, -1, -1]
    assert r["sums"][2] == 3.75
    # no live question: loss 0, gradient 0, no NaN
    z = ref.reference(logits, answers, torch.zeros(Bq))
    assert float(z["loss"]) == 0.0 and bool((z["dlogits"] == 0).all()) and z["sums"] == (0.0, 0.0, 0.0)


# ---- AnswerTotals ------------------------------------------------------------------------------------------------------------------
def test_answer_totals_read_arithmetic(macx):
    totals = macx.output.AnswerTotals("cpu")                    # (the holder is plain memory; the loss refuses one that is not on the device)
    assert totals.tensor.dtype == torch.float64 and totals.tensor.shape == (3,)
    assert totals.read() == dict(loss=0.0, accuracy=0.0, weight=0.0)              # W == 0: both ratios are 0, no division
    totals.tensor.copy_(torch.tensor([3.0, 1.5, 0.0], dtype=torch.float64))
    assert totals.read() == dict(loss=0.0, accuracy=0.0, weight=0.0)
    totals.tensor.copy_(torch.tensor([3.0, 1.5, 6.0], dtype=torch.float64))
    assert totals.read() == dict(loss=0.5, accuracy=0.25, weight=6.0)
    totals.reset()
    assert totals.tensor.tolist() == [0.0, 0.0, 0.0]


# ---- answer_loss_and_pred: the arguments, before the device -------------------------------------------------------------------------
def test_weights_dtype_shape_and_device_are_refused(macx):
    logits, answers = torch.zeros(B, 28), torch.zeros(B, dtype=torch.int32)
    for call in (macx.output.answer_loss_and_pred, macx.MACNetCore.loss_and_pred):
        for bad in (torch.ones(B, dtype=torch.float64), torch.ones(B, dtype=torch.int32), [1.0] * B):
            with pytest.raises(TypeError, match="weights"):
                call(logits, answers, weights=bad)
        for bad in (torch.ones(B - 1), torch.ones(B, 1), torch.ones(())):
            with pytest.raises(ValueError, match="weights"):
                call(logits, answers, weights=bad)
        with pytest.raises(RuntimeError, match="weights.*no CPU path"):
            call(logits, answers, weights=torch.ones(B))
        with pytest.raises(TypeError, match="totals"):
            call(logits, answers, totals=torch.zeros(3, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="totals.*no CPU path"):
            call(logits, answers, totals=macx.output.AnswerTotals("cpu"))
        with pytest.raises(RuntimeError, match="no CPU path"):               # both None: the call of before, which needs the device
            call(logits, answers)


# ---- the captured tower classes ---------------------------------------------------------------------------------------------------
def batch(n, g=None):
    """(images, questions, lengths, answers) of n questions (g shared images, or one image per question)"""
    return (torch.zeros(n if g is None else g, N, 128), torch.ones(n, S, dtype=torch.int32), torch.full((n,), S, dtype=torch.int32),
            torch.zeros(n, dtype=torch.int32))


def tower(macx, name, weights=True, **attrs):
    built = dict(weights=torch.ones(B)) if weights else {}
    if name == "CapturedTowerForward" and weights:
        built["answers"] = torch.zeros(B, dtype=torch.int32)
    return bare(macx, name, B=B, S=S, N=N, **dict(dict(G=None), **dict(built, **attrs)))


def load(obj, images, questions, lengths, answers, **kw):
    if type(obj).__name__ == "CapturedTowerTrainStep":
        return obj.load(images, questions, lengths, answers, check_ids=False, **kw)
    return obj.load(images, questions, lengths, check_ids=False, answers=answers if obj.answers is not None else None, **kw)


@pytest.mark.parametrize("name", TOWER_CLASSES)
def test_a_class_built_without_weights_refuses_a_short_batch_and_weights(macx, name):
    for n in (1, 4, 7):                                                         # n = 1 used to be broadcast into all B slots
        with pytest.raises(ValueError, match="weights=True"):
            load(tower(macx, name, weights=False), *batch(n))
    with pytest.raises(TypeError, match="no weights"):
        load(tower(macx, name, weights=False), *batch(B), weights=torch.ones(B))
    shared = dict(weights=False, G=G, image_index=torch.zeros(B, dtype=torch.int32), images=torch.zeros(G, N, 128))
    with pytest.raises(ValueError, match="weights=True"):                       # fewer shared images than the capture's
        load(tower(macx, name, **shared), *batch(B, g=2), image_index=torch.zeros(B, dtype=torch.int32))
    # a short batch is the first thing said, ahead of the shapes of the attention loss's arguments
    if name == "CapturedTowerTrainStep":
        built = dict(att_loss=dict(on="kb", kind="ce"), att_target=torch.zeros(B, N), att_row_weights=torch.ones(B),
                     att_step_weights=torch.ones(3))
        with pytest.raises(ValueError, match="weights=True"):
            load(tower(macx, name, weights=False, **built), *batch(4), att_target=torch.zeros(4, N))


@pytest.mark.parametrize("name", TOWER_CLASSES)
def test_a_class_built_without_weights_takes_any_image_layout_with_the_right_count(macx, name):
    """as before this change: the images are reshaped into the static tensor, [B * N, C] included"""
    obj = tower(macx, name, weights=False, images=torch.full((B, N, 128), -1.0), questions=torch.zeros(B, S, dtype=torch.int32),
                lengths=torch.zeros(B, dtype=torch.int32), answers=torch.zeros(B, dtype=torch.int32) if name.endswith("Step") else None)
    images, q, lengths, answers = batch(B)
    flat = torch.arange(B * N * 128, dtype=torch.float32).reshape(B * N, 128)
    assert load(obj, flat, q, lengths, answers) == B
    assert torch.equal(obj.images, flat.reshape(B, N, 128)) and torch.equal(obj.questions, q) and torch.equal(obj.lengths, lengths)


def test_forward_takes_answers_exactly_when_built_with_score(macx):
    images, q, lengths, answers = batch(B)
    with pytest.raises(TypeError, match="no answers"):
        tower(macx, "CapturedTowerForward", weights=False).load(images, q, lengths, answers=answers)
    with pytest.raises(TypeError, match="needs answers"):
        tower(macx, "CapturedTowerForward").load(images, q, lengths)


@pytest.mark.parametrize("name", TOWER_CLASSES)
@pytest.mark.parametrize("n", [0, B + 1])
def test_batch_size_outside_the_capture_is_refused(macx, name, n):
    with pytest.raises(ValueError, match="1 <= n <= %d" % B):
        load(tower(macx, name), *batch(n))


@pytest.mark.parametrize("name", TOWER_CLASSES)
def test_every_per_question_argument_must_have_the_leading_size(macx, name):
    n = 4
    images, q, lengths, answers = batch(n)
    wrong = lambda t: torch.cat([t, t[:1]])                                      # n + 1 entries
    with pytest.raises(ValueError, match="lengths"):
        load(tower(macx, name), images, q, wrong(lengths), answers)
    with pytest.raises(ValueError, match="answers"):
        load(tower(macx, name), images, q, lengths, wrong(answers))
    with pytest.raises(ValueError, match="images"):
        load(tower(macx, name), wrong(images), q, lengths, answers)
    kbl = torch.ones(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="kb_lengths"):
        load(tower(macx, name, kb_lengths=torch.ones(B, dtype=torch.int32)), images, q, lengths, answers, kb_lengths=wrong(kbl))
    with pytest.raises(ValueError, match="kb_lengths"):                          # the capture's B is no longer the right size either
        load(tower(macx, name, kb_lengths=torch.ones(B, dtype=torch.int32)), images, q, lengths, answers,
             kb_lengths=torch.ones(B, dtype=torch.int32))
    shared = dict(G=G, image_index=torch.zeros(B, dtype=torch.int32))
    index = torch.zeros(n, dtype=torch.int32)
    with pytest.raises(ValueError, match="image_index"):
        load(tower(macx, name, **shared), batch(n, g=2)[0], q, lengths, answers, image_index=wrong(index))
    with pytest.raises(ValueError, match="images"):                             # more shared images than the capture's
        load(tower(macx, name, **shared), batch(n, g=G + 1)[0], q, lengths, answers, image_index=index)
    with pytest.raises(ValueError, match="image_lengths"):                      # one size per LOADED image
        load(tower(macx, name, image_lengths=torch.ones(G, dtype=torch.int32), **shared), batch(n, g=2)[0], q, lengths, answers,
             image_index=index, image_lengths=torch.ones(G, dtype=torch.int32))
    # weights: one per question, float32
    with pytest.raises(ValueError, match="weights"):
        load(tower(macx, name), images, q, lengths, answers, weights=torch.ones(n + 1))
    with pytest.raises(ValueError, match="weights"):
        load(tower(macx, name), images, q, lengths, answers, weights=torch.ones(B))
    with pytest.raises(TypeError, match="weights"):
        load(tower(macx, name), images, q, lengths, answers, weights=torch.ones(n, dtype=torch.float64))


def test_attention_loss_arguments_follow_the_short_batch(macx):
    n, p = 4, 3
    images, q, lengths, answers = batch(n)
    built = dict(att_loss=dict(on="kb", kind="ce"), att_target=torch.zeros(B, N), att_row_weights=torch.ones(B),
                 att_step_weights=torch.ones(p))
    step = lambda: tower(macx, "CapturedTowerTrainStep", **built)
    with pytest.raises(ValueError, match="att_target"):
        load(step(), images, q, lengths, answers, att_target=torch.zeros(B, N))
    with pytest.raises(ValueError, match="att_row_weights"):
        load(step(), images, q, lengths, answers, att_target=torch.zeros(n, N), att_row_weights=torch.ones(B))
    per_step = dict(built, att_target=torch.zeros(p, B, N))
    with pytest.raises(ValueError, match="att_target"):
        load(tower(macx, "CapturedTowerTrainStep", **per_step), images, q, lengths, answers, att_target=torch.zeros(p, B, N))


def test_constructors_refuse_before_the_device(macx):
    net = small_net(macx)
    make = lambda **kw: macx.CapturedTowerTrainStep(net, None, None, B, S, H=5, W=5, imageInDim=128, **kw)
    with pytest.raises(TypeError, match="totals"):
        make(weights=True, totals=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights=True"):
        make(totals=True)

    class Spanning:                                            # a bucket over more than one process: out of scope
        _active = staticmethod(lambda: True)
    with pytest.raises(ValueError, match="more than one process"):
        macx.CapturedTowerTrainStep(net, None, Spanning(), B, S, H=5, W=5, imageInDim=128, weights=True)
    with pytest.raises(RuntimeError, match="HIP device"):      # valid arguments: on to the device
        make(weights=True, totals=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        macx.CapturedTowerForward(net, B, S, H=5, W=5, imageInDim=128, score=True)
