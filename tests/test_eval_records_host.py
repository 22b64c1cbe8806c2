"""The host side of evaluation records resident in device memory (macx_records_scatter, macx_record_desc, macx.EvalRecords,
`records=` on CapturedTowerForward): the export and the struct against the header, every MACX_EINVAL of the call (returned before
any HIP call, so without a device), the constructor's and file()'s refusals, the captured class's refusals -- all raised before the
device is asked -- and instances() against what the reference's own buildPredsList returned
(tests/golden/eval_records/preds_list.json, recorded by tools/record_preds_list.py; replayed here without the reference).  No GPU."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import records_ref
from test_abi_host import header_code, header_prototypes, header_structs, prototype_mismatches
from test_question_store_host import Q, S, columns, cpu_questions
from test_tower_graph_host import small_net

NAME = "macx_records_scatter"
A16 = 0x10000           # addresses that are never dereferenced: every raw call below is refused before anything is launched
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_records", "preds_list.json")


def test_export_and_struct_against_the_header(macx):
    lib = macx._lib
    protos = header_prototypes()
    assert NAME in lib.EXPORTS and NAME in lib.TABLE and NAME in protos
    assert prototype_mismatches({NAME: lib.TABLE[NAME]}) == []
    assert protos[NAME] == ("int", ["pointer", "int", "pointer", "int", "int", "pointer"])
    order = list(lib.EXPORTS)
    assert order[order.index("macx_preds_scatter") + 1] == NAME                    # directly behind macx_preds_scatter, as in the header
    assert header_structs()["macx_record_desc"] == [("src", "pointer"), ("table", "pointer"), ("steps", "int32"), ("n", "int32"),
                                                    ("dtype", "int32")]
    D = lib.MacxRecordDesc
    assert [f for f, _ in D._fields_] == ["src", "table", "steps", "n", "dtype"]
    assert C.sizeof(D) == 32 and [getattr(D, f).offset for f in ("src", "table", "steps", "n", "dtype")] == [0, 8, 16, 20, 24]
    assert "MACX_RECORDS_MAX = 4" in header_code() and lib.RECORDS_MAX == 4
    L = lib.lib()
    f = getattr(L, NAME)
    assert list(f.argtypes) == list(lib.TABLE[NAME][1]) and f.restype is C.c_int
    assert lib.ABI_VERSION == 5 and L.macx_abi_version() == 5                      # a new export and a new struct; nothing else moved


# a legal call, then one argument at a time made illegal
DESC_OK = dict(src=A16, table=2 * A16, steps=12, n=196, dtype=1)
CALL_OK = dict(count=1, ids=3 * A16, B=64, Q=300)
DESC_BAD = [("src", 0), ("table", 0), ("steps", 0), ("steps", -1), ("n", 0), ("n", -5), ("dtype", 2), ("dtype", -1), ("src", A16 + 2),
            ("src", A16 + 1), ("table", 2 * A16 + 1)]
CALL_BAD = [("count", 0), ("count", -1), ("count", 5), ("ids", 0), ("ids", 3 * A16 + 2), ("B", 0), ("B", -2), ("Q", 0), ("Q", -1)]


def raw(macx, descs, descs_null=False, **over):
    a = dict(CALL_OK, **over)
    arr = (macx._lib.MacxRecordDesc * max(len(descs), 5))()
    for slot, d in zip(arr, descs):
        slot.src, slot.table, slot.steps, slot.n, slot.dtype = d["src"], d["table"], d["steps"], d["n"], d["dtype"]
    return macx._lib.lib().macx_records_scatter(None if descs_null else arr, a["count"], a["ids"], a["B"], a["Q"], None)


@pytest.mark.parametrize("name,value", DESC_BAD)
def test_a_bad_descriptor_is_refused_before_any_launch(macx, name, value):
    bad = dict(DESC_OK, **{name: value})
    assert raw(macx, [bad]) == macx._lib.MACX_EINVAL
    for k in range(4):                                                            # ... wherever it stands among four
        descs = [dict(DESC_OK, table=(2 + j) * A16 * 4) for j in range(4)]
        descs[k] = bad
        assert raw(macx, descs, count=4) == macx._lib.MACX_EINVAL, k


@pytest.mark.parametrize("name,value", CALL_BAD)
def test_a_bad_call_is_refused_before_any_launch(macx, name, value):
    assert raw(macx, [DESC_OK] * 4, **{name: value}) == macx._lib.MACX_EINVAL


def test_null_descs_and_a_table_off_its_element_size(macx):
    EINVAL = macx._lib.MACX_EINVAL
    assert raw(macx, [DESC_OK], descs_null=True) == EINVAL
    assert raw(macx, [dict(DESC_OK, dtype=0, table=2 * A16 + 2)]) == EINVAL       # fp32 table off 4 bytes (an fp16 one may sit there)
    assert raw(macx, [dict(DESC_OK, dtype=1, table=2 * A16 + 3)]) == EINVAL
    assert macx._lib.lib().macx_records_scatter(None, 0, None, 0, 0, None) == EINVAL


# ---- EvalRecords -------------------------------------------------------------------------------------------------------------------
P, N, A = 3, 25, 28


def records(macx, store=None, **over):
    kw = dict(p=P, N=N, S=S, answers=A, maps=("kb", "question"), logits=True, dtype=torch.float16)
    return macx.EvalRecords(cpu_questions(macx) if store is None else store, **dict(kw, **over))


def test_tables_attributes_and_clear(macx):
    assert macx.records.EvalRecords is macx.EvalRecords
    store = cpu_questions(macx)
    r = records(macx, store)
    assert (r.store, r.count, r.device, r.p, r.N, r.S, r.answers, r.dtype) == (store, Q, torch.device("cpu"), P, N, S, A, torch.float16)
    assert list(r.tables) == ["kb", "question", "logits"]
    assert {k: (tuple(t.shape), t.dtype) for k, t in r.tables.items()} == {
        "kb": ((Q, P, N), torch.float16), "question": ((Q, P, S), torch.float16), "logits": ((Q, 1, A), torch.float32)}
    assert r.nbytes == Q * P * (N + S) * 2 + Q * A * 4
    assert all(bool(torch.isnan(t).all()) for t in r.tables.values())             # never filed: NaN
    r.tables["kb"].zero_()
    assert r.clear() is r and bool(torch.isnan(r.tables["kb"]).all())
    full = records(macx, maps=("self", "question", "kb"), dtype=torch.float32)
    assert list(full.tables) == ["kb", "question", "self", "logits"] and tuple(full.tables["self"].shape) == (Q, P, P)
    assert all(t.dtype == torch.float32 for t in full.tables.values())
    bare = records(macx, maps=("kb",), logits=False)
    assert list(bare.tables) == ["kb"] and bare.answers is None
    assert records(macx, maps=(), answers=2).nbytes == Q * 2 * 4
    assert "EvalRecords of 8 questions" in repr(r)
    got = r.read()
    assert set(got) == set(r.tables) and got["kb"].dtype == np.float16 and got["kb"].shape == (Q, P, N) and np.isnan(got["logits"]).all()
    assert r.read([5, 0, 5])["question"].shape == (3, P, S)
    for bad in ([0, Q], [-1]):
        with pytest.raises(IndexError, match=r"outside \[0, 8\)"):
            r.read(bad)
    with pytest.raises(ValueError, match="1-D integer"):
        r.read([0.5])


def test_constructor_refusals(macx):
    with pytest.raises(TypeError, match="macx.QuestionStore"):
        macx.EvalRecords(columns()["questions"], p=P, N=N, S=S, answers=A)
    for name in ("p", "N", "S"):
        with pytest.raises(ValueError, match="%s must be at least 1" % name):
            records(macx, **{name: 0})
    for bad in (torch.bfloat16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="torch.float16 or torch.float32"):
            records(macx, dtype=bad)
    for bad in (("gate",), ("kb", "controls")):
        with pytest.raises(ValueError, match="no attention map"):
            records(macx, maps=bad)
    with pytest.raises(ValueError, match="twice"):
        records(macx, maps=("kb", "kb"))
    for bad in (None, 0):
        with pytest.raises(ValueError, match="needs answers"):
            records(macx, answers=bad)
    with pytest.raises(ValueError, match="nothing to record"):
        records(macx, maps=(), logits=False)


def test_file_refusals_come_before_the_device(macx):
    r = records(macx, maps=("kb", "question", "self"), dtype=torch.float32)
    B = 4
    ids = torch.tensor([0, 3, -1, 3], dtype=torch.int32)
    ok = dict(kb=torch.zeros(P, B, N), question=torch.zeros(P, B, S), self_att=torch.zeros(P, B, P), logits=torch.zeros(B, A))
    for missing in ok:
        with pytest.raises(ValueError, match="no %s= was given" % missing):
            r.file(ids, **{k: v for k, v in ok.items() if k != missing})
    small = records(macx, maps=("kb",), logits=False)
    for extra in ("question", "self_att", "logits"):
        with pytest.raises(ValueError, match="%s= was given and the records hold no" % extra):
            small.file(ids, kb=ok["kb"], **{extra: ok[extra]})
    for name, bad in (("kb", torch.zeros(P, B, N + 1)), ("kb", torch.zeros(B, P, N)), ("kb", torch.zeros(P, B, N).double()),
                      ("question", torch.zeros(P, B, 2 * S)[:, :, ::2]), ("question", [[0.0]]), ("self_att", torch.zeros(P, B + 1, P)),
                      ("logits", torch.zeros(1, B, A)), ("logits", torch.zeros(B, A, device="meta"))):
        with pytest.raises(ValueError, match="%s must be a contiguous float32" % name):
            r.file(ids, **dict(ok, **{name: bad}))
    for bad in ([0, 1, 2, 3], torch.zeros(2, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="question ids must be a"):
            r.file(bad, **ok)
    with pytest.raises(ValueError, match="integer dtype"):
        r.file(torch.zeros(B), **ok)
    with pytest.raises(ValueError, match="names no slot"):
        r.file(torch.zeros(0, dtype=torch.int32), **{k: v[:, :0] if v.dim() == 3 else v[:0] for k, v in ok.items()})
    with pytest.raises(RuntimeError, match="HIP device"):                           # a legal call: on to the device, and there is none
        r.file(ids, **ok)
    cell = type("Cell", (), {"state_tensor": lambda self, name: {"att_kb": ok["kb"], "att_question": ok["question"]}[name]})()
    with pytest.raises(ValueError, match="the cell's run has no att_self"):
        r.file_run(ids, cell, ok["logits"])
    with pytest.raises(RuntimeError, match="HIP device"):
        records(macx, dtype=torch.float32).file_run(ids, cell, ok["logits"])


def test_topk(macx):
    r = records(macx, answers=4, maps=())
    logits = torch.tensor([[0.0, 3.0, 1.0, -1.0], [2.0, 2.0, 5.0, 0.0]])
    r.tables["logits"][2, 0], r.tables["logits"][5, 0] = logits[0], logits[1]
    index, prob = r.topk(2)
    assert tuple(index.shape) == (Q, 2) and tuple(prob.shape) == (Q, 2) and prob.dtype == torch.float32
    assert index[2].tolist() == [1, 2] and index[5, 0].item() == 2
    assert torch.equal(prob[2], torch.softmax(logits[0], 0)[[1, 2]]) and bool(torch.isnan(prob[0]).all())
    for bad in (0, 5):
        with pytest.raises(ValueError, match="1 <= k <= 4"):
            r.topk(bad)
    with pytest.raises(ValueError, match="no logits table"):
        records(macx, logits=False).topk(1)


# ---- instances() against the reference's buildPredsList ------------------------------------------------------------------------------
def recorded(macx, dtype=torch.float32):
    """the fixture, and EvalRecords over a store of 6 questions whose rows 4, 1, 3 hold the fixture's three questions"""
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    count, ids = 6, [4, 1, 3]
    lengths, kb_lengths = torch.full((count,), 5), torch.full((count,), 4)
    lengths[ids], kb_lengths[ids] = torch.tensor(fx["lengths"]), torch.tensor(fx["kb_lengths"])
    store = macx.QuestionStore(torch.ones(count, fx["S"], dtype=torch.int32), lengths, kb_lengths=kb_lengths, device="cpu")
    r = macx.EvalRecords(store, p=fx["p"], N=fx["N"], S=fx["S"], answers=len(fx["answers"]), maps=("kb", "question", "self"), dtype=dtype)
    for name, steps in fx["maps"].items():
        src = np.asarray(steps, dtype=np.float64).astype(np.float32)               # [p, B, n]: what a run's `saved` holds
        assert np.array_equal(src.astype(np.float64), np.asarray(steps))           # (the fixture's numbers are fp32 values)
        filed = records_ref.scatter(r.tables[name].numpy(), src, np.asarray(ids))
        r.tables[name].copy_(torch.from_numpy(filed))
    predictions = torch.full((count,), -1, dtype=torch.int32)
    predictions[ids] = torch.tensor(fx["predictions"], dtype=torch.int32)
    return fx, r, ids, predictions


def test_instances_equal_the_references_preds_list(macx):
    fx, r, ids, predictions = recorded(macx)
    assert len(fx["preds_list"]) == fx["B"] == 3 and (fx["p"], fx["N"], fx["S"]) == (2, 4, 5)
    given = [dict(i) for i in fx["instances"]]
    got = r.instances(given, ids, predictions=predictions, decode=fx["answers"].__getitem__, trim=False)
    assert got == fx["preds_list"]                                                 # exactly: every number is the fp32 value as a double
    assert given == fx["instances"]                                                # copies: the caller's dicts are as they were
    assert json.loads(json.dumps(got)) == fx["preds_list"]                         # plain lists, strings and numbers
    plain = r.instances(given, torch.tensor(ids), predictions=predictions, trim=False)
    assert [i["prediction"] for i in plain] == fx["predictions"]                   # decode=None: the integer
    assert "prediction" not in r.instances(given, ids, trim=False)[0]              # predictions=None: as the reference leaves it out
    with pytest.raises(ValueError, match="one question id per instance"):
        r.instances(given, ids[:2])
    with pytest.raises(ValueError, match=r"\[6\] table"):
        r.instances(given, ids, predictions=predictions[:3])


def test_trim_cuts_rows_at_the_questions_own_lengths(macx):
    fx, r, ids, predictions = recorded(macx)
    whole = fx["preds_list"]
    got = r.instances(fx["instances"], ids, predictions=predictions, decode=fx["answers"].__getitem__)
    assert fx["lengths"] == [5, 2, 3] and fx["kb_lengths"] == [4, 3, 1]
    for j, (length, kb_length) in enumerate(((5, 4), (2, 3), (3, 1))):
        att, ref = got[j]["attentions"], whole[j]["attentions"]
        for i in range(2):
            assert att["question"][i] == ref["question"][i][:length] and len(att["question"][i]) == length
            assert att["kb"][i] == ref["kb"][i][:kb_length] and len(att["kb"][i]) == kb_length
            assert att["self"][i] == ref["self"][i][:i + 1]                         # row i: i + 1 entries, as cell.attentions["self"]
            assert all(v == 0.0 for v in ref["question"][i][length:] + ref["kb"][i][kb_length:])     # what was cut is exact zeros
        assert got[j]["prediction"] == whole[j]["prediction"]
    # a store without kb_lengths leaves the kb rows whole
    store = macx.QuestionStore(torch.ones(6, 5, dtype=torch.int32), r.store.lengths, device="cpu")
    other = macx.EvalRecords(store, p=2, N=4, S=5, maps=("kb", "question"), logits=False, dtype=torch.float32)
    other.tables["kb"].copy_(r.tables["kb"]); other.tables["question"].copy_(r.tables["question"])
    att = other.instances(fx["instances"], ids)[1]["attentions"]
    assert att["kb"] == whole[1]["attentions"]["kb"] and att["question"][0] == whole[1]["attentions"]["question"][0][:2]
    # fp16 tables read back as the fp16 values
    _, half, _, _ = recorded(macx, dtype=torch.float16)
    h = half.instances(fx["instances"], ids, trim=False)[0]["attentions"]["kb"][0]
    assert h == np.asarray(whole[0]["attentions"]["kb"][0], dtype=np.float32).astype(np.float16).astype(np.float64).tolist()


# ---- CapturedTowerForward(records=) --------------------------------------------------------------------------------------------------
def test_records_keyword_defaults_to_off(macx):
    assert inspect.signature(macx.CapturedTowerForward.__init__).parameters["records"].default is None
    assert macx.CapturedTowerForward.records is None
    assert "records" not in inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters      # out of scope: the training step


def test_captured_forward_refuses_before_the_device(macx):
    """the net lives on the host, so a construction that passes every refusal ends at the device's RuntimeError"""
    net = small_net(macx, stemDropout=1.0)                                         # vocab 11, 28 answers, 5 x 5 cells, 3 steps
    plain = cpu_questions(macx, image_rows=None)
    B = 6
    make = lambda **kw: macx.CapturedTowerForward(net, B, S, **kw)
    good = lambda **over: records(macx, plain, **over)
    with pytest.raises(ValueError, match="build the class with questions="):
        make(records=good())
    with pytest.raises(TypeError, match="macx.EvalRecords"):
        make(questions=plain, records=plain.predictions())
    with pytest.raises(ValueError, match="another QuestionStore"):
        make(questions=plain, records=records(macx, cpu_questions(macx, image_rows=None)))
    for name, value in (("p", 4), ("N", 16), ("S", S + 1), ("answers", 27)):
        with pytest.raises(ValueError, match="built for %s = %d" % (name, value)):
            make(questions=plain, records=good(**{name: value}))
    with pytest.raises(ValueError, match="without writeSelfAtt"):
        make(questions=plain, records=good(maps=("kb", "self")))
    moved = good()
    moved.device = torch.device("meta")
    with pytest.raises(ValueError, match="live on meta"):
        make(questions=plain, records=moved)
    with pytest.raises(RuntimeError, match="HIP device"):                           # nothing to refuse: on to the device
        make(questions=plain, records=good())
    with pytest.raises(RuntimeError, match="HIP device"):
        make(questions=plain, records=good(logits=False, dtype=torch.float32), score=True, predictions=plain.predictions())
