"""The host side of questions resident in device memory (macx_questions_gather / macx_preds_scatter, macx.QuestionStore,
macx.EpochOrder, `questions=` / `predictions=` on CapturedTowerForward / CapturedTowerTrainStep): the exports against the header,
every MACX_EINVAL of the two calls (returned before any HIP call, so without a device), the store's validation by exception type,
the epoch order, and the constructors' refusals, all raised before the device is asked.  No GPU."""
import ctypes as C
import inspect

import pytest
import torch

from test_abi_host import header_prototypes, prototype_mismatches
from test_feature_store_host import cpu_store
from test_lengths_paths_host import bare
from test_tower_graph_host import small_net

NEW = ("macx_questions_gather", "macx_preds_scatter")
B, S = 6, 7
A16 = 0x10000           # addresses that are never dereferenced: every call below is refused before anything is launched


def test_exports_are_in_the_table_in_the_headers_place(macx):
    protos = header_prototypes()
    for n in NEW:
        assert n in macx._lib.EXPORTS and n in macx._lib.TABLE and n in protos, n
    assert prototype_mismatches({n: macx._lib.TABLE[n] for n in NEW}) == []
    assert protos["macx_questions_gather"] == ("int", ["pointer"] * 6 + ["int", "int", "pointer", "int", "int"] + ["pointer"] * 6
                                               + ["pointer", "int", "pointer", "pointer"])
    assert protos["macx_preds_scatter"] == ("int", ["pointer", "pointer", "int", "int", "pointer", "pointer"])
    order = list(macx._lib.EXPORTS)
    at = order.index("macx_features_gather")
    assert tuple(order[at + 1:at + 3]) == NEW                             # directly behind macx_features_gather, as in the header
    L = macx._lib.lib()
    for n in NEW:
        assert list(getattr(L, n).argtypes) == list(macx._lib.TABLE[n][1]) and getattr(L, n).restype is C.c_int
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5       # new exports only, no struct


# a legal call, then one argument at a time made illegal
NAMES = ("q_words", "q_lengths", "q_answers", "q_images", "q_kb_len", "q_weights", "Q", "S_tab", "ids", "B", "S", "questions", "lengths",
         "answers", "image_ids", "kb_lengths", "weights", "image_index", "G", "bad")
GATHER_OK = dict(zip(NAMES, (A16, 2 * A16, 3 * A16, 4 * A16, 5 * A16, 6 * A16, 9, 6, 7 * A16, 5, 8, 8 * A16, 9 * A16, 10 * A16, 11 * A16,
                             12 * A16, 13 * A16, 0, 0, 14 * A16)))
GROUP_OK = dict(GATHER_OK, image_index=15 * A16, G=3)
GATHER_BAD = [("q_words", 0), ("q_lengths", 0), ("ids", 0), ("questions", 0), ("lengths", 0), ("Q", 0), ("Q", -1), ("S_tab", 0), ("B", 0),
              ("B", -4), ("S", 5), ("S", 0), ("q_answers", 0), ("q_images", 0), ("q_kb_len", 0), ("q_words", A16 + 2), ("ids", 7 * A16 + 1),
              ("questions", 8 * A16 + 2), ("weights", 13 * A16 + 2), ("q_weights", 6 * A16 + 1), ("bad", 14 * A16 + 2),
              ("kb_lengths", 12 * A16 + 3), ("q_lengths", 2 * A16 + 2)]
GROUP_BAD = [("G", 0), ("G", -1), ("B", 1025), ("q_images", 0), ("image_ids", 0), ("image_index", 15 * A16 + 2)]
SCATTER_OK = dict(pred=A16, ids=2 * A16, B=5, Q=9, table=3 * A16)
SCATTER_BAD = [("pred", 0), ("ids", 0), ("table", 0), ("B", 0), ("B", -1), ("Q", 0), ("Q", -3), ("pred", A16 + 2), ("ids", 2 * A16 + 1),
               ("table", 3 * A16 + 2)]


def gather(L, a):
    return L.macx_questions_gather(*[a[n] for n in NAMES], None)


@pytest.mark.parametrize("name,value", GATHER_BAD)
def test_gather_refuses_before_any_launch(macx, name, value):
    assert gather(macx._lib.lib(), dict(GATHER_OK, **{name: value})) == macx._lib.MACX_EINVAL


@pytest.mark.parametrize("name,value", GROUP_BAD)
def test_grouping_refuses_before_any_launch(macx, name, value):
    assert gather(macx._lib.lib(), dict(GROUP_OK, **{name: value})) == macx._lib.MACX_EINVAL


def test_an_output_column_without_its_table_is_refused_on_every_row_path(macx):
    """(weights without q_weights is the one pairing that is taken: tests/test_gpu_questions_gather.py runs it)"""
    L = macx._lib.lib()
    for S_tab, S_ in ((4, 4), (6, 8), (5, 7)):
        for table in ("q_answers", "q_images", "q_kb_len"):
            assert gather(L, dict(GATHER_OK, S_tab=S_tab, S=S_, **{table: 0})) == macx._lib.MACX_EINVAL


@pytest.mark.parametrize("name,value", SCATTER_BAD)
def test_scatter_refuses_before_any_launch(macx, name, value):
    a = dict(SCATTER_OK, **{name: value})
    assert macx._lib.lib().macx_preds_scatter(a["pred"], a["ids"], a["B"], a["Q"], a["table"], None) == macx._lib.MACX_EINVAL


# ---- QuestionStore -----------------------------------------------------------------------------------------------------------------
Q = 8


def columns(seed=0):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, S + 1, (Q,), generator=g, dtype=torch.int32)
    q = torch.randint(1, 12, (Q, S), generator=g, dtype=torch.int32) * (torch.arange(S)[None] < lengths[:, None]).to(torch.int32)
    return dict(questions=q, lengths=lengths, answers=torch.randint(0, 28, (Q,), generator=g), image_rows=torch.randint(0, 5, (Q,), generator=g),
                kb_lengths=torch.randint(1, 26, (Q,), generator=g), weights=torch.rand(Q, generator=g))


def cpu_questions(macx, device="cpu", **over):
    return macx.QuestionStore(device=device, **dict(columns(), **over))


def test_store_attributes(macx):
    c = columns()
    s = cpu_questions(macx)
    assert (s.count, s.S, s.device) == (Q, S, torch.device("cpu"))
    assert s.max_word == int(c["questions"].max()) and s.max_answer == int(c["answers"].max())
    assert s.nbytes == Q * S * 4 + 5 * Q * 4
    for name in ("questions", "lengths", "answers", "image_rows", "kb_lengths"):
        assert getattr(s, name).dtype == torch.int32 and torch.equal(getattr(s, name), c[name].to(torch.int32)), name
    assert s.weights.dtype == torch.float32 and torch.equal(s.weights, c["weights"])
    assert tuple(s.bad.shape) == (1,) and s.bad.dtype == torch.int32 and int(s.bad) == 0
    bare_ = macx.QuestionStore(c["questions"].numpy(), c["lengths"].tolist(), device="cpu")       # arrays and lists are taken too
    assert (bare_.answers, bare_.image_rows, bare_.kb_lengths, bare_.weights, bare_.max_answer) == (None,) * 5
    assert bare_.nbytes == Q * S * 4 + Q * 4 and torch.equal(bare_.questions, s.questions)
    assert macx.questions.QuestionStore is macx.QuestionStore and macx.questions.EpochOrder is macx.EpochOrder
    assert tuple(s.predictions().shape) == (Q,) and s.predictions().dtype == torch.int32 and bool((s.predictions() == -1).all())


def test_store_validation(macx):
    c = columns()
    with pytest.raises(TypeError, match="integer dtype"):
        cpu_questions(macx, questions=c["questions"].float())
    with pytest.raises(TypeError, match="array or a tensor"):
        cpu_questions(macx, lengths=3)
    for bad in (c["questions"][0], torch.zeros(0, S, dtype=torch.int32), torch.zeros(Q, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\[count, S\]"):
            cpu_questions(macx, questions=bad)
    q = c["questions"].clone()
    q[3, 2] = -1
    with pytest.raises(ValueError, match="word ids must be >= 0"):
        cpu_questions(macx, questions=q)
    for bad in (-1, S + 1):
        lengths = c["lengths"].clone()
        lengths[5] = bad
        with pytest.raises(ValueError, match=r"lengths must lie in \[0, 7\]"):
            cpu_questions(macx, lengths=lengths)
    assert cpu_questions(macx, lengths=torch.zeros(Q, dtype=torch.int32)).count == Q              # 0 is a legal length
    for name, bad in (("answers", -1), ("image_rows", -1), ("kb_lengths", 0)):
        col = c[name].clone()
        col[Q - 1] = bad
        with pytest.raises(ValueError, match="%s must be >= %d" % (name, bad + 1)):
            cpu_questions(macx, **{name: col})
        with pytest.raises(ValueError, match=r"%s must be \[8\]" % name):
            cpu_questions(macx, **{name: c[name][:-1]})
        with pytest.raises(TypeError, match="integer dtype"):
            cpu_questions(macx, **{name: c[name].float()})
    with pytest.raises(ValueError, match="does not fit int32"):
        cpu_questions(macx, image_rows=torch.full((Q,), 1 << 31))
    with pytest.raises(TypeError, match="floating-point"):
        cpu_questions(macx, weights=torch.ones(Q, dtype=torch.int32))
    for bad in (float("nan"), float("inf")):
        w = c["weights"].clone()
        w[0] = bad
        with pytest.raises(ValueError, match="finite"):
            cpu_questions(macx, weights=w)
    assert cpu_questions(macx, weights=c["weights"].double().numpy()).weights.dtype == torch.float32


def test_check_reads_the_bad_word(macx):
    s = cpu_questions(macx)
    assert s.check() is s
    s.bad.fill_(1)
    with pytest.raises(ValueError, match="outside"):
        s.check()
    assert s.reset_bad().check() is s


def test_check_ids_and_no_cpu_path(macx):
    s = cpu_questions(macx)
    for bad in (torch.zeros(2, 2, dtype=torch.int32), [0, 1]):
        with pytest.raises(ValueError, match="question ids must be a"):
            s.gather(bad)
    with pytest.raises(ValueError, match=r"must be a \[3\]"):
        s.check_ids(torch.zeros(4, dtype=torch.int32), 3)
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="integer dtype"):
            s.check_ids(bad)
    for bad in ([0, Q, 1], [0, -1, 1]):
        with pytest.raises(IndexError, match=r"outside \[0, 8\)"):
            s.check_ids(torch.tensor(bad), host_check=True)
    assert s.check_ids(torch.tensor([0, Q, -1])) is not None                # without host_check the range is the kernel's business
    with pytest.raises(ValueError, match="narrower"):
        s.gather(torch.tensor([0, 1]), S=S - 1)
    with pytest.raises(ValueError, match="holds no image_rows"):
        cpu_questions(macx, image_rows=None).gather(torch.tensor([0, 1]), images=2)
    with pytest.raises(ValueError, match="at most 1024"):
        s.gather(torch.zeros(1025, dtype=torch.int32), images=2)
    with pytest.raises(ValueError, match="G >= 1"):
        s.gather(torch.tensor([0, 1]), images=0)
    with pytest.raises(RuntimeError, match="HIP device"):                   # a legal call: on to the device, and there is none
        s.gather(torch.tensor([0, 7, 7]))


# ---- EpochOrder --------------------------------------------------------------------------------------------------------------------
def test_epoch_order(macx):
    s = cpu_questions(macx)
    for b, steps in ((3, 3), (4, 2), (8, 1), (9, 1), (1, 8)):              # count % B both 0 and not
        assert macx.EpochOrder(s, b).steps == steps, b
    order = macx.EpochOrder(s, 3)
    assert order.order.dtype == torch.int32 and order.order.tolist() == list(range(Q)) and order.position == 0 and order.remaining == Q
    assert [order.take().tolist() for _ in range(3)] == [[0, 1, 2], [3, 4, 5], [6, 7]] and order.position == Q
    with pytest.raises(IndexError, match="exhausted"):
        order.take()
    perm = torch.tensor([5, 2, 7, 0, 1, 6, 4, 3])
    assert order.rewind(perm) is order and order.position == 0
    assert [order.take().tolist() for _ in range(3)] == [[5, 2, 7], [0, 1, 6], [4, 3]]
    with pytest.raises(IndexError):
        order.take()
    order.rewind()                                                          # None: 0 .. count-1 again
    assert order.take().tolist() == [0, 1, 2] and order.position == 3
    assert macx.EpochOrder(s, 4, order=perm).take().tolist() == [5, 2, 7, 0]
    for bad, exc in ((perm[:-1], ValueError), (perm.float(), ValueError), (perm + 1, IndexError), (perm - 1, IndexError)):
        with pytest.raises(exc):
            order.rewind(bad)
    with pytest.raises(TypeError, match="QuestionStore"):
        macx.EpochOrder(cpu_store(macx), 3)
    with pytest.raises(ValueError, match="at least 1"):
        macx.EpochOrder(s, 0)


# ---- the captured classes ----------------------------------------------------------------------------------------------------------
def test_new_keywords_default_to_off(macx):
    for cls in (macx.CapturedTowerForward, macx.CapturedTowerTrainStep):
        assert inspect.signature(cls.__init__).parameters["questions"].default is None, cls
        assert cls.question_store is None and cls.question_ids is None and cls.predictions is None
        assert inspect.signature(cls.load_ids).parameters["check_ids"].default is True
    assert inspect.signature(macx.CapturedTowerForward.__init__).parameters["predictions"].default is None


def makers(macx, net):
    return (lambda **kw: macx.CapturedTowerForward(net, B, S, **kw),
            lambda **kw: macx.CapturedTowerTrainStep(net, None, None, B, S, **kw))


def test_constructors_refuse_before_the_device(macx):
    """the net lives on the host, so a construction that passes every refusal ends at the device's RuntimeError: everything listed
    here is raised in front of it"""
    net = small_net(macx, stemDropout=1.0)                                  # vocab 11, 28 answers, 5 x 5 x 128 image features
    feats = cpu_store(macx)
    c = columns()
    full = cpu_questions(macx)
    plain = cpu_questions(macx, image_rows=None)
    for make in makers(macx, net):
        with pytest.raises(TypeError, match="macx.QuestionStore"):
            make(questions=feats)
        with pytest.raises(TypeError, match="macx.QuestionStore"):
            make(questions=c["questions"])
        with pytest.raises(ValueError, match="questions of 7 words"):
            macx.CapturedTowerForward(net, B, S - 1, questions=plain)
        with pytest.raises(ValueError, match="vocabulary ends at 11"):
            make(questions=cpu_questions(macx, image_rows=None, questions=c["questions"] + 1))    # (holds word id 12)
        with pytest.raises(ValueError, match="classifier has 28 answers"):
            make(questions=cpu_questions(macx, image_rows=None, answers=torch.full((Q,), 28)))
        with pytest.raises(ValueError, match="the store holds no image_rows"):
            make(questions=plain, features=feats)
        with pytest.raises(ValueError, match="no features= was given"):
            make(questions=full)
        with pytest.raises(ValueError, match="holds no kb_lengths"):
            make(questions=cpu_questions(macx, image_rows=None, kb_lengths=None), kb_lengths=True)
        with pytest.raises(ValueError, match="needs features="):
            make(questions=plain, images=2)
        with pytest.raises(ValueError, match="image_lengths=True is out of scope"):
            make(questions=full, features=feats, images=2, image_lengths=True)
        with pytest.raises(ValueError, match="lives on meta"):
            make(questions=cpu_questions(macx, device="meta", image_rows=None))
        with pytest.raises(RuntimeError, match="HIP device"):               # nothing to refuse: on to the device
            make(questions=plain)
        with pytest.raises(RuntimeError, match="HIP device"):
            make(questions=full, features=feats, images=2, kb_lengths=True)
    with pytest.raises(ValueError, match="at most 1024 questions"):
        macx.CapturedTowerForward(net, 1025, S, questions=full, features=feats, images=2)
    with pytest.raises(RuntimeError, match="HIP device"):                   # (one image per question has no such cap)
        macx.CapturedTowerForward(net, 1025, S, questions=full, features=feats)
    with pytest.raises(ValueError, match="att_loss= is out of scope"):
        macx.CapturedTowerTrainStep(net, None, None, B, S, questions=plain, att_loss=dict(on="kb", kind="entropy"))
    with pytest.raises(ValueError, match="holds none"):                     # the classes that read answers need them in the store
        macx.CapturedTowerTrainStep(net, None, None, B, S, questions=cpu_questions(macx, image_rows=None, answers=None))
    with pytest.raises(ValueError, match="holds none"):
        macx.CapturedTowerForward(net, B, S, questions=cpu_questions(macx, image_rows=None, answers=None), score=True)
    # predictions=: a table over the store, and with questions= only
    with pytest.raises(ValueError, match="build the class with questions="):
        macx.CapturedTowerForward(net, B, S, predictions=plain.predictions())
    for bad in (plain.predictions()[:-1], plain.predictions().long(), plain.predictions().tolist()):
        with pytest.raises(ValueError, match=r"contiguous \[8\] int32"):
            macx.CapturedTowerForward(net, B, S, questions=plain, predictions=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        macx.CapturedTowerForward(net, B, S, questions=plain, predictions=plain.predictions())


@pytest.mark.parametrize("name", ["CapturedTowerForward", "CapturedTowerTrainStep"])
def test_a_batch_is_ids_exactly_when_built_with_questions(macx, name):
    store = cpu_questions(macx)
    q, lengths = torch.ones(B, S, dtype=torch.int32), torch.full((B,), S, dtype=torch.int32)
    tail = (torch.zeros(B, dtype=torch.int32),) if name == "CapturedTowerTrainStep" else ()
    plain = bare(macx, name, B=B, S=S, N=25)
    for call in (lambda: plain.load_ids(torch.zeros(B, dtype=torch.int32)), lambda: plain.next_batch(macx.EpochOrder(store, B))):
        with pytest.raises(TypeError, match="built with questions="):
            call()
    ids = lambda: torch.full((B,), 5, dtype=torch.int32)
    built = bare(macx, name, B=B, S=S, N=25, question_store=store, question_ids=ids())
    with pytest.raises(ValueError, match="load_ids"):
        built.load(torch.zeros(B, 25, 128), q, lengths, *tail)
    assert built.load_ids(torch.tensor([7, 0, 3, 3, 1, 2])) == B and built.question_ids.tolist() == [7, 0, 3, 3, 1, 2] and built.n == B
    with pytest.raises(ValueError, match=r"captured for batches of 6 questions and got 2"):     # load()'s rule and message
        built.load_ids(torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="integer dtype"):
        built.load_ids(torch.zeros(B))
    with pytest.raises(ValueError, match="question ids must be a"):
        built.load_ids(torch.zeros(B, 1, dtype=torch.int32))
    for bad in ([0, 1, 2, 3, 4, Q], [0, -1, 2, 3, 4, 5]):
        with pytest.raises(IndexError, match=r"outside \[0, 8\)"):
            built.load_ids(torch.tensor(bad))
    assert built.load_ids(torch.tensor([0, 1, 2, 3, 4, Q]), check_ids=False) == B             # unchecked: the kernel poisons it
    assert built.question_ids.tolist() == [0, 1, 2, 3, 4, Q]
    # a class with weights takes short batches: -1 behind the n ids
    short = bare(macx, name, B=B, S=S, N=25, question_store=store, question_ids=ids(), weights=torch.ones(B))
    assert short.load_ids(torch.tensor([4, 2])) == 2 and short.question_ids.tolist() == [4, 2, -1, -1, -1, -1] and short.n == 2
    for bad in (torch.zeros(0, dtype=torch.int32), torch.zeros(B + 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="1 <= n <= 6"):
            short.load_ids(bad)
    # next_batch: 8 questions at B = 6 are batches of 6 and 2
    order = macx.EpochOrder(store, B, order=torch.tensor([5, 2, 7, 0, 1, 6, 4, 3]))
    assert short.next_batch(order) == B and short.question_ids.tolist() == [5, 2, 7, 0, 1, 6]
    assert short.next_batch(order) == 2 and short.question_ids.tolist() == [4, 3, -1, -1, -1, -1] and short.n == 2
    with pytest.raises(IndexError, match="exhausted"):
        short.next_batch(order)
    order.rewind()
    assert built.next_batch(order) == B and built.question_ids.tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="got 2"):                          # the short last batch needs weights; the order stays put
        built.next_batch(order)
    assert order.position == B
    for other in (macx.EpochOrder(store, B - 1), macx.EpochOrder(cpu_questions(macx), B)):
        with pytest.raises(ValueError, match="EpochOrder over this class's QuestionStore"):
            built.next_batch(other)
