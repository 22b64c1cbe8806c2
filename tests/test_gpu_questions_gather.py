"""-m gpu: macx_questions_gather and macx_preds_scatter on their own, through the raw ABI.  Every expected value is an integer (or a
weight copied bit for bit) made by torch indexing on the CPU under the slot rules of include/macx.h; every output sits between guard
bands.

Shapes: Q = 9 questions; (S_tab, S) = (1, 1)/(5, 7), (6, 6)/(6, 8)/(50, 50) and (4, 4)/(8, 12): the scalar, the 8-byte and the 16-byte
row paths ((6, .) and (50, 50) are even and no multiple of 4: 8-byte accesses on rows that start off 16 bytes), with and without
padded columns.
B = 1, 5, 64 and one B behind a single pass of the capped grid (QG_MAX_BLOCKS workgroups of 256 threads, one unit each: units >= B)."""
import pytest
import torch

from abi_kit import Guarded, bits_equal, ptr

pytestmark = pytest.mark.gpu

Q = 9
SHAPES = [(1, 1), (4, 4), (6, 6), (6, 8), (8, 12), (50, 50), (5, 7)]
QG_MAX_BLOCKS = 256                                   # macx_questions.hip.h: the grid cap; a pass covers QG_MAX_BLOCKS * 256 units
B_BEHIND_A_PASS = QG_MAX_BLOCKS * 256 + 3             # a unit is 1, 2 or 4 words of ONE row, so units >= B: more than a pass for every shape
IFILL, FFILL = -77, -7.5                              # what the guard bands (and unwritten outputs) hold
I31 = (1 << 31) - 1
COLUMNS = ("answers", "images", "kb", "weights")


def tables(S_tab, seed=0, q=Q, image_rows=None):
    g = torch.Generator().manual_seed(seed + S_tab)
    lengths = torch.randint(0, S_tab + 1, (q,), generator=g, dtype=torch.int32)
    words = torch.randint(1, 90, (q, S_tab), generator=g, dtype=torch.int32) * (torch.arange(S_tab)[None] < lengths[:, None]).to(torch.int32)
    images = torch.randint(0, 40, (q,), generator=g, dtype=torch.int32) if image_rows is None else image_rows
    return dict(words=words, lengths=lengths, answers=torch.randint(0, 28, (q,), generator=g, dtype=torch.int32), images=images,
                kb=torch.randint(1, 197, (q,), generator=g, dtype=torch.int32), weights=torch.rand(q, generator=g) + 0.25)


def expected(t, ids, S, G=None):
    """the outputs of one call by the header's slot rules: {name: tensor}; a column whose table is None is absent, except the weights"""
    q, S_tab = t["words"].shape
    ids = ids.long()
    B = ids.shape[0]
    live = (ids >= 0) & (ids < q)
    dead = ids == -1
    poison = ~live & ~dead
    row = live | (dead & live[0])                                          # slots that copy a question's row
    src = torch.where(live, ids, torch.where(row, ids[0], torch.zeros_like(ids)))
    out = {"questions": torch.zeros(B, S, dtype=torch.int32)}
    out["questions"][row, :S_tab] = t["words"][src[row]]
    pick = lambda col, pad, bad: torch.where(row, col[src], torch.where(poison, torch.tensor(bad), torch.tensor(pad))).to(torch.int32)
    out["lengths"] = pick(t["lengths"], 0, 0)
    if t["answers"] is not None:
        out["answers"] = pick(t["answers"], 0, -1)
    if t["images"] is not None:
        out["images"] = pick(t["images"], 0, -1)
    if t["kb"] is not None:
        out["kb"] = pick(t["kb"], 1, 1)
    w = torch.ones(q) if t["weights"] is None else t["weights"]
    out["weights"] = torch.where(live, w[src], torch.where(poison, torch.tensor(1.0), torch.tensor(0.0)))
    out["bad"] = int(poison.any())
    if G is not None:
        rows, index = [], []
        for b in range(B):
            if live[b]:
                r = int(t["images"][ids[b]])
                if r not in rows:
                    rows.append(r)
                index.append(rows.index(r) if rows.index(r) < G else -1)
            else:
                index.append(0 if dead[b] else -1)
        out["bad"] |= int(len(rows) > G)
        first = rows[0] if rows else 0
        out["images"] = torch.tensor((rows + [first] * G)[:G], dtype=torch.int32)
        out["index"] = torch.tensor(index, dtype=torch.int32)
    return out


class Call:
    """one call on guarded outputs: .rc, .out {name: CPU tensor}, .bad (the word afterwards), .intact()"""

    def __init__(self, macx, dev, t, ids, S, outputs=COLUMNS, G=None, bad=0, shift=0):
        q, S_tab = t["words"].shape
        B = ids.shape[0]
        self.dt = {k: (None if v is None else v.to(dev)) for k, v in t.items()}
        self.ids = ids.to(torch.int32).to(dev)
        sizes = {"questions": B * S + shift, "lengths": B, "answers": B, "images": B if G is None else G, "kb": B, "weights": B, "index": B}
        want = ("questions", "lengths") + tuple(outputs) + (("index",) if G is not None else ())
        self.g = {n: Guarded(sizes[n], dev, dtype=torch.float32 if n == "weights" else torch.int32, fill=FFILL if n == "weights" else IFILL)
                  for n in want}
        self.word = torch.full((1,), bad, dtype=torch.int32, device=dev)
        p = lambda n: ptr(self.g[n].view) if n in self.g else None
        questions = self.g["questions"].view[shift:]                     # shift > 0: a pointer off the vector boundary
        self.rc = macx._lib.lib().macx_questions_gather(
            ptr(self.dt["words"]), ptr(self.dt["lengths"]), ptr(self.dt["answers"]), ptr(self.dt["images"]), ptr(self.dt["kb"]),
            ptr(self.dt["weights"]), q, S_tab, ptr(self.ids), B, S, ptr(questions), p("lengths"), p("answers"), p("images"), p("kb"),
            p("weights"), p("index"), 0 if G is None else G, ptr(self.word), None)
        torch.cuda.synchronize()
        self.out = {n: g.view.cpu() for n, g in self.g.items()}
        self.out["questions"] = self.out["questions"][shift:].view(B, S)
        self.bad = int(self.word)

    def intact(self):
        return all(g.intact() for g in self.g.values())

    def untouched(self):
        return all(g.untouched() for g in self.g.values())

    def matches(self, want):
        return [n for n in self.out if not bits_equal(self.out[n], want[n])]


def batch_ids(B, slot0_dead, seed=1):
    """repeats, the last row, a dead slot in the middle and at the end (B >= 5), slot 0 dead or not"""
    ids = torch.randint(0, Q, (B,), generator=torch.Generator().manual_seed(seed + B), dtype=torch.int32)
    if B >= 5:
        ids[1], ids[3] = ids[0], ids[0]
        ids[B // 2], ids[-1] = -1, -1
    ids[B // 3] = Q - 1
    if slot0_dead:
        ids[0] = -1
    return ids


def without(t, variant):
    if variant == "every column":
        return t, COLUMNS
    if variant == "no weight table":                                       # the one output that needs no table: ones
        return dict(t, weights=None), COLUMNS
    return dict(t, answers=None, images=None, kb=None, weights=None), ()     # "no optional column"


@pytest.mark.parametrize("variant", ["every column", "no weight table", "no optional column"])
@pytest.mark.parametrize("slot0_dead", [False, True], ids=["slot 0 live", "slot 0 dead"])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d" % s)
def test_gather_is_indexing(macx, dev, shape, B, slot0_dead, variant):
    S_tab, S = shape
    t, outputs = without(tables(S_tab), variant)
    ids = batch_ids(B, slot0_dead)
    want = expected(t, ids, S)
    a, b = Call(macx, dev, t, ids, S, outputs), Call(macx, dev, t, ids, S, outputs)
    assert a.rc == 0 and b.rc == 0
    assert set(a.out) == {"questions", "lengths"} | set(outputs)
    assert a.matches(want) == [] and a.intact() and a.bad == 0
    assert all(bits_equal(a.out[n], b.out[n]) for n in a.out)             # identical calls, identical bits
    if slot0_dead:                                                         # the pad question in every dead slot
        assert not a.out["questions"][ids == -1].any() and not a.out["lengths"][ids == -1].any()
    if variant == "every column" and B >= 5:
        dead = ids == -1
        assert bits_equal(a.out["weights"][dead], torch.zeros(int(dead.sum())))       # +0.0f
        if not slot0_dead:                                                 # slot 0's question in the dead slots
            assert bool((a.out["questions"][dead] == a.out["questions"][0]).all()) and bool((a.out["images"][dead] == a.out["images"][0]).all())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d" % s)
def test_a_batch_behind_one_grid_pass(macx, dev, shape):
    S_tab, S = shape
    t = tables(S_tab)
    ids = batch_ids(B_BEHIND_A_PASS, False)
    ids[-2] = Q                                                            # ... and the poison's store from the last pass
    got = Call(macx, dev, t, ids, S)
    assert got.rc == 0 and got.matches(expected(t, ids, S)) == [] and got.intact() and got.bad == 1


OUTSIDE = {"-2": [-2], "Q": [Q], "2^31-1": [I31], "-2^31": [-I31 - 1], "together": [-2, Q, I31, -I31 - 1]}


@pytest.mark.parametrize("values", list(OUTSIDE))
@pytest.mark.parametrize("shape", [(1, 1), (6, 8), (8, 12)], ids=lambda s: "%dto%d" % s)
def test_ids_outside_the_store_are_poisoned_never_read(macx, dev, shape, values):
    S_tab, S = shape
    t = tables(S_tab)
    ids = batch_ids(64, False)
    where = [7, 20, 41, 63][:len(OUTSIDE[values])]
    ids[where] = torch.tensor(OUTSIDE[values], dtype=torch.int32)
    want = expected(t, ids, S)
    got = Call(macx, dev, t, ids, S)
    assert got.rc == 0 and got.matches(want) == [] and got.intact() and got.bad == 1
    for n, poison in (("lengths", 0), ("answers", -1), ("images", -1), ("kb", 1)):      # the header's values, spelt out
        assert got.out[n][where].tolist() == [poison] * len(where), n
    assert got.out["weights"][where].tolist() == [1.0] * len(where) and not got.out["questions"][where].any()
    # slot 0 outside the store: the dead slots take the pad question, not its row
    ids0 = batch_ids(64, False)
    ids0[0] = OUTSIDE[values][-1]
    got0 = Call(macx, dev, t, ids0, S)
    assert got0.rc == 0 and got0.matches(expected(t, ids0, S)) == [] and got0.bad == 1
    assert got0.out["answers"][[0, 32, 63]].tolist() == [-1, 0, 0] and got0.out["kb"][[0, 32, 63]].tolist() == [1, 1, 1]


def test_the_bad_word_is_set_never_cleared(macx, dev):
    t, ids = tables(6), batch_ids(64, False)
    assert Call(macx, dev, t, ids, 8, bad=0).bad == 0                      # an all-valid call leaves it alone
    assert Call(macx, dev, t, ids, 8, bad=1).bad == 1                      # ... whatever it holds
    ids[5] = Q
    assert Call(macx, dev, t, ids, 8, bad=0).bad == 1


@pytest.mark.parametrize("shape,shift", [((4, 4), 1), ((4, 4), 2), ((8, 12), 3), ((6, 8), 1)], ids=str)
def test_a_pointer_off_the_vector_boundary_takes_a_narrower_path(macx, dev, shape, shift):
    """`questions` 4, 8 or 12 bytes behind a 16-byte boundary: not refused, and exact"""
    S_tab, S = shape
    t, ids = tables(S_tab), batch_ids(64, False)
    got = Call(macx, dev, t, ids, S, shift=shift)
    assert got.rc == 0 and got.matches(expected(t, ids, S)) == [] and got.intact()
    assert bool((got.g["questions"].view[:shift] == IFILL).all())          # the words in front of the shifted pointer


# ---- grouping ----------------------------------------------------------------------------------------------------------------------
ROWS = torch.tensor([7, 5, 2, 5, 0, 2, 1, 7, 3], dtype=torch.int32)           # the image row of each of the 9 questions
GROUPS = {
    # ids -> their rows [5, 5, 2, 5, 2, 7, dead, dead]
    "three of three": ([1, 3, 2, 1, 5, 0, -1, -1], [5, 2, 7], [0, 0, 1, 0, 1, 2, 0, 0], 0),
    # rows [5, 2, 5, 5, 2, 2, dead, 5]: the third image slot is a copy of the first
    "two of three": ([1, 2, 3, 1, 5, 5, -1, 3], [5, 2, 5], [0, 1, 0, 0, 1, 1, 0, 0], 0),
    # rows [5, 2, 7, 0, 5, 0, 7, 2]: the fourth distinct row does not fit
    "four of three": ([1, 2, 0, 4, 3, 4, 7, 5], [5, 2, 7], [0, 1, 2, -1, 0, -1, 2, 1], 1),
    # slot 0 dead, an id outside the store: group 0 is the first LIVE slot's row; the outsider joins no group
    "slot 0 dead": ([-1, 6, Q, 6, 8, -1, 2, 8], [1, 3, 2], [0, 0, -1, 0, 1, 0, 2, 1], 1),
    "no live slot": ([-1] * 8, [0, 0, 0], [0] * 8, 0),
}


@pytest.mark.parametrize("case", list(GROUPS))
def test_grouping_numbers_images_by_first_appearance(macx, dev, case):
    ids, image_ids, index, bad = GROUPS[case]
    ids = torch.tensor(ids, dtype=torch.int32)
    t = tables(6, image_rows=ROWS)
    want = expected(t, ids, 8, G=3)
    assert want["images"].tolist() == image_ids and want["index"].tolist() == index and want["bad"] == bad      # (the reference itself)
    a, b = Call(macx, dev, t, ids, 8, G=3), Call(macx, dev, t, ids, 8, G=3)
    assert a.rc == 0 and a.matches(want) == [] and a.intact() and a.bad == bad
    assert a.out["images"].tolist() == image_ids and a.out["index"].tolist() == index
    assert all(bits_equal(a.out[n], b.out[n]) for n in a.out)
    # G = 1: everything but the first row overflows; G = 8: five spare image slots
    for G in (1, 8):
        got = Call(macx, dev, t, ids, 8, G=G)
        assert got.rc == 0 and got.matches(expected(t, ids, 8, G=G)) == [] and got.intact(), G


def test_grouping_at_the_largest_batch(macx, dev):
    """B = 1024 over 2 000 questions about 300 images: a few hundred groups, repeats far apart, dead slots and one outsider"""
    q, B, G = 2000, 1024, 300
    g = torch.Generator().manual_seed(5)
    t = tables(6, q=q, image_rows=torch.randint(0, 300, (q,), generator=g, dtype=torch.int32))
    ids = torch.randint(0, q, (B,), generator=g, dtype=torch.int32)
    ids[1000:] = -1
    ids[517] = q
    want = expected(t, ids, 8, G=G)
    assert 250 < int(want["index"].max()) < G - 1 and want["bad"] == 1     # (image slots are left over: the padding rule runs)
    got = Call(macx, dev, t, ids, 8, G=G)
    assert got.rc == 0 and got.matches(want) == [] and got.intact() and got.bad == 1
    few = Call(macx, dev, t, ids, 8, G=100)                                # ... and the overflow at this size
    assert few.rc == 0 and few.matches(expected(t, ids, 8, G=100)) == [] and few.intact() and few.bad == 1


def test_grouping_refuses_more_than_1024_questions(macx, dev):
    t = tables(6, image_rows=ROWS)
    got = Call(macx, dev, t, torch.zeros(1025, dtype=torch.int32), 8, G=3)
    assert got.rc == macx._lib.MACX_EINVAL and got.untouched() and got.bad == 0
    assert Call(macx, dev, t, torch.zeros(1025, dtype=torch.int32), 8).rc == 0          # (without grouping any B is taken)


# ---- macx_preds_scatter ------------------------------------------------------------------------------------------------------------
def scatter(macx, dev, pred, ids, q=Q):
    table = Guarded(q, dev, dtype=torch.int32, fill=IFILL)
    table.view.fill_(-7)
    dpred, dids = torch.tensor(pred, dtype=torch.int32, device=dev), torch.tensor(ids, dtype=torch.int32, device=dev)     # (kept alive)
    rc = macx._lib.lib().macx_preds_scatter(ptr(dpred), ptr(dids), len(ids), q, ptr(table.view), None)
    torch.cuda.synchronize()
    assert rc == 0 and table.intact()
    return table.view.cpu().tolist()


def test_scatter_places_predictions_by_id(macx, dev):
    assert scatter(macx, dev, [10, 11, 12, 13], [4, 0, 8, 2]) == [11, -7, 13, -7, 10, -7, -7, -7, 12]
    # dead and outside slots write nothing
    assert scatter(macx, dev, [10, 11, 12, 13, 14, 15, 16], [4, -1, Q, 2, -2, I31, -I31 - 1]) == [-7, -7, 13, -7, 10, -7, -7, -7, -7]
    # a repeated id takes the highest slot's value
    assert scatter(macx, dev, [10, 11, 12, 13, 14], [3, 5, 3, 5, 3]) == [-7, -7, -7, 14, -7, 13, -7, -7, -7]


def test_scatter_duplicates_across_workgroups(macx, dev):
    """B = 3 000 over 700 ids: every id many times, in slots of different workgroups; the highest slot's value is the one stored"""
    B, q = 3000, 700
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(-1, q, (B,), generator=g)
    pred = torch.arange(B) + 100
    want = torch.full((q,), -7)
    for b in range(B):
        if ids[b] >= 0:
            want[ids[b]] = pred[b]
    assert scatter(macx, dev, pred.tolist(), ids.tolist(), q) == want.tolist()
