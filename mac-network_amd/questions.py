"""Questions resident in device memory: `QuestionStore` holds a question set as per-question tables (word ids [count, S], lengths,
and optionally answers, image rows of a macx.FeatureStore, knowledge-base sizes, weights), validated ONCE on the host, and a batch
names its questions by id.  One launch (macx_questions_gather) fills every per-question input of a step from a [B] id vector read
when the kernel runs, so a captured graph follows ids rewritten between replays; `EpochOrder` deals an epoch's ids out batch by batch.

    qs = macx.QuestionStore(questions, lengths, answers, image_rows=rows, device="cuda:0")       # 700 000 x 50 int32: 140 MB
    fwd = macx.CapturedTowerForward(net, B=64, S=50, features=store, questions=qs, score=True, predictions=qs.predictions())
    order = macx.EpochOrder(qs, 64)
    for _ in range(order.steps):
        fwd.next_batch(order); fwd.replay()
    qs.check(); result = fwd.totals.read()              # two synchronisations per epoch

Slot rules (include/macx.h): an id of -1 is a DEAD slot (slot 0's question under weight 0: a short last batch), any other id outside
[0, count) is never dereferenced and poisons its question (NaN loss, NaN image block) and sets the store's `bad` word: check()."""
import collections

import numpy as np
import torch

from . import _lib, generic
from .features import INT_DTYPES

MAX_GROUP_BATCH = 1024                  # macx_questions_gather's grouping holds the batch in one workgroup's LDS

QuestionBatch = collections.namedtuple("QuestionBatch", "questions lengths answers image_ids kb_lengths weights image_index")


def _host_column(t, name, count, floating=False):
    """a column argument as a contiguous host tensor: [count] (the questions themselves: [count, S]), integer -> int64 for the range
    checks, floating -> float32"""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    elif isinstance(t, (list, tuple)):
        t = torch.as_tensor(t)
    if not torch.is_tensor(t):
        raise TypeError("QuestionStore: %s must be an array or a tensor, not %s" % (name, type(t).__name__))
    if floating:
        if not t.dtype.is_floating_point:
            raise TypeError("QuestionStore: %s must have a floating-point dtype, not %s" % (name, t.dtype))
    elif t.dtype not in INT_DTYPES:
        raise TypeError("QuestionStore: %s must have an integer dtype, not %s" % (name, t.dtype))
    if count is not None and tuple(t.shape) != (count,):
        raise ValueError("QuestionStore: %s must be [%d], one entry per question; got %s" % (name, count, list(t.shape)))
    return t.detach().cpu().to(torch.float32 if floating else torch.int64).contiguous()


class QuestionStore:
    """Attributes: count, S, device, nbytes; max_word, max_answer (None without answers); the column tensors `questions` [count, S],
    `lengths`, `answers`, `image_rows`, `kb_lengths` (int32) and `weights` (float32), None where not given; `bad`, a 1-element int32
    word that a gather sets when it meets an id outside [0, count) other than -1, or more distinct images than a grouped batch has
    room for."""

    def __init__(self, questions, lengths, answers=None, image_rows=None, kb_lengths=None, weights=None, device="cuda"):
        q = _host_column(questions, "questions", None)
        if q.dim() != 2 or q.shape[0] < 1 or q.shape[1] < 1:
            raise ValueError("QuestionStore: questions must be [count, S] word ids with count, S >= 1; got %s" % list(q.shape))
        count, S = int(q.shape[0]), int(q.shape[1])
        if count >= 1 << 31:
            raise ValueError("QuestionStore: count must lie in [1, 2^31), got %d" % count)
        if int(q.min()) < 0:
            raise ValueError("QuestionStore: word ids must be >= 0 (0 is the pad id), got %d" % int(q.min()))
        cols = {"questions": q, "lengths": _host_column(lengths, "lengths", count)}
        if int(cols["lengths"].min()) < 0 or int(cols["lengths"].max()) > S:
            raise ValueError("QuestionStore: lengths must lie in [0, %d], got %d .. %d"
                             % (S, int(cols["lengths"].min()), int(cols["lengths"].max())))
        for name, t, low in (("answers", answers, 0), ("image_rows", image_rows, 0), ("kb_lengths", kb_lengths, 1)):
            cols[name] = None if t is None else _host_column(t, name, count)
            if t is not None and int(cols[name].min()) < low:
                raise ValueError("QuestionStore: %s must be >= %d, got %d" % (name, low, int(cols[name].min())))
        for name, t in cols.items():
            if t is not None and int(t.max()) >= 1 << 31:
                raise ValueError("QuestionStore: %s does not fit int32 (maximum %d)" % (name, int(t.max())))
        cols["weights"] = None if weights is None else _host_column(weights, "weights", count, floating=True)
        if weights is not None and not bool(torch.isfinite(cols["weights"]).all()):
            raise ValueError("QuestionStore: weights must be finite")
        self.count, self.S = count, S
        self.max_word = int(q.max())
        self.max_answer = None if answers is None else int(cols["answers"].max())
        self.device = torch.device(device)
        for name, t in cols.items():
            setattr(self, name, None if t is None else t.to(torch.float32 if name == "weights" else torch.int32).to(self.device))
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _columns(self):
        return [t for t in (self.questions, self.lengths, self.answers, self.image_rows, self.kb_lengths, self.weights) if t is not None]

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._columns())

    def __repr__(self):
        have = [n for n in ("answers", "image_rows", "kb_lengths", "weights") if getattr(self, n) is not None]
        return "<macx.QuestionStore %d x %d on %s, %.1f MB%s>" % (self.count, self.S, self.device, self.nbytes / 1e6,
                                                                  "; " + ", ".join(have) if have else "")

    def check(self):
        """Reads the `bad` word (one synchronisation): ValueError if a gather so far has seen a question id outside [0, count) other
        than -1, or a grouped batch has named more distinct images than it has room for."""
        if int(self.bad.item()):
            raise ValueError("QuestionStore: a gathered batch named a question id outside [0, %d) (other than -1, a dead slot), or a "
                             "grouped batch named more distinct images than images=G; those questions were poisoned (NaN)" % self.count)
        return self

    def reset_bad(self):
        self.bad.zero_()
        return self

    def check_ids(self, ids, count=None, host_check=False, what="question ids"):
        """The validation of an id vector ([count] integer tensor), done before anything asks for the device.  host_check: also
        0 <= ids < count-of-the-store on the host (synchronises), IndexError."""
        if not torch.is_tensor(ids) or ids.dim() != 1 or (count is not None and ids.shape[0] != count):
            raise ValueError("%s must be a [%s] tensor, one question of the store per slot; got %s"
                             % (what, "B" if count is None else count, tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__))
        if ids.dtype not in INT_DTYPES:
            raise ValueError("%s must have an integer dtype, not %s" % (what, ids.dtype))
        if host_check and ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.count:
                raise IndexError("%s outside [0, %d)" % (what, self.count))
        return ids

    def gather_into(self, ids, questions, lengths, answers=None, image_ids=None, kb_lengths=None, weights=None, image_index=None):
        """The one launch, no allocation (what the captured graphs record): slot b of every given output <- question ids[b].  ids: [B]
        int32, contiguous, on the device; questions [B, S' >= S] and lengths [B] int32; the others None or [B] (weights: float32).
        image_index: grouping -- image_ids is then [G] and receives the batch's distinct image rows (include/macx.h)."""
        B, G = ids.shape[0], 0 if image_index is None else image_ids.shape[0]
        _lib.check(_lib.lib().macx_questions_gather(
            _lib.ptr(self.questions), _lib.ptr(self.lengths), _lib.ptr(self.answers), _lib.ptr(self.image_rows), _lib.ptr(self.kb_lengths),
            _lib.ptr(self.weights), self.count, self.S, _lib.ptr(ids), B, questions.shape[1], _lib.ptr(questions), _lib.ptr(lengths),
            _lib.ptr(answers), _lib.ptr(image_ids), _lib.ptr(kb_lengths), _lib.ptr(weights), _lib.ptr(image_index), G, _lib.ptr(self.bad),
            _lib.stream_of(questions)), "macx_questions_gather")

    def gather(self, ids, S=None, images=None):
        """The eager route: a QuestionBatch (questions [B, S], lengths, answers, image_ids, kb_lengths, weights, image_index) of new
        tensors from one launch; a column the store does not hold is None, weights are ones without a table.  S: the batch's width
        (default the store's; wider: pad ids behind).  images=G: grouping -- image_ids is [G], image_index [B]."""
        self.check_ids(ids)
        S = self.S if S is None else int(S)
        if S < self.S:
            raise ValueError("QuestionStore.gather: S = %d is narrower than the store's %d" % (S, self.S))
        if images is not None:
            if self.image_rows is None:
                raise ValueError("QuestionStore.gather(images=G) groups by image row: the store holds no image_rows")
            if int(images) < 1 or ids.shape[0] > MAX_GROUP_BATCH:
                raise ValueError("QuestionStore.gather(images=G): G >= 1 and at most %d questions; got G = %r, B = %d"
                                 % (MAX_GROUP_BATCH, images, ids.shape[0]))
        generic._require_device(ids, "question ids")
        generic._require_device(self.questions, "the question store")
        if ids.dtype != torch.int32 or not ids.is_contiguous():
            ids = ids.to(torch.int32).contiguous()
        B, dev = ids.shape[0], self.device
        new = lambda have, n=B, dtype=torch.int32: torch.empty(n, dtype=dtype, device=dev) if have else None
        out = QuestionBatch(torch.empty(B, S, dtype=torch.int32, device=dev), new(True), new(self.answers is not None),
                            new(self.image_rows is not None, B if images is None else int(images)), new(self.kb_lengths is not None),
                            new(True, dtype=torch.float32), new(images is not None))
        self.gather_into(ids, *out)
        return out

    def predictions(self):
        """a new [count] int32 table of -1: the predictions of a whole set, filled batch by batch (scatter_predictions)"""
        return torch.full((self.count,), -1, dtype=torch.int32, device=self.device)

    def scatter_predictions(self, table, pred, ids):
        """table[ids[b]] = pred[b] for the live slots (one launch, no allocation; of a repeated id the highest slot wins)"""
        _lib.check(_lib.lib().macx_preds_scatter(_lib.ptr(pred), _lib.ptr(ids), ids.shape[0], self.count, _lib.ptr(table),
                                                 _lib.stream_of(table)), "macx_preds_scatter")
        return table


class EpochOrder:
    """The order in which an epoch visits a store's questions, on the store's device: `order` [count] int32 (None: 0 .. count-1; or a
    permutation, uploaded once per epoch -- the shuffle is the caller's), the host position `position` and `steps` = ceil(count / B).
    A batch is a device-to-device slice of the order: take() returns the next one, the captured classes' next_batch() copies it into
    their static question_ids.  Plain torch."""

    def __init__(self, store, B, order=None):
        if not isinstance(store, QuestionStore):
            raise TypeError("EpochOrder takes a macx.QuestionStore, not %s" % type(store).__name__)
        if int(B) < 1:
            raise ValueError("EpochOrder: B must be at least 1, got %r" % (B,))
        self.store, self.B = store, int(B)
        self.count = store.count
        self.steps = -(-self.count // self.B)
        self.rewind(order)

    def rewind(self, order=None):
        """start a new epoch: position 0 and, if given, a new order ([count] integer tensor; a host tensor is range-checked)"""
        if order is not None:
            self.store.check_ids(order, self.count, host_check=torch.is_tensor(order) and not order.is_cuda, what="order")
            self.order = order.to(device=self.store.device, dtype=torch.int32).contiguous()
        elif not getattr(self, "_identity", False):          # (an identity order is kept across epochs)
            self.order = torch.arange(self.count, dtype=torch.int32, device=self.store.device)
        self._identity = order is None
        self.position = 0
        return self

    @property
    def remaining(self):
        return self.count - self.position

    def take(self):
        """the next min(B, remaining) ids as a view of the order; advances.  IndexError when the epoch is exhausted."""
        if self.position >= self.count:
            raise IndexError("EpochOrder: the epoch's %d questions are exhausted (%d steps of %d): rewind()" % (self.count, self.steps, self.B))
        n = min(self.B, self.count - self.position)
        ids = self.order[self.position:self.position + n]
        self.position += n
        return ids
