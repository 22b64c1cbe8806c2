"""Evaluation records resident in device memory: `EvalRecords` holds, per question of a macx.QuestionStore, the attention maps and the
logits of the run that evaluated it -- the reference's --getPreds / --getAtt output (model.py:693-710 buildPredsList, what
visualization.py draws) -- as device tables filed by question id.  One launch (macx_records_scatter) files a batch into every
table; it reads the [B] id vector when the kernel runs, so a captured graph follows ids rewritten between replays and an evaluation
epoch stays a loop of replays:

    rec = macx.EvalRecords(qs, p=12, N=196, S=50, answers=28, maps=("kb", "question"), logits=True, dtype=torch.float16)
    fwd = macx.CapturedTowerForward(net, B=64, S=50, features=store, questions=qs, score=True, predictions=qs.predictions(), records=rec)
    order = macx.EpochOrder(qs, 64)
    for _ in range(order.steps):
        fwd.next_batch(order); fwd.replay()
    qs.check(); result = fwd.totals.read(); maps = rec.read()         # three synchronisations per epoch
    preds = rec.instances(instances, ids, predictions=fwd.predictions, decode=answerDict.decodeId)

Slot rules (include/macx.h): only 0 <= id < count files; a dead slot (-1) and any other id write nothing; of a repeated id the highest
slot's rows are kept.  A question never filed reads NaN, as a prediction never made reads -1.  The gate is out of scope (it is as
wide as the state, and a zero-padded cell crops it to a strided view)."""
import numpy as np
import torch

from . import _lib, generic
from .questions import QuestionStore

MAPS = {"kb": "att_kb", "question": "att_question", "self": "att_self"}        # table name -> MACCell.state_tensor's name
ARGUMENTS = {"kb": "kb", "question": "question", "self": "self_att", "logits": "logits"}     # table name -> file()'s keyword


class EvalRecords:
    """Attributes: store, count, p, N, S, answers, dtype, device; `tables`: name -> device tensor, "kb" [count, p, N],
    "question" [count, p, S], "self" [count, p, p] (a cell with writeSelfAtt only) in `dtype` (torch.float16 | torch.float32) and
    "logits" [count, 1, answers], always float32 (an fp16 logit could disagree with the filed argmax); `nbytes`."""

    def __init__(self, store, p, N, S, answers=None, maps=("kb", "question"), logits=True, dtype=torch.float16):
        if not isinstance(store, QuestionStore):
            raise TypeError("EvalRecords takes a macx.QuestionStore, not %s" % type(store).__name__)
        for name, v in (("p", p), ("N", N), ("S", S)):
            if int(v) < 1:
                raise ValueError("EvalRecords: %s must be at least 1, got %r" % (name, v))
        if dtype not in _lib.FEATURES_DTYPE:
            raise ValueError("EvalRecords: dtype is torch.float16 or torch.float32, not %r" % (dtype,))
        maps = (maps,) if isinstance(maps, str) else tuple(maps)
        for m in maps:
            if m not in MAPS:
                raise ValueError("EvalRecords: no attention map %r (have %s; the gate is out of scope)" % (m, ", ".join(MAPS)))
        if len(set(maps)) != len(maps):
            raise ValueError("EvalRecords: maps names a map twice: %r" % (maps,))
        if logits and (answers is None or int(answers) < 1):
            raise ValueError("EvalRecords(logits=True) needs answers, the classifier's answer count (at least 1), got %r" % (answers,))
        if not maps and not logits:
            raise ValueError("EvalRecords: nothing to record (no maps and logits=False)")
        self.store, self.count, self.device, self.dtype = store, store.count, store.questions.device, dtype      # (cuda -> cuda:0)
        self.p, self.N, self.S = int(p), int(N), int(S)
        self.answers = int(answers) if logits else None
        widths = {"kb": self.N, "question": self.S, "self": self.p}
        self.tables = {m: torch.empty(self.count, self.p, widths[m], dtype=dtype, device=self.device) for m in MAPS if m in maps}
        if logits:
            self.tables["logits"] = torch.empty(self.count, 1, self.answers, dtype=torch.float32, device=self.device)
        assert len(self.tables) <= _lib.RECORDS_MAX
        self.clear()

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tables.values())

    def __repr__(self):
        return "<macx.EvalRecords of %d questions on %s, %.1f MB: %s>" % (
            self.count, self.device, self.nbytes / 1e6,
            ", ".join("%s %s %s" % (k, list(t.shape[1:]), str(t.dtype).split(".")[-1]) for k, t in self.tables.items()))

    def clear(self):
        """every table back to quiet NaN: nothing filed"""
        for t in self.tables.values():
            t.fill_(float("nan"))
        return self

    # ---- filing
    def _source(self, name, t, B):
        steps, n = self.tables[name].shape[1:]
        want = (B, n) if name == "logits" else (steps, B, n)
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != want or not t.is_contiguous()
                or t.device != self.tables[name].device):
            raise ValueError("EvalRecords.file: %s must be a contiguous float32 %s tensor on %s, got %s"
                             % (ARGUMENTS[name], list(want), self.device,
                                "%s %s on %s" % (t.dtype, list(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
        return t

    def file(self, ids, kb=None, question=None, self_att=None, logits=None):
        """ONE launch, no allocation (what the captured graph records): the rows of every table <- the given tensors, by ids [B]
        (int32, contiguous, on the device; another integer dtype is converted first).  kb [p, B, N], question [p, B, S], self_att
        [p, B, p]: contiguous float32 on the device, step-major as a run's `saved` holds them; logits [B, answers].  A table
        without its tensor, or a tensor without its table, is a ValueError."""
        self.store.check_ids(ids)
        given = {"kb": kb, "question": question, "self": self_att, "logits": logits}
        for name, t in given.items():
            if (t is None) != (name not in self.tables):
                raise ValueError("EvalRecords.file: %s" % (
                    "the records hold a %r table and no %s= was given" % (name, ARGUMENTS[name]) if t is None
                    else "%s= was given and the records hold no %r table" % (ARGUMENTS[name], name)))
        B = int(ids.shape[0])
        if B < 1:
            raise ValueError("EvalRecords.file: ids names no slot")
        srcs = [(name, self._source(name, given[name], B)) for name in self.tables]
        generic._require_device(ids, "question ids")
        generic._require_device(next(iter(self.tables.values())), "the evaluation records")
        if ids.dtype != torch.int32 or not ids.is_contiguous():
            ids = ids.to(torch.int32).contiguous()
        descs = (_lib.MacxRecordDesc * len(srcs))()
        for d, (name, t) in zip(descs, srcs):
            table = self.tables[name]
            d.src, d.table, d.steps, d.n, d.dtype = t.data_ptr(), table.data_ptr(), table.shape[1], table.shape[2], _lib.FEATURES_DTYPE[table.dtype]
        _lib.check(_lib.lib().macx_records_scatter(descs, len(srcs), _lib.ptr(ids), B, self.count, _lib.stream_of(ids)),
                   "macx_records_scatter")
        return self

    def file_run(self, ids, cell, logits=None):
        """file() with the maps of a run: cell.state_tensor("att_kb" | "att_question" | "att_self") of the fused cell (MACCell, or
        net.last_cell after any eager MACNet / MACNetCore forward), detached."""
        maps = {}
        for name in self.tables:
            if name != "logits":
                try:
                    maps[ARGUMENTS[name]] = cell.state_tensor(MAPS[name]).detach()
                except KeyError as e:
                    raise ValueError("EvalRecords.file_run: the records hold a %r table and the cell's run has no %s: %s"
                                     % (name, MAPS[name], e.args[0])) from None
        return self.file(ids, logits=None if logits is None else logits.detach(), **maps)

    # ---- reading
    def _rows(self, ids):
        if ids is None:
            return None
        idx = torch.as_tensor(ids)
        if idx.dim() != 1 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise ValueError("EvalRecords: ids must be a 1-D integer tensor, array or list of question ids")
        idx = idx.long()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.count):
            raise IndexError("EvalRecords: question ids outside [0, %d)" % self.count)
        return idx

    def read(self, ids=None):
        """{table name: host array [len(ids) or count, steps, n] in the table's dtype}: the epoch-end read next to totals.read().
        One synchronisation: every table's rows are copied out asynchronously, then the stream is waited for once.
        "self": row i of the map has i + 1 entries (cell.attentions["self"]); the entries behind them are no part of it -- the run's
        buffer holds whatever was there, and so does the device table -- and come back as zeros, filed or not."""
        idx = self._rows(ids)
        out = {}
        for name, t in self.tables.items():
            rows = t if idx is None else t.index_select(0, idx.to(t.device))
            if t.is_cuda:
                host = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
                host.copy_(rows, non_blocking=True)
                rows = host
            out[name] = rows
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        out = {name: rows.numpy().copy() for name, rows in out.items()}
        if "self" in out:
            out["self"] = np.tril(out["self"])
        return out

    def topk(self, k):
        """(indices [count, k] int64, probabilities [count, k] float32) of the logits table by torch.softmax / torch.topk, on the
        tables' device: once per epoch, off the hot path.  A question never filed has NaN probabilities."""
        if "logits" not in self.tables:
            raise ValueError("EvalRecords.topk: the records hold no logits table (logits=False)")
        if not 1 <= int(k) <= self.answers:
            raise ValueError("EvalRecords.topk: 1 <= k <= %d answers, got %r" % (self.answers, k))
        prob, index = torch.topk(torch.softmax(self.tables["logits"][:, 0, :], dim=-1), int(k), dim=-1)
        return index, prob

    def instances(self, instances, ids, predictions=None, decode=None, trim=True):
        """The reference's prediction records (model.py:693-710 buildPredsList): for instance j, question ids[j], a COPY of the
        instance dict plus "prediction" (predictions given: the store.predictions() table's entry, through `decode` --
        answerDict.decodeId -- or the integer) and "attentions": {"kb": [p lists], "question": [p lists], "self": ...}, every value
        a Python float.
        trim=True cuts a word-attention row to the question's own length and a kb row to its kb_length where the store holds that
        column -- what is cut is exact zeros -- and row i of "self" to i + 1 entries, as cell.attentions["self"] does.  (The
        reference cuts at the longest question of its batch, which depends on the batching and is not reproduced.)
        trim=False emits whole rows."""
        idx = self._rows(ids)
        instances = list(instances)
        if idx is None or len(instances) != idx.numel():
            raise ValueError("EvalRecords.instances: one question id per instance (%d instances, %s ids)"
                             % (len(instances), "no" if idx is None else idx.numel()))
        maps = {k: v for k, v in self.read(idx).items() if k != "logits"}
        pred = None
        if predictions is not None:
            pred = torch.as_tensor(predictions)
            if tuple(pred.shape) != (self.count,):
                raise ValueError("EvalRecords.instances: predictions is the store's [%d] table (store.predictions())" % self.count)
            pred = pred[idx.to(pred.device)].cpu().tolist()
        cut = {"question": self.store.lengths, "kb": self.store.kb_lengths}
        cut = {k: t[idx.to(t.device)].cpu().tolist() for k, t in cut.items() if trim and t is not None and k in maps}
        out = []
        for j, instance in enumerate(instances):
            record = dict(instance)
            if pred is not None:
                record["prediction"] = decode(pred[j]) if decode is not None else pred[j]
            att = {}
            for name, rows in maps.items():
                steps = rows[j].astype(np.float32) if rows.dtype != np.float32 else rows[j]
                if name in cut:
                    att[name] = [step[:cut[name][j]].tolist() for step in steps]
                elif name == "self" and trim:
                    att[name] = [step[:i + 1].tolist() for i, step in enumerate(steps)]
                else:
                    att[name] = [step.tolist() for step in steps]
            record["attentions"] = att
            out.append(record)
        return out
