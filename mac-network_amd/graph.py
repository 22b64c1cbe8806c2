"""Inference forward of the MAC cell replayed from ONE captured HIP graph.

Forward only at p = 4 (BASELINE.json configs[1]) is about 70 kernel launches of 5 - 80 us each: issued one ctypes call at a
time the host, not the GPU, sets the pace (3.2 ms per batch of 64 against 0.7 ms of kernel time).  The loop of
model.py:453-458 has no data-dependent control flow, every buffer is caller-owned and every launch goes to the stream the
caller passes, so the whole run is capturable: `CapturedForward` captures a `MACCell`'s `run()` once on static input / output
tensors and replays it per batch.

    fwd = macx.CapturedForward(cfg, params, B=64, S=50, N=196)
    memory = fwd(vecQuestions, questionCntxWords, questionLengths, knowledgeBase)       # [B, d], valid until the next call
    att_kb = fwd.attentions["kb"]                                                       # p x [B, N] views, refreshed by replay

Evaluation only (no dropout, nothing kept for a backward pass); parameters are read at replay time, so an optimizer step or
a checkpoint load between calls is seen.  Changing a parameter's storage (`.to()`, `.data = `) needs a new capture.

Knowledge bases of per-question size (MACCell's kb_lengths): every class here takes `kb_lengths=True`.  The lengths are device data
the attention kernel reads when it runs, so ONE graph serves every set of them: a static int32 [B] tensor `.kb_lengths` (all N) is
allocated with the other inputs, `load(..., kb_lengths=)` copies into it (required exactly when the class was built with it), or
write it directly.  The self-checks then draw lengths too (one N, one 1, the rest random).

    fwd = macx.CapturedForward(cfg, params, B=64, S=50, N=100, kb_lengths=True)
    memory = fwd(vecQuestions, questionCntxWords, questionLengths, knowledgeBase, kb_lengths=boxes)     # [B] integers in [1, N]

A capture checks itself before it is used (`verify=True`): three replays on random inputs must reproduce the eager run bit
for bit; a process whose replays do not falls back to eager launches (`captured` is False, a warning says so): slower where
the host is slow, never wrong.  The check exists because of a bug it would have caught.  Until the end of round 3 the
per-matrix maximum behind every packed weight's exponent was a 16-byte hipMemsetAsync followed by integer atomicMax, and in
about one process in ten (one in three for the smallest shapes) the replayed graph ran the two out of order from its second
replay on -- maximum 0, exponent 0, weights split at the wrong scale, results finite and 1e-2 off, deterministically for
that process, while eager launches of the same kernels stayed bit-identical.  Round 3 removed that one pair; round 4 found
the general rule behind it (tools/graph_train_probe_verify.py, profiles/r04_graph_train_verify_8_processes.txt): under
ROCm 7.2 a captured hipMemsetAsync / hipMemcpyAsync becomes a memset / memcpy NODE, and replay does not keep such nodes in
stream order with the kernel nodes around them.  The library therefore issues no memset or memcpy at all any more -- every
fill and copy on the step's path is a kernel (`dev_zero` / `dev_copy` / `dev_copy2d` in macx_api.hip) -- and reductions that
used to start from a memset write per-workgroup partials that a later kernel combines.
(What torch adds around the library inside a capture is not under its control: the two `.clone()`s of the final state are
device-to-device copy nodes.  They deliver `memory`, which the self-check compares on every verification replay, and they have
never been seen out of order -- but they are the reason the check stays on by default.)

Did a replay go wrong?  The captured run's `saved` buffer carries the sticky hand-off status of include/macx.h (macx_run_status):
every class here has `.check()` (raises macx.HandoffTimeout; SYNCHRONISES), `.reset_status()` and a constructor argument
`check_every=k`: with k > 0 every k-th replay() / step() ends in a check(); the default 0 adds nothing to a replay.  The reset is
never part of a graph -- the status survives replays until the caller clears it.

Six classes, one protocol, written once in `_Captured`: warm up on a side stream and capture (`_capture`), compare replays with
the eager run and fall back (`_self_check`, `_eager_on_captured`, `_compare_replays`), report the status.  A class adds its static
inputs (`_CellInputs`, `_TowerInputs`; the training classes' mask word: `_MaskWord`), `_eager()` -- its launches on the current
stream -- and `_issue()`, which publishes what they return: the body of the capture and the eager fallback of `replay()`.

Losses on the run's own attention maps and states (attention supervision, entropy regularisers, per-step heads): the three training
classes take `att_loss=dict(...)` -- one launch of the library (macx_att_loss) between the forward and the backward launches, its
target and weights static tensors read at replay time -- and, where autograd runs, `aux_loss=callable` (`_AttLoss`;
CapturedTrainStep documents both).

Per-question answer weights and partial batches (the tower's two classes): `CapturedTowerTrainStep(weights=True)` and
`CapturedTowerForward(score=True)` put macx_answer_loss_weighted in the place of macx_answer_loss -- a static [B] `weights` read when the
kernel runs, a weighted-mean loss, optional running totals (output.AnswerTotals) -- and their load() takes n <= B questions: the slots
behind them become copies of slot 0 with weight 0 (`_pad_slots`, `_TowerInputs._load_inputs`).  Built without, the classes issue the
launches of before and refuse a batch of any other size than B.  The cell-level classes are out of this: their caller owns d_memory.
Over several processes the weighted mean needs the weights summed over the ranks: `CapturedDPTowerTrainStep(weights=True)`, the tower's
step cut at its collectives (dp.TowerExchangeStep) into two or three graphs that replay the eager step's launches.
"""
import warnings

import torch

from .cell import MACCell, MACCellTuple, _Run
from .dp import TowerExchangeStep, TwoPhaseStep, live_weight_sum
from .options import UnsupportedOptions, get
from .params import MACCellParams
# (encoder, output and stem are imported where the tower's classes use them, not here.  No cycle: `from macx.graph import mix32`,
# the package under its alias, executes this module a second time, and an import at this level would make second copies of those
# modules too and bind them to the package's attributes.)


def mix32(x):
    """the 32-bit finaliser the dropout stream hashes with (macx_common.hip.h, hash_mix): iteration number -> mask word"""
    h = (x + 0x7F4A7C15) & 0xFFFFFFFF
    h = (h * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE3D) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _require_hip(dev, who, what):
    if dev.type != "cuda":
        raise RuntimeError("%s needs the HIP device: %s has no CPU path" % (who, what))
    return dev


class _Captured:
    """The protocol of the captured classes (module docstring): capture, self-check with the eager fallback behind it, and
    check() / reset_status() / check_every.  `_status_run()` is the cell._Run whose `saved` the replays write (None before the
    first run); `_WHAT` names the captured and the eager side in the fallback's warning."""
    check_every = 0
    _replays = 0
    captured = False
    mask_word = None                                 # (the training classes have one: _MaskWord)
    verify_report = ()                               # (replay, label) of everything the self-check saw differ
    _WHAT = ("step", "step")

    def _capture(self, dev, warmup, warm, graphs, before=None):
        """warm() `warmup` times on a side stream -- code objects, LDS attributes and the allocator settle outside the capture --
        then before() and one capture per (graph, body) of `graphs`, every later graph in the first one's pool"""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                warm()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if before is not None:
            before()
        pool = None
        for graph, body in graphs:
            with torch.cuda.graph(graph, pool=pool):
                body()
            pool = pool or graph.pool()
        self._after_capture()

    def _self_check(self, verify, *args):
        """use the capture unless `verify` and its replays do not reproduce the eager run (_replays_match_eager(*args))"""
        self._captured_cell = self.cell              # the run whose buffers the graph replays on
        self.captured = True
        try:
            matched = not verify or self._replays_match_eager(*args)
        finally:
            # the check drew a target and weights into the static att_loss= tensors: back to what a constructed step documents
            # (target zeros, weights ones), whether or not the replays matched -- load() does not force the weights
            getattr(self, "_reset_att_loss", lambda: None)()
        if not matched:
            self.captured = False
            warnings.warn("%s: replays of the captured %s do not reproduce the eager %s in this process; "
                          "falling back to eager launches" % ((type(self).__name__,) + self._WHAT), RuntimeWarning)

    def _eager_on_captured(self, leaves, reference):
        """reference(): an eager run on the static tensors, returning clones of what it wrote.  Afterwards the `.grad` tensors the
        graph writes (`leaves`: who has one) and `self.cell` are the captured ones again, so the next replay writes where it is
        looked at; a step that fell back to eager launches has nothing to put back.  Checks the eager run's status: synchronises."""
        captured_grads = [t.grad for t in leaves]
        want = reference()
        self.check()                                 # the eager run's own buffers
        if self.captured:
            self.cell = self._captured_cell
            for t, g in zip(leaves, captured_grads):
                t.grad = g
        return want

    def _compare_replays(self, replays, written, want, before=None, replay=None):
        """`replays` replays (before() in front of each): written() is the (label, tensor) list of what the graph wrote, `want` the
        eager run's clones of the same; (replay, label) of everything that differed goes to `verify_report`.  replay: what a class
        of several graphs replays in the place of self.graph"""
        self.verify_report = []
        for r in range(replays):
            if before is not None:
                before()
            (replay or self.graph.replay)()
            for (label, t), w in zip(written(), want):
                if not torch.equal(t, w):
                    self.verify_report.append((r, label))
        torch.cuda.synchronize(want[0].device)
        if self.mask_word is not None:
            self.set_mask_word(0)
        self.check()
        return not self.verify_report

    def _status_run(self):
        cell = getattr(self, "cell", None)
        cell = getattr(cell, "inner", cell)          # (a zero-padded cell wraps the real one)
        return getattr(cell, "_run", None)

    def _after_capture(self):
        """a run allocated under capture could not zero its status words (the reset must not become a graph node): do it now"""
        run = self._status_run()
        if run is not None and getattr(run, "status_reset_pending", False):
            run.reset_status()

    def status(self):
        run = self._status_run()
        return run.status() if run is not None else (0, -1)

    def check(self):
        """raises macx.HandoffTimeout if an in-launch hand-off of any replay since the last reset gave up.  Synchronises."""
        run = self._status_run()
        if run is not None:
            run.check(type(self).__name__)

    def reset_status(self):
        run = self._status_run()
        if run is not None:
            run.reset_status()

    def _count_replay(self):
        if self.check_every > 0:
            self._replays += 1
            if self._replays % self.check_every == 0:
                self.check()


class _MaskWord:
    """the device word of a captured training step, which every dropout site XORs into its key when the kernel runs"""

    def _alloc_mask_word(self, dev):
        self.mask_word = torch.zeros(1, dtype=torch.int32, device=dev)        # macx_dropout.mask_word of every run of this step

    def set_mask_word(self, word):
        """the raw 32-bit word the next replays XOR into every dropout key (0: the masks of the plain seed)"""
        word &= 0xFFFFFFFF
        self.mask_word.fill_(word - (1 << 32) if word >= (1 << 31) else word)

    def _set_iteration(self, iteration):
        """iteration: None keeps the current mask word; an int draws the masks of word mix32(iteration)"""
        if iteration is not None:
            self.set_mask_word(mix32(int(iteration)))


def _draw_lengths(gen, n, N):
    """n knowledge-base sizes for the self-checks: one N, one 1 (n > 1), the rest random in [1, N]"""
    L = torch.randint(1, N + 1, (n,), generator=gen, dtype=torch.int32)
    L[0] = N
    if n > 1:
        L[-1] = 1
    return L


def _check_lengths(t, n, N, check, name):
    """load()'s validation of a [n] tensor of knowledge-base sizes; check: also 1 <= size <= N on the host (synchronises)"""
    if not torch.is_tensor(t) or tuple(t.shape) != (n,) or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("%s must be a [%d] integer tensor" % (name, n))
    if check and n and (int(t.min()) < 1 or int(t.max()) > N):
        raise ValueError("%s must lie in [1, %d] (the knowledge base's cells); got %d .. %d" % (name, N, int(t.min()), int(t.max())))


def _pad_slots(buf, t, n, axis=0):
    """the padding rule of a short batch: along `axis` slots 0 .. n-1 of the static tensor `buf` become `t`, slots n .. copies of slot 0
    -- finite and in range whatever the batch holds, and the same launches for every n"""
    live, rest = buf.narrow(axis, 0, n), buf.narrow(axis, n, buf.shape[axis] - n)
    live.copy_(t)
    if rest.shape[axis]:
        rest.copy_(buf.narrow(axis, 0, 1).expand_as(rest))


def _lengths_argument(who, name, given, built, how=None):
    """load() takes `name` exactly when the class was built with it (as d_memory); how: the constructor argument that builds it"""
    if given != built:
        raise TypeError("%s.load() %s %s: the graph was captured %s %s"
                        % (who, "needs" if built else "takes no", name, "with" if built else "without", how or name + "=True"))


# ---------------------------------------------------------------------------------------------------------------------------
# a loss on the run's attention maps inside the captured step (att_loss=) and losses written in torch ops (aux_loss=)
# ---------------------------------------------------------------------------------------------------------------------------
_ATT_LOSS_KEYS = {"on": "kb", "kind": "ce", "weight": 1.0, "eps": 1e-8, "per_step_target": False}


def _att_loss_spec(who, spec):
    """att_loss=None | dict(on="kb" | "question", kind="ce" | "entropy", weight=lambda, eps=1e-8, per_step_target=False) -> the
    dict with every key, validated (before anything asks for the device)"""
    if spec is None:
        return None
    from .losses import check_scalars
    if not isinstance(spec, dict):
        raise TypeError("%s: att_loss is None or a dict(on=, kind=, weight=, eps=, per_step_target=), not %r" % (who, spec))
    unknown = sorted(set(spec) - set(_ATT_LOSS_KEYS))
    if unknown:
        raise ValueError("%s: att_loss has no key %s (have %s)" % (who, ", ".join(map(repr, unknown)), ", ".join(sorted(_ATT_LOSS_KEYS))))
    out = dict(_ATT_LOSS_KEYS, **spec)
    if out["on"] not in ("kb", "question"):
        raise ValueError('%s: att_loss on=%r: the supervised map is "kb" or "question" (the self-attention and the gate are reached '
                         "through aux_loss= and cell.state_tensor)" % (who, out["on"]))
    _, out["eps"], out["weight"] = check_scalars(out["kind"], out["eps"], out["weight"])
    out["per_step_target"] = bool(out["per_step_target"])
    if out["per_step_target"] and out["kind"] != "ce":
        raise ValueError('%s: att_loss per_step_target=True belongs to kind "ce": kind "entropy" has no target' % who)
    return out


class _AttLoss:
    """What the three captured training steps share for att_loss= / aux_loss=: the static tensors (allocated with the other inputs,
    BEFORE the capture: DESIGN 8), load() into them, the draw of the self-checks (undone behind the check: _Captured._self_check puts
    the target back to zeros and the weights to ones, what a constructed step documents), and the launch.

    The auxiliary loss is  weight * sum(rows) / (p * B)  with B the class's own batch -- a data-parallel shard takes the mean over its
    shard, like the loss whose d_memory the caller hands it; weight / (p * B) travels into the launch by value, everything else
    (target, row weights, step weights, lengths) is device data read when the kernel runs."""

    att_loss, aux_loss = None, None
    att_target, att_row_weights, att_step_weights, aux_rows = None, None, None, None

    def _alloc_att_loss(self, spec, p, B, S, N, dev):
        self.att_loss = _att_loss_spec(type(self).__name__, spec)
        if self.att_loss is None:
            return
        n = N if self.att_loss["on"] == "kb" else S
        self._att_segment = "att_" + self.att_loss["on"]
        self._att_shape = (int(p), int(B), int(n))
        self._att_scale = self.att_loss["weight"] / float(p * B)
        if self.att_loss["kind"] == "ce":
            self.att_target = torch.zeros(self._att_shape if self.att_loss["per_step_target"] else self._att_shape[1:], device=dev)
        self.att_row_weights = torch.ones(B, device=dev)
        self.att_step_weights = torch.ones(p, device=dev)
        self.aux_rows = torch.zeros(p, B, device=dev)

    def _check_att_loss(self, att_target, att_row_weights, att_step_weights, n=None):
        """load()'s refusals: att_target exactly when built for kind "ce", the weights only when built with att_loss, shapes.
        n: None, or the questions of a short batch (a tower class built with weights=True): the per-question axis is n long"""
        who = type(self).__name__
        _lengths_argument(who, "att_target", att_target is not None, self.att_target is not None, 'att_loss=dict(kind="ce")')
        for name, t in (("att_row_weights", att_row_weights), ("att_step_weights", att_step_weights)):
            if t is not None:
                _lengths_argument(who, name, True, self.att_loss is not None, "att_loss=")
        for name, t, buf, axis in (("att_target", att_target, self.att_target, -2), ("att_row_weights", att_row_weights, self.att_row_weights, 0),
                                   ("att_step_weights", att_step_weights, self.att_step_weights, None)):
            if t is None:
                continue
            want = list(buf.shape)
            if n is not None and axis is not None:
                want[axis] = n
            if not torch.is_tensor(t) or list(t.shape) != want or not t.dtype.is_floating_point:
                raise ValueError("%s must be a %s floating-point tensor" % (name, want))

    def _copy_att_loss(self, att_target, att_row_weights, att_step_weights, n=None):
        """... and its copies (None keeps what the buffer holds).  n (a tower class built with weights=True): the target's slots behind
        the n questions become copies of slot 0 (_pad_slots), the row weights there 0 -- and att_row_weights=None then means ones for
        the n questions, not "keep": a longer batch after a shorter one would otherwise inherit its zeros"""
        with torch.no_grad():
            if n is not None and self.att_loss is not None:
                if att_target is not None:
                    _pad_slots(self.att_target, att_target, n, axis=self.att_target.dim() - 2)
                    att_target = None
                self.att_row_weights[:n] = 1.0 if att_row_weights is None else att_row_weights
                self.att_row_weights[n:] = 0.0
                att_row_weights = None
            for t, buf in ((att_target, self.att_target), (att_row_weights, self.att_row_weights), (att_step_weights, self.att_step_weights)):
                if t is not None:
                    buf.copy_(t)

    def _randomise_att_loss(self, gen, live):
        """the self-check's draw: target = softmax of N(0,1) over each question's live cells (live: [B] sizes on the host, None = all;
        zeros behind them), row weights in [0.5, 1.5] with the last question unsupervised (B > 1), step weights in [0.5, 1.5]"""
        if self.att_loss is None:
            return
        p, B, n = self._att_shape
        with torch.no_grad():
            if self.att_target is not None:
                dead = torch.zeros(B, n, dtype=torch.bool) if live is None else torch.arange(n).unsqueeze(0) >= live.clamp(1, n).unsqueeze(1)
                logits = torch.randn(self.att_target.shape, generator=gen).masked_fill(dead.expand(self.att_target.shape), float("-inf"))
                self.att_target.copy_(torch.softmax(logits, dim=-1))
            rw = 0.5 + torch.rand(B, generator=gen)
            if B > 1:
                rw[-1] = 0.0
            self.att_row_weights.copy_(rw)
            self.att_step_weights.copy_(0.5 + torch.rand(p, generator=gen))

    def _reset_att_loss(self):
        """the static tensors as construction leaves them: target zeros, row and step weights ones, rows zeros"""
        with torch.no_grad():
            for t, value in ((self.att_target, 0.0), (self.att_row_weights, 1.0), (self.att_step_weights, 1.0), (self.aux_rows, 0.0)):
                if t is not None:
                    t.fill_(value)

    def _att_lengths(self, cell):
        """the lengths the supervised map was computed under: the cell's own device tensors (kb: None when every question has N)"""
        cell = getattr(cell, "inner", cell)          # (a zero-padded cell wraps the real one)
        return cell.kb_lengths if self.att_loss["on"] == "kb" else cell.questionLengths

    def _att_loss_rows(self, cell):
        """attention_loss on the cell's stacked map, the rows written into the static `aux_rows`: [p, B] with the autograd edge"""
        from .losses import attention_loss
        a = self.att_loss
        return attention_loss(cell.state_tensor(self._att_segment), self.att_target, self._att_lengths(cell), self.att_step_weights,
                              self.att_row_weights, kind=a["kind"], eps=a["eps"], scale=self._att_scale, _rows_out=self.aux_rows)

    def _aux_terms(self, cell, state):
        """the scalars the step differentiates besides its own loss: [] for a class built without att_loss / aux_loss"""
        terms = [] if self.att_loss is None else [self._att_loss_rows(cell).sum()]
        if self.aux_loss is not None:
            terms.append(self.aux_loss(cell, state))
        return terms


class _CellInputs(_AttLoss):
    """the static input tensors of a captured cell (the training classes' att_loss= tensors among them: _AttLoss), load() into them
    and the cell built on them"""

    d_memory = None                                  # [B, d] gradient of the final memory: the training classes
    kb_lengths = None                                # [B] int32 live knowledge-base cells per question: kb_lengths=True

    def _alloc_inputs(self, config, params, B, S, N, device, netLength, train=False, requires_grad=False, kb_lengths=False):
        """kb_lengths: also a static [B] int32 `kb_lengths` (all N), which the cell's attention kernel reads when it runs -- one
        graph serves every set of lengths.  Allocated here, before the capture: the host writes it between replays, so it must not
        come from the graph's pool."""
        dev = _require_hip(torch.device(device) if device is not None else params.tensors()[0].device, type(self).__name__, "the MAC cell")
        d = int(get(config, "memDim"))
        self.config, self.params = config, params
        self.netLength = int(netLength if netLength is not None else get(config, "netLength"))
        self.vecQuestions = torch.zeros(B, d, device=dev, requires_grad=requires_grad)
        self.words = torch.zeros(B, S, d, device=dev, requires_grad=requires_grad)
        self.lengths = torch.full((B,), S, dtype=torch.int32, device=dev)
        self.knowledgeBase = torch.zeros(B, N, d, device=dev, requires_grad=requires_grad)
        if train:
            self.d_memory = torch.zeros(B, d, device=dev)
        if kb_lengths:
            self.kb_lengths = torch.full((B,), N, dtype=torch.int32, device=dev)
        return dev

    def _randomise(self, seed):
        """N(0, 1) inputs for the self-check; with kb_lengths: one question at N, one at 1, the rest random (the device-read path)"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for t in (self.vecQuestions, self.words, self.knowledgeBase) + (() if self.d_memory is None else (self.d_memory,)):
                t.copy_(torch.randn(t.shape, generator=g).to(t.device))
            live = None
            if self.kb_lengths is not None:
                live = _draw_lengths(g, *self.knowledgeBase.shape[:2])
                self.kb_lengths.copy_(live)
        if self.att_loss is not None:
            self._randomise_att_loss(g, live if self.att_loss["on"] == "kb" else self.lengths.cpu())

    def load(self, vecQuestions, words, lengths, knowledgeBase, d_memory=None, kb_lengths=None, check_ids=True, att_target=None,
             att_row_weights=None, att_step_weights=None):
        """Copy a batch into the captured run's input tensors (or write into .knowledgeBase etc. directly and skip this);
        d_memory: the training classes' [B, d] gradient of the final memory, and theirs only;
        kb_lengths: the [B] integer sizes of a class built with kb_lengths=True, and of such a class only; check_ids tests
        1 <= kb_lengths <= N on the host first (synchronises; unchecked values are clamped by the kernel);
        att_target: the target distribution of a training class built with att_loss=dict(kind="ce"), and of such a class only
        ([B, n], or [p, B, n] with per_step_target); att_row_weights [B] / att_step_weights [p]: a class built with att_loss= (None
        keeps what .att_row_weights / .att_step_weights hold: ones after construction)"""
        if (d_memory is None) != (self.d_memory is None):
            raise TypeError("%s.load() takes %s d_memory" % (type(self).__name__, "no" if self.d_memory is None else "a"))
        _lengths_argument(type(self).__name__, "kb_lengths", kb_lengths is not None, self.kb_lengths is not None)
        if kb_lengths is not None:
            _check_lengths(kb_lengths, *self.knowledgeBase.shape[:2], check_ids, "kb_lengths")
        self._check_att_loss(att_target, att_row_weights, att_step_weights)
        self._copy_att_loss(att_target, att_row_weights, att_step_weights)
        with torch.no_grad():
            self.vecQuestions.copy_(vecQuestions)
            self.words.copy_(words)
            self.lengths.copy_(lengths)
            self.knowledgeBase.copy_(knowledgeBase)
            if d_memory is not None:
                self.d_memory.copy_(d_memory)
            if kb_lengths is not None:
                self.kb_lengths.copy_(kb_lengths)

    def _make_cell(self, train):
        """evaluation: no dropout, no seed, no word; training: the config's keep values, seed, b0 and the mask word"""
        keep = [float(get(self.config, k)) if train else 1.0 for k in ("memoryDropout", "readDropout", "writeDropout")]
        drawn = dict(seed=self.seed, b0=self.b0, mask_word=self.mask_word) if train else {}
        if self.kb_lengths is not None:               # (None: the cell's call of before)
            drawn["kb_lengths"] = self.kb_lengths
        return MACCell(vecQuestions=self.vecQuestions, questionWords=self.words, questionCntxWords=self.words,
                       questionLengths=self.lengths, knowledgeBase=self.knowledgeBase, memoryDropout=keep[0], readDropout=keep[1],
                       writeDropout=keep[2], batchSize=self.vecQuestions.shape[0], train=train, config=self.config,
                       params=self.params, netLength=self.netLength, **drawn)


class CapturedForward(_Captured, _CellInputs):
    _WHAT = ("run", "run")

    def __init__(self, config, params, B, S, N, device=None, netLength=None, warmup=2, verify=True, check_every=0, kb_lengths=False):
        self.check_every = int(check_every)
        dev = self._alloc_inputs(config, params, B, S, N, device, netLength, kb_lengths=kb_lengths)
        self.graph = torch.cuda.CUDAGraph()
        self._capture(dev, warmup, self._eager, [(self.graph, self._issue)])
        self._self_check(verify)

    @torch.no_grad()
    def _eager(self):
        self.cell = self._make_cell(train=False)      # (status(): the latest run's buffers)
        return self.cell.run()

    def _issue(self):
        state = self._eager()
        self.memory, self.control, self.attentions = state.memory, state.control, self.cell.attentions

    def _replays_match_eager(self, replays=3):
        self._randomise(20240519)
        want = self._eager_on_captured([], lambda: [self._eager().memory.clone()])
        return self._compare_replays(replays, lambda: [("memory", self.memory)], want)

    def replay(self):
        if self.captured:
            self.graph.replay()
        else:                                    # (see the module docstring)
            self._issue()
        self._count_replay()
        return self.memory

    def __call__(self, vecQuestions, words, lengths, knowledgeBase, kb_lengths=None):
        self.load(vecQuestions, words, lengths, knowledgeBase, kb_lengths=kb_lengths)
        return self.replay()


class CapturedTrainStep(_Captured, _CellInputs, _MaskWord):
    """Forward + backward of the cell (train-mode dropout, every gradient) replayed from ONE captured HIP graph.

        step = macx.CapturedTrainStep(cfg, params, B=64, S=50, N=196, seed=1234)
        step.load(vecQuestions, words, lengths, knowledgeBase, d_memory)     # or write into step.knowledgeBase etc.
        step.replay()                        # params' .grad, step.knowledgeBase.grad, step.words.grad, step.vecQuestions.grad
        memory = step.memory                 # [B, d] final memory of the run

    About 140 launches per step (p = 12) plus what autograd adds around them; a host that cannot issue them faster than the
    GPU retires them (gpurun boxes differ by 7x in host speed) sets the pace of the eager step, a replay does not depend on it.
    The library issues no memset / memcpy node (module docstring; the minimum-exponent arrays behind the deferred contractions
    were the last memset-then-atomicMin pair), which is what makes the backward pass capturable.

    Fresh masks per replay -- the dropout masks are a function of (seed, site, step, element) and the seed travels BY VALUE in
    the kernel arguments, so a capture bakes it.  The run therefore also carries one 32-bit word in DEVICE memory
    (`macx_dropout.mask_word`, `step.mask_word`) that every dropout site XORs into its key when the kernel RUNS:

        for it in range(steps):
            step.load(...)
            step.replay(iteration=it)        # word = mix32(it): the masks of (seed, word); same word => same masks

    `replay()` without an argument keeps the word it has (0 after construction: the masks of the plain seed), which is what
    measurement wants.  The eager step behind `_eager()` reads the same word, so verification compares like with like.

    `verify=True` replays three times against the eager step on random inputs and falls back to eager launches when a replay
    differs in any gradient (`captured` False, a warning says so).

    Losses on the run's own maps and states, inside the graph (the gradient of such a loss depends on the forward pass of the SAME
    replay, so it cannot be a static input):

    att_loss=dict(on="kb" | "question", kind="ce" | "entropy", weight=lam, eps=1e-8, per_step_target=False) adds
    lam * sum(rows) / (p * B) of losses.attention_loss on cell.state_tensor("att_kb" | "att_question") to what the step
    differentiates -- one launch (macx_att_loss) between the forward and the backward launches.  Static tensors, allocated before
    the capture and read when the kernel runs: `att_target` ([B, n], [p, B, n] with per_step_target; kind "ce" only),
    `att_row_weights` [B] and `att_step_weights` [p] (ones; a row weight of 0: that question is unsupervised), written by
    load(..., att_target=, att_row_weights=, att_step_weights=) or directly; the output `aux_rows` [p, B].  on="kb" masks by the
    class's kb_lengths, on="question" by the question lengths.  The self-check draws all of them and afterwards puts the target
    back to zeros and the weights back to ones: None in load() keeps ones until the caller writes others.

        step = macx.CapturedTrainStep(cfg, params, B=64, S=50, N=196, att_loss=dict(on="kb", kind="ce", weight=0.1))
        step.load(vecQuestions, words, lengths, knowledgeBase, d_memory, att_target=boxes_as_distribution)
        step.replay(); aux = step.aux_rows.sum()

    aux_loss=callable(cell, state) -> scalar tensor: a loss written in torch ops on cell.state_tensor(...) (per-step heads on
    "memories", the self-attention, the gate), evaluated inside the step and therefore inside the graph.  It must not synchronise
    with the host (no .item(), no printing of values, no data-dependent Python branches), and every tensor it reads that the HOST
    writes between replays must be allocated by the caller BEFORE this class is constructed (a tensor allocated inside the callable
    comes from the graph's pool).  A head's own parameters take their gradients as any leaf does, but the step does not clear
    them: their .grad is allocated by the warm-up and every replay ADDS to it in place -- zero it in place (grad.zero_(), never
    grad = None) before a replay whose gradient is to be read alone."""

    def __init__(self, config, params, B, S, N, seed=0, device=None, netLength=None, b0=0, warmup=2, verify=True, check_every=0,
                 kb_lengths=False, att_loss=None, aux_loss=None):
        self.seed, self.b0 = int(seed), int(b0)
        self.check_every = int(check_every)
        att_loss = _att_loss_spec(type(self).__name__, att_loss)
        dev = self._alloc_inputs(config, params, B, S, N, device, netLength, train=True, requires_grad=True, kb_lengths=kb_lengths)
        self._alloc_att_loss(att_loss, self.netLength, B, S, N, dev)
        self.aux_loss = aux_loss
        self._alloc_mask_word(dev)
        self.graph = torch.cuda.CUDAGraph()
        self._capture(dev, warmup, self._eager, [(self.graph, self._issue)], before=self._clear_grads)
        self._self_check(verify)

    def _leaves(self):
        return [self.vecQuestions, self.words, self.knowledgeBase] + list(self.params.tensors())

    def _clear_grads(self):
        for t in self._leaves():
            t.grad = None

    def _eager(self):
        self._clear_grads()
        self.cell = self._make_cell(train=True)   # (status(): the latest run's buffers)
        state = self.cell.run()
        aux = self._aux_terms(self.cell, state)
        torch.autograd.backward([state.memory] + aux, [self.d_memory] + [None] * len(aux))
        return state.memory.detach()

    def _issue(self):
        self.memory = self._eager()

    def eager_reference(self):
        """The eager step on the static tensors under the current mask word: (memory, [gradient of each of _leaves()]), all clones.
        The captured `.grad` tensors and `cell` are put back, so the next replay() writes where the graph writes.  Synchronises."""
        leaves = self._leaves()
        return self._eager_on_captured(leaves, lambda: (self._eager().clone(), [t.grad.clone() for t in leaves]))

    def _replays_match_eager(self, replays=3):
        self.set_mask_word(0x5bd1e995)          # a non-trivial word: the check covers the device-read path as well
        self._randomise(20240520)
        memory, grads = self.eager_reference()
        extra = [] if self.aux_rows is None else [self.aux_rows.clone()]                  # (the eager run wrote the static buffer)
        # labels: the index into [memory] + leaves (+ aux_rows)
        written = lambda: enumerate([self.memory] + [t.grad for t in self._leaves()] + ([] if self.aux_rows is None else [self.aux_rows]))
        return self._compare_replays(replays, written, [memory] + grads + extra)

    def replay(self, iteration=None):
        """iteration: None keeps the current mask word; an int draws the masks of word mix32(iteration)"""
        self._set_iteration(iteration)
        if self.captured:
            self.graph.replay()
        else:
            self._issue()
        self._count_replay()
        return self.memory


class CapturedDPTrainStep(_Captured, _CellInputs, _MaskWord, TwoPhaseStep):
    """One DATA-PARALLEL training step of the cell as TWO graph replays with the gradient exchange between and behind them.

    The eager data-parallel step is ~125 host-issued launches per rank; at 8 questions per GPU that is more host work than GPU work
    and inherits the host's launch rate (DESIGN: boxes differ 7x).  The exchange itself cannot sit inside a graph (RCCL calls are
    issued by torch.distributed), but the backward pass has exactly one seam where it is needed: after phase 1
    (macx_cell_backward_phase) every gradient except the read unit's deferred contractions is final.  So:

        graph A = forward + backward phase 1            replay
        early bucket: scale + all-reduce                side stream, in flight under graph B     (bucket._phase1)
        graph B = backward phase 2                      replay
        late bucket: scale + all-reduce, join           (bucket.allreduce_)

    -- 2 replays + 2 collectives per step instead of ~125 launches.  `bucket` is a macx.dp.OverlappedBuckets (two buckets; RCCL) or a
    macx.dp.GradBucket built over params (one all-reduce behind graph B); the step drives it exactly as the cell's autograd node
    drives it in the eager step, so both produce the same bits (tests/test_gpu_dp.py, two ranks sharing the GPU).  No autograd is
    involved: the two phases are the C-ABI calls themselves, captured on static buffers; parameters' .grad are views of the flat
    gradient buffer.  Fresh dropout masks per step through the mask word, as CapturedTrainStep.

        bucket = macx.dp.OverlappedBuckets(params)
        step = macx.CapturedDPTrainStep(cfg, params, bucket, B=shard, S=50, N=196, global_batch=64, seed=1234, b0=lo)
        step.load(vecQ[lo:hi], words[lo:hi], lengths[lo:hi], kb[lo:hi], d_memory[lo:hi])
        step.step(iteration=it)              # params' .grad = the all-reduced full-batch gradient; step.memory: [shard, d]

    att_loss=: CapturedTrainStep's, with B the shard -- lam * sum(rows) / (p * shard), the mean over the shard that the bucket then
    weights like the loss behind d_memory.  There is no autograd here: behind the forward pass, phase A launches macx_att_loss on
    the run's stacked map (a segment of `saved`), which writes `aux_rows` and a static d_att buffer that the backward pass's
    macx_state_grads points at -- in both graphs' capture and on the uncaptured route alike.  aux_loss= (a loss in torch ops)
    needs autograd and is refused: att_loss= is this class's route, CapturedTrainStep takes callables.
    """

    def __init__(self, config, params, bucket, B, S, N, global_batch, seed=0, b0=0, device=None, netLength=None, warmup=2, capture=True,
                 check_every=0, kb_lengths=False, att_loss=None, aux_loss=None):
        if aux_loss is not None:
            raise TypeError("CapturedDPTrainStep takes no aux_loss: its two phases are the library's calls themselves, without autograd, "
                            "so a loss written in torch ops has nothing to differentiate it.  Losses on the attention maps go through "
                            "att_loss= (one launch of the library inside phase A); CapturedTrainStep takes aux_loss=")
        att_loss = _att_loss_spec(type(self).__name__, att_loss)
        dev = self._alloc_inputs(config, params, B, S, N, device, netLength, train=True, kb_lengths=kb_lengths)
        self._alloc_att_loss(att_loss, self.netLength, B, S, N, dev)
        if self.att_loss is not None:
            self._d_att = torch.zeros(self._att_shape, device=dev)      # macx_state_grads.d_att_kb / d_att_question of every run
        if bucket.flat.data_ptr() != params.grad_buffer().data_ptr():
            raise ValueError("the bucket must be built over params' own flat gradient buffer (OverlappedBuckets(params) / "
                             "GradBucket(params.tensors(), params=params))")
        super().__init__(params, bucket, B, global_batch)
        self.check_every = int(check_every)
        self.seed, self.b0 = int(seed), int(b0)
        self._alloc_mask_word(dev)
        self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        for t in params.tensors():
            t.grad = None
        self._capture(dev, warmup, self._warm, [(self.graph_a, self._phase_a), (self.graph_b, self._phase_b)] if capture else [])
        self.captured = bool(capture)
        params.release_grad_buffer()

    def _warm(self):
        self._phase_a()
        self._phase_b()
        self.params.release_grad_buffer()

    def _phase_a(self):
        """forward + backward phase 1 on the current stream; leaves self._run / self._args for phase 2"""
        with torch.no_grad():
            cell = self._make_cell(train=True)
            run = _Run(cell, True)
            run.forward()
            state_grads = None
            if self.att_loss is not None:
                from .losses import KINDS, launch
                launch(run.segment(self._att_segment, self._att_shape), self.att_target, self._att_lengths(cell), self.att_step_weights,
                       self.att_row_weights, KINDS[self.att_loss["kind"]], self.att_loss["eps"], self._att_scale, self.aux_rows, self._d_att)
                state_grads = {"d_" + self._att_segment: self._d_att}
            args, grads, gi, flat, keep = run.backward_begin(None, self.d_memory, state_grads)
            if flat.data_ptr() != self.bucket.flat.data_ptr():
                raise RuntimeError("the backward pass did not receive the parameters' flat gradient buffer (is a gradient still attached?)")
            run.backward_phase(args, 1)
        p = run.shapes.p
        self.memory = run.segment("memories", (p + 1, run.shapes.B, run.shapes.d))[p]
        self.d_vecQuestions, self.d_words, self.d_knowledgeBase = gi
        self._grads = grads
        self._run, self._args, self._keep = run, args, (keep, cell)

    def _status_run(self):
        return getattr(self, "_run", None)

    def _phase_b(self):
        with torch.no_grad():
            self._run.backward_phase(self._args, 2)

    def run_part_a(self):
        if self.captured:
            self.graph_a.replay()
        else:
            for t in self.params.tensors():
                t.grad = None
            self._phase_a()
        return self._grads

    def run_part_b(self):
        if self.captured:
            self.graph_b.replay()
        else:
            self._phase_b()

    def step(self, iteration=None):
        """one data-parallel step; afterwards every parameter's .grad is its view of the all-reduced flat buffer"""
        self._set_iteration(iteration)
        self.exchange_step()
        self._count_replay()
        return self.memory


# ---------------------------------------------------------------------------------------------------------------------------
# the whole tower (model.MACNet: question ids, lengths, image features in; logits out) from one graph
# ---------------------------------------------------------------------------------------------------------------------------
def _require_fused_tower(net, who):
    """the tower's captured classes take a model.MACNet whose four modules are the fused ones (UnsupportedOptions otherwise), on
    the HIP device (RuntimeError otherwise); returns the device"""
    from .encoder import QuestionEncoder, RecurrentQuestionEncoder
    from .output import OutputClassifier
    from .stem import Stem
    want = (("enc", QuestionEncoder), ("stem", Stem), ("cell", MACCellParams), ("out", OutputClassifier))
    for name, cls in want:
        mod = getattr(net, name, None)
        if mod is None:
            raise TypeError("%s takes a macx.MACNet (question encoder, stem, cell, output unit); this net has no .%s" % (who, name))
        if not isinstance(mod, cls) and not (name == "enc" and isinstance(mod, RecurrentQuestionEncoder)):
            raise UnsupportedOptions("%s: net.%s is a %s; only a tower of the fused modules (%s) is captured -- the generic "
                                     "one-kernel-per-op modules are out of its scope" % (who, name, type(mod).__name__,
                                                                                        ", ".join(c.__name__ for _, c in want)))
    return _require_hip(net.tensors()[0].device, who, "the tower")


def _random_tower_inputs(gen, B, S, vocab, shape_images, answers, dev):
    """(images, questions, lengths, answer ids) for the self-checks: relu(N(0,1)) features, ids in [1, vocab] up to each question's
    length (question 0 at full length, one of length 1 when B > 1), zero pad ids behind it"""
    images = torch.relu(torch.randn(shape_images, generator=gen))
    lengths = torch.randint(1, S + 1, (B,), generator=gen, dtype=torch.int32)
    lengths[0] = S
    if B > 1:
        lengths[1] = 1
    q = torch.randint(1, vocab + 1, (B, S), generator=gen, dtype=torch.int32)
    q = q * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)
    ans = torch.randint(0, answers, (B,), generator=gen, dtype=torch.int32)
    return images.to(dev), q.to(dev), lengths.to(dev), ans.to(dev)


class _TowerInputs(_AttLoss):
    """the static input tensors of a captured tower (the training step's att_loss= tensors among them: _AttLoss) and load() into them"""

    G, image_index = None, None            # questions that share images (images=G): see _alloc_inputs
    kb_lengths, image_lengths = None, None # knowledge bases of per-question / per-image size: see _alloc_inputs
    weights, totals, n = None, None, None  # per-question answer weights, running totals, questions of the last load: _alloc_weights
    features, image_ids = None, None       # image features resident in device memory (features=store): see _alloc_inputs
    _WEIGHTS_HOW = "weights=True"          # the constructor argument that builds `weights`
    question_store, question_ids, predictions = None, None, None   # questions resident in device memory (questions=store)
    records = None                         # evaluation records resident in device memory (records=rec): see _check_questions

    def _alloc_weights(self, dev, totals):
        """A static [B] float32 `weights` (all ones), which the answer-loss kernel (macx_answer_loss_weighted) reads when it runs: one
        graph serves every n <= B questions (weights of 0 behind them) and every re-weighting.  totals: None, True (a new
        output.AnswerTotals) or one to adopt.  Both are allocated here, before the capture: the host writes them between replays, so
        they must not come from the graph's pool."""
        from .output import AnswerTotals
        self.weights = torch.ones(self.B, dtype=torch.float32, device=dev)
        if totals is not None and totals is not False:
            self.totals = AnswerTotals(dev) if totals is True else totals

    @staticmethod
    def _check_totals(who, weights, totals):
        """what a constructor refuses about weights= / totals= before it asks for the device"""
        from .output import AnswerTotals
        if totals is not None and totals is not False and totals is not True and not isinstance(totals, AnswerTotals):
            raise TypeError("%s: totals is None, True or a macx.output.AnswerTotals, not %r" % (who, totals))
        if totals and not weights:
            raise ValueError("%s: totals= belongs to the weighted answer loss: build the class with weights=True" % who)

    def _loss_arguments(self):
        """the keyword arguments of loss_and_pred that the static tensors stand for ({}: the call of before)"""
        return {} if self.weights is None else {"weights": self.weights, "totals": self.totals}

    def _draw_weights(self):
        """the self-checks' weights: one 0 (the last question, B > 1), one fraction, the rest ones -- the device-read path, as
        _draw_lengths for the lengths"""
        if self.weights is not None:
            w = torch.ones(self.B)
            w[0] = 0.5
            if self.B > 1:
                w[-1] = 0.0
            self.weights.copy_(w)

    def _reset_weights(self):
        """as construction leaves them: weights ones, totals cleared, a full batch"""
        if self.weights is not None:
            self.weights.fill_(1.0)
            self.n = self.B
        if self.totals is not None:
            self.totals.reset()

    def _refuse_other_count(self, n):
        if self.weights is None and n != self.B:
            raise ValueError("%s was captured for batches of %d questions and got %d: a class built with weights=True "
                             "(CapturedTowerForward: score=True) takes any n <= %d" % (type(self).__name__, self.B, n, self.B))

    def _refuse_other_size(self, questions):
        """a class built without `weights` takes batches of B questions only (this used to be a reshape error, and n = 1 was broadcast
        into every slot); load() raises it before any other complaint about the batch's shapes"""
        if torch.is_tensor(questions) and questions.dim() == 2:
            self._refuse_other_count(questions.shape[0])

    # ---- questions resident in device memory (questions=store): the batch is a vector of question ids
    @staticmethod
    def _check_questions(net, who, store, B, S, images, kb_lengths, image_lengths, features, att_loss, needs_answers, predictions=None,
                         records=None):
        """what a constructor refuses about questions= / predictions= / records= before it asks for the device"""
        from .questions import MAX_GROUP_BATCH, QuestionStore
        if store is None:
            if predictions is not None:
                raise ValueError("%s: predictions= is a table over a question store: build the class with questions=" % who)
            if records is not None:
                raise ValueError("%s: records= files by the ids of a question store: build the class with questions=" % who)
            return
        if not isinstance(store, QuestionStore):
            raise TypeError("%s: questions is None or a macx.QuestionStore, not %s" % (who, type(store).__name__))
        if store.S > int(S):
            raise ValueError("%s: the QuestionStore holds questions of %d words, the graph is captured for S = %d" % (who, store.S, int(S)))
        vocab = getattr(getattr(net, "enc", None), "vocab", None)
        if vocab is not None and store.max_word > vocab:
            raise ValueError("%s: the QuestionStore holds word id %d, the encoder's vocabulary ends at %d" % (who, store.max_word, vocab))
        answers = getattr(getattr(net, "out", None), "answers", None)
        if needs_answers and store.answers is None:
            raise ValueError("%s: the class reads answers and the QuestionStore holds none" % who)
        if store.max_answer is not None and answers is not None and store.max_answer >= answers:
            raise ValueError("%s: the QuestionStore holds answer %d, the classifier has %d answers" % (who, store.max_answer, answers))
        if (features is not None) != (store.image_rows is not None):
            raise ValueError("%s: features= and the QuestionStore's image_rows go together (the rows of the questions' images in the "
                             "FeatureStore): %s" % (who, "the store holds no image_rows" if features is not None
                                                    else "the store holds image_rows and no features= was given"))
        if kb_lengths and store.kb_lengths is None:
            raise ValueError("%s(kb_lengths=True): the QuestionStore holds no kb_lengths" % who)
        if images is not None and features is None:
            raise ValueError("%s(questions=, images=G) groups the batch by FeatureStore row: it needs features=" % who)
        if image_lengths:
            raise ValueError("%s(questions=): image_lengths=True is out of scope -- per-image sizes do not come from a question store" % who)
        if att_loss is not None:
            raise ValueError("%s(questions=): att_loss= is out of scope -- the store holds no per-question attention targets" % who)
        if images is not None and int(B) > MAX_GROUP_BATCH:
            raise ValueError("%s(questions=, images=G): the grouping launch takes at most %d questions, B = %d" % (who, MAX_GROUP_BATCH, int(B)))
        if hasattr(net, "tensors") and store.questions.device != net.tensors()[0].device:
            raise ValueError("%s: the QuestionStore lives on %s, the net on %s" % (who, store.questions.device, net.tensors()[0].device))
        if predictions is not None:
            if (not torch.is_tensor(predictions) or predictions.dtype != torch.int32 or tuple(predictions.shape) != (store.count,)
                    or not predictions.is_contiguous() or predictions.device != store.questions.device):
                raise ValueError("%s: predictions is a contiguous [%d] int32 tensor on the store's device (store.predictions())"
                                 % (who, store.count))
        if records is not None:
            from .records import EvalRecords
            if not isinstance(records, EvalRecords):
                raise TypeError("%s: records is None or a macx.EvalRecords, not %s" % (who, type(records).__name__))
            if records.store is not store:
                raise ValueError("%s: the EvalRecords were built over another QuestionStore than questions=" % who)
            if records.device != store.questions.device:
                raise ValueError("%s: the EvalRecords live on %s, the QuestionStore on %s" % (who, records.device, store.questions.device))
            stem = getattr(net, "stem", None)
            have = {"p": getattr(net, "netLength", None), "N": None if stem is None else stem.out_hw[0] * stem.out_hw[1], "S": int(S),
                    "answers": getattr(getattr(net, "out", None), "answers", None)}
            for name, want in have.items():
                got = getattr(records, name)
                if want is not None and got is not None and int(got) != int(want):
                    raise ValueError("%s: the EvalRecords were built for %s = %d, the captured run has %s = %d" % (who, name, got, name, want))
            if "self" in records.tables and not get(net.config, "writeSelfAtt"):
                raise ValueError("%s: the EvalRecords hold a \"self\" table and the cell runs without writeSelfAtt" % who)

    def _alloc_questions(self, store, dev, predictions=None, records=None):
        """A static int32 `question_ids` [B], all -1 (dead slots), which the gather at the head of the graph (macx_questions_gather)
        reads when it runs.  Allocated here, before the capture, like every buffer the host writes; the predictions table
        and the records' tables are the caller's, allocated before the capture for the same reason (the host reads them)."""
        self.question_store, self.predictions, self.records = store, predictions, records
        if store is not None:
            self.question_ids = torch.full((self.B,), -1, dtype=torch.int32, device=dev)

    def _gather_questions(self):
        """the head of the captured body: every per-question static tensor <- the questions `question_ids` names (one launch; with
        images=G also the batch's distinct image rows and image_index)"""
        if self.question_store is not None:
            self.question_store.gather_into(self.question_ids, self.questions, self.lengths, self.answers, self.image_ids, self.kb_lengths,
                                            self.weights, self.image_index)

    def _scatter_predictions(self, pred):
        if self.predictions is not None:
            self.question_store.scatter_predictions(self.predictions, pred, self.question_ids)

    def _file_records(self, logits):
        """the tail of the captured body: the run's attention maps and logits into the records' tables by question id (one launch)"""
        if self.records is not None:
            self.records.file_run(self.question_ids, self.cell, logits if "logits" in self.records.tables else None)

    def _draw_question_ids(self, gen):
        """the self-checks' batch: random ids with the store's last row in slot 0, a repeat of it in the middle and, where the class has
        weights, a dead slot at the end; with images=G no more than G distinct image rows (more would poison the run on purpose)"""
        store, B = self.question_store, self.B
        ids = torch.randint(0, store.count, (B,), generator=gen, dtype=torch.int32)
        ids[0] = store.count - 1
        ids[B // 2] = ids[0]
        if self.G is not None:
            rows = store.image_rows[ids.to(store.device).long()].cpu()
            seen = []
            for b in range(B):
                if int(rows[b]) not in seen:
                    if len(seen) == self.G:
                        ids[b] = ids[0]
                        continue
                    seen.append(int(rows[b]))
        if self.weights is not None and B > 1:
            ids[-1] = -1
        self.question_ids.copy_(ids)

    def _reset_questions(self):
        """as construction leaves them: every slot dead, the store's `bad` word cleared, a full batch"""
        if self.question_store is not None:
            self.question_ids.fill_(-1)
            self.question_store.reset_bad()
            self.n = self.B

    def _refuse_load(self):
        if self.question_store is not None:
            raise ValueError("%s was captured with questions= (a macx.QuestionStore): a batch is a vector of question ids -- load_ids(ids) "
                             "or next_batch(order), not load()" % type(self).__name__)

    def _require_questions(self, what):
        if self.question_store is None:
            raise TypeError("%s.%s() belongs to a class built with questions= (a macx.QuestionStore)" % (type(self).__name__, what))
        return self.question_store

    def _write_ids(self, ids, n):
        with torch.no_grad():
            self.question_ids[:n].copy_(ids)
            if n < self.B:
                self.question_ids[n:].fill_(-1)
        self.n = n
        return n

    def load_ids(self, ids, check_ids=True):
        """A batch by question id: 1 <= n <= B ids of the store's questions (an integer tensor) into the static `question_ids`, -1 (dead
        slots) behind them; n < B only in a class built with weights=True / score=True.  check_ids tests 0 <= ids < count on the host
        (synchronises for a device tensor; unchecked ids outside the store poison their question and set store.bad).  Returns n."""
        store = self._require_questions("load_ids")
        store.check_ids(ids)
        n = int(ids.shape[0])
        self._refuse_other_count(n)
        if not 1 <= n <= self.B:
            raise ValueError("%s was captured for batches of %d questions: load_ids() takes 1 <= n <= %d of them, got %d"
                             % (type(self).__name__, self.B, self.B, n))
        store.check_ids(ids, n, host_check=check_ids)
        return self._write_ids(ids, n)

    def next_batch(self, order):
        """The next B ids of a macx.EpochOrder into `question_ids` (a device-to-device copy; -1 behind the epoch's end, which needs a
        class built with weights=True / score=True) and the order advanced.  Returns n; IndexError when the epoch is exhausted."""
        store = self._require_questions("next_batch")
        if getattr(order, "store", None) is not store or order.B != self.B:
            raise ValueError("%s.next_batch(): the order must be a macx.EpochOrder over this class's QuestionStore with B = %d"
                             % (type(self).__name__, self.B))
        if order.remaining > 0:
            self._refuse_other_count(min(self.B, order.remaining))
        ids = order.take()
        return self._write_ids(ids, int(ids.shape[0]))

    def _batch(self, questions, weights, per_question):
        """n, the questions of a load -- B, or with `weights` 1 <= n <= B -- and the refusals about it, raised before anything is
        copied: per_question is the (name, tensor) list of the arguments that carry one entry per question"""
        who = type(self).__name__
        if weights is not None and self.weights is None:
            raise TypeError("%s.load() takes no weights: the graph was captured without %s" % (who, self._WEIGHTS_HOW))
        if not torch.is_tensor(questions) or questions.dim() != 2:
            raise ValueError("questions must be a [n, %d] integer tensor" % self.S)
        n = int(questions.shape[0])
        self._refuse_other_size(questions)
        if not 1 <= n <= self.B:
            raise ValueError("%s was captured for batches of %d questions: load() takes 1 <= n <= %d of them, got %d" % (who, self.B, self.B, n))
        for name, t in per_question:
            if t is not None and (not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] != n):
                raise ValueError("%s must have the leading size %d of questions (one entry per question)" % (name, n))
        if weights is not None:
            if not torch.is_tensor(weights) or weights.dtype != torch.float32:
                raise TypeError("weights must be a float32 tensor")
            if tuple(weights.shape) != (n,):
                raise ValueError("weights must be [%d] (one per question), got %s" % (n, list(weights.shape)))
        return n

    @staticmethod
    def _check_options(net, who, images, kb_lengths, image_lengths, train):
        """what a constructor refuses before it asks for the device"""
        if image_lengths and images is None:
            raise ValueError("%s(image_lengths=True) needs images=G: the sizes belong to shared images (one image per question: "
                             "kb_lengths=True)" % who)
        if image_lengths and kb_lengths:
            raise ValueError("%s: image_lengths and kb_lengths both given: with image_lengths the per-question sizes are made on the "
                             "device (image_lengths[image_index])" % who)
        if images is not None and train and hasattr(net, "stem"):       # the eager path's ValueError for a stem that drops (stem.check_image_index)
            from .stem import check_image_index
            check_image_index(torch.zeros(1, dtype=torch.int32), 1, True, net.stem)

    def _alloc_inputs(self, net, B, S, H, W, imageInDim, dev, images=None, kb_lengths=False, image_lengths=False, features=None):
        """features: None, or a macx.FeatureStore: no static image tensor; a static int32 `image_ids` ([B], or [G] with images=G)
        names the table rows of the batch's images and the captured gather (macx_features_gather) reads it at replay time.  H, W and
        imageInDim are then the store's.  Allocated here, before the capture, like every buffer the host writes.
        images: None (one image per question), or G: the static image tensor holds G images and a static [B] int32
        `image_index`, read by the captured gather kernel at replay time, says which one each question looks at.
        kb_lengths: a static [B] int32 `kb_lengths` (all N), read by the cell's attention kernel at replay time.
        image_lengths (with images=G): a static [G] int32 `image_lengths` (all N), read by the captured gather (macx_kb_gather_l),
        which makes the cell's per-question lengths on the device.  Both are allocated here, before the capture."""
        if features is not None:
            from .features import FeatureStore
            if not isinstance(features, FeatureStore):
                raise TypeError("features is None or a macx.FeatureStore, not %r" % type(features).__name__)
            H, W, imageInDim = features.hwc
        self.B, self.S, self.H, self.W, self.imageInDim = int(B), int(S), int(H), int(W), int(imageInDim)
        self.n = self.B
        self.N = net.stem.out_hw[0] * net.stem.out_hw[1]
        if kb_lengths:
            self.kb_lengths = torch.full((self.B,), self.N, dtype=torch.int32, device=dev)
        if images is not None:
            if int(images) < 1:
                raise ValueError("images = %r: the number of distinct images of a batch is at least 1" % (images,))
            self.G = int(images)
            self.image_index = torch.zeros(self.B, dtype=torch.int32, device=dev)
            if image_lengths:
                self.image_lengths = torch.full((self.G,), self.N, dtype=torch.int32, device=dev)
        if (net.stem.H, net.stem.W, net.stem.inDim) != (self.H, self.W, self.imageInDim):
            raise ValueError("the net's stem was built for %d x %d x %d image features, not %d x %d x %d"
                             % (net.stem.H, net.stem.W, net.stem.inDim, self.H, self.W, self.imageInDim))
        count = self.B if self.G is None else self.G
        if features is not None:
            if features.table.device != dev:
                raise ValueError("the FeatureStore lives on %s, the net on %s" % (features.table.device, dev))
            self.features, self.images = features, None
            self.image_ids = torch.zeros(count, dtype=torch.int32, device=dev)
        else:
            self.images = torch.zeros(count, self.H * self.W, self.imageInDim, device=dev)   # NHWC, what the stem's kernels read
        self.questions = torch.zeros(self.B, self.S, dtype=torch.int32, device=dev)
        self.lengths = torch.full((self.B,), self.S, dtype=torch.int32, device=dev)

    def _net_arguments(self):
        """the keyword arguments of the net's call that the static tensors stand for ({}: the call of before)"""
        named = (("image_index", self.image_index), ("kb_lengths", self.kb_lengths), ("image_lengths", self.image_lengths),
                 ("image_ids", self.image_ids))
        return {k: t for k, t in named if t is not None}

    def _net_images(self):
        """the net's `images` argument: the static image tensor, or the FeatureStore that `image_ids` names rows of"""
        return self.images if self.features is None else self.features

    def _random_images(self, gen, answers):
        """(images, questions, lengths, answers) and {"image_ids": ...} for the self-checks: _random_tower_inputs' features, or for
        a class built with features= no images and row ids with a repeat: the table's last row in the first and the last slot"""
        dev = self.questions.device
        shape = (0,) if self.features is not None else self.images.shape
        images, q, lengths, ans = _random_tower_inputs(gen, self.B, self.S, self.net.enc.vocab, shape, answers, dev)
        if self.features is None:
            return (images, q, lengths, ans), {}
        rows, count = self.features.rows, self.image_ids.shape[0]
        ids = torch.randint(0, max(rows - 1, 1), (count,), generator=gen, dtype=torch.int32)
        ids[0] = rows - 1
        ids[-1] = ids[0]
        return (None, q, lengths, ans), {"image_ids": ids.to(dev)}

    def _random_groups(self, gen):
        """(image_index, kb_lengths, image_lengths) for the self-checks, None where the class has none: an index with repeats and
        (G > 1) one image that no question names; lengths with one N and one 1"""
        index = None
        if self.G is not None:
            index = torch.randint(0, max(self.G - 1, 1), (self.B,), generator=gen, dtype=torch.int32)
            index[-1] = index[0]
        kbl = None if self.kb_lengths is None else _draw_lengths(gen, self.B, self.N)
        iml = None if self.image_lengths is None else _draw_lengths(gen, self.G, self.N)
        return index, kbl, iml

    def _load_inputs(self, images, questions, lengths, check_ids, image_index=None, kb_lengths=None, image_lengths=None, answers=None,
                     weights=None, image_ids=None):
        """A batch into the static tensors.  A class built with `weights` takes n <= B questions (n = questions.shape[0]; with
        images=G also g <= G images): every per-question argument -- lengths, answers, images (one image per question), image_index,
        kb_lengths; the training step's att_target and att_row_weights: _check_att_loss -- must have that leading size (ValueError
        naming it).
        Slots n .. B-1 of every per-question static tensor become copies of slot 0 (_pad_slots: finite and in range), their weights 0;
        image slots g .. G-1 copies of image 0 and of image_lengths[0].  A class built without `weights` refuses n != B.
        A class built with features= takes image_ids (the table rows of the batch's images, an integer tensor with the leading size
        `images` would have) and images=None; its dead slots take slot 0's id.  check_ids also tests 0 <= image_ids < rows."""
        who = type(self).__name__
        if self.features is None and image_ids is not None:
            raise ValueError("%s.load() takes no image_ids: the graph was captured without features= (a macx.FeatureStore)" % who)
        if self.features is not None and (images is not None or image_ids is None):
            raise ValueError("%s was captured with features= (a macx.FeatureStore): load() takes image_ids=, the table rows of the "
                             "batch's images, and images=None" % who)
        _lengths_argument(who, "kb_lengths", kb_lengths is not None, self.kb_lengths is not None)
        _lengths_argument(who, "image_lengths", image_lengths is not None, self.image_lengths is not None)
        per_question = [("lengths", lengths), ("answers", answers), ("image_index", image_index), ("kb_lengths", kb_lengths)]
        # (images: with one image per question, and in a class built with `weights` only -- a class built without keeps taking any
        # tensor with the static tensor's element count, e.g. [B * N, C], as it always did)
        if self.features is not None and self.G is None:
            per_question.append(("image_ids", image_ids))
        n = self._batch(questions, weights, per_question + ([("images", images)] if self.G is None and self.weights is not None else []))
        g = n if self.G is None else self.G
        if self.G is not None and self.weights is not None:
            per_image, name = (images, "images") if self.features is None else (image_ids, "image_ids")
            g = int(per_image.shape[0]) if torch.is_tensor(per_image) and per_image.dim() else 0
            if not 1 <= g <= self.G:
                raise ValueError("%s: this graph was captured for %d shared images: load() takes 1 <= g <= %d of them, got %d"
                                 % (name, self.G, self.G, g))
        if self.features is not None:
            self.features.check_ids(image_ids, g, host_check=check_ids)
        if kb_lengths is not None:
            _check_lengths(kb_lengths, n, self.N, check_ids, "kb_lengths")
        if image_lengths is not None:
            _check_lengths(image_lengths, g, self.N, check_ids, "image_lengths")
        if self.G is None and image_index is not None:
            raise ValueError("this graph was captured with one image per question (images=None): it takes no image_index")
        if self.G is not None:
            if image_index is None:
                raise ValueError("this graph was captured for %d shared images (images=%d): load() needs the [%d] image_index"
                                 % (self.G, self.G, n))
            if tuple(image_index.shape) != (n,) or image_index.dtype.is_floating_point or image_index.dtype == torch.bool:
                raise ValueError("image_index must be a [%d] integer tensor" % n)
            if check_ids and (int(image_index.max()) >= g or int(image_index.min()) < 0):
                raise IndexError("image_index outside [0, %d)" % g)
        if self.weights is None and torch.is_tensor(images) and images.numel() != self.images.numel():
            # (any layout with the static tensor's element count is taken, as always; anything else used to be a reshape error)
            raise ValueError("images: this graph was captured for %s image features and got %s: a class built with weights=True "
                             "(CapturedTowerForward: score=True) takes fewer images" % (list(self.images.shape), list(images.shape)))
        if check_ids:                          # the encoder's own validation (host synchronisation), outside the graph
            vocab = self.net.enc.vocab
            if int(questions.max()) > vocab or int(questions.min()) < 0:
                raise IndexError("question word id outside [0, %d]" % vocab)
            if int(lengths.max()) > self.S or int(lengths.min()) < 0:
                raise ValueError("question length outside [0, %d]" % self.S)
        with torch.no_grad():
            if self.features is not None:
                _pad_slots(self.image_ids, image_ids, g)
            else:
                if images.dim() == 4 and images.shape[1] == self.imageInDim and tuple(images.shape[2:]) == (self.H, self.W):
                    from .stem import k_nchw_to_nhwc          # the feed-dict layout [B, C, H, W]: transposed on the device
                    images = k_nchw_to_nhwc(images.to(self.images.device).contiguous(), self.imageInDim, self.H * self.W)
                _pad_slots(self.images, images.reshape((g,) + tuple(self.images.shape[1:])), g)
            _pad_slots(self.questions, questions, n)
            _pad_slots(self.lengths, lengths, n)
            if self.G is not None:
                _pad_slots(self.image_index, image_index, n)
            if kb_lengths is not None:
                _pad_slots(self.kb_lengths, kb_lengths, n)
            if image_lengths is not None:
                _pad_slots(self.image_lengths, image_lengths, g)
            if answers is not None:
                _pad_slots(self.answers, answers, n)
            if self.weights is not None:
                self.weights[:n] = 1.0 if weights is None else weights
                self.weights[n:] = 0.0
        self.n = n
        return n


class CapturedTowerForward(_Captured, _TowerInputs):
    """Evaluation forward of a whole macx.MACNet -- embedding + biLSTM encoder (about 100 dependent LSTM step launches), stem, cell,
    output unit + classifier, argmax -- replayed from ONE captured HIP graph on static input tensors.

        fwd = macx.CapturedTowerForward(net, B=64, S=50)
        logits = fwd(images, questions, lengths)          # [B, answers], valid until the next call; fwd.pred: int32 argmax
        att_kb = fwd.attentions["kb"]                     # the captured cell's p x [B, N] views, refreshed by every replay

    Questions that share images (an evaluation set asks many questions per image): `images=G` captures the stem on G images and
    the gather of its output into the [B, N, d] knowledge base (macx_kb_gather), which reads the static `fwd.image_index` when it
    runs -- any grouping of the B questions over the G images replays from the one graph:

        fwd = macx.CapturedTowerForward(net, B=64, S=50, images=7)
        logits = fwd(images7, questions, lengths, image_index=index)      # question b looks at images7[index[b]]

    Knowledge bases of different sizes: `kb_lengths=True` (a static [B] `fwd.kb_lengths`, MACNet.forward's kb_lengths) or, with
    images=G, `image_lengths=True` (a static [G] `fwd.image_lengths`: the captured gather is macx_kb_gather_l, which zeroes each
    question's padded rows and makes the per-question lengths on the device).  Both are read at replay time and loaded like the index:

        fwd = macx.CapturedTowerForward(net, B=64, S=50, images=7, image_lengths=True)
        logits = fwd(images7, questions, lengths, image_index=index, image_lengths=sizes)

    Image features resident in device memory: `features=store` (a macx.FeatureStore; H, W, imageInDim are the store's) captures
    the gather of the batch's images from the table (macx_features_gather) in front of the stem; it reads the static int32
    `fwd.image_ids` ([B], or [G] with images=G) when it runs, so a batch is a vector of row ids and no image crosses the bus:

        fwd = macx.CapturedTowerForward(net, B=64, S=50, features=store)
        logits = fwd(None, questions, lengths, image_ids=ids)

    Questions resident in device memory: `questions=qstore` (a macx.QuestionStore, validated once on the host) puts ONE launch
    (macx_questions_gather) in front of the encoder.  It reads the static int32 `fwd.question_ids` [B] (all -1 after construction)
    when it runs and writes every per-question static tensor -- questions, lengths, answers and weights (score=True), image_ids
    (features=), kb_lengths -- so a batch is a vector of question ids: load_ids(ids), next_batch(order) with a macx.EpochOrder, or a
    write into `question_ids`; load() is refused.  An id of -1 is a dead slot (slot 0's question under weight 0); any other id
    outside the store poisons its question (NaN logits, NaN loss) and sets `qstore.bad` (qstore.check()).  With images=G the launch
    also groups the batch by image row on the device: the [G] image_ids and image_index need no host work.  predictions=table
    (qstore.predictions()): the graph ends with macx_preds_scatter, table[question_ids[b]] = pred[b].  records=rec (a macx.EvalRecords
    over the same store, built by the caller before the capture for this run's p, N, S and answer count): behind it ONE more launch
    (macx_records_scatter) files the run's attention maps and logits in rec's tables by question id -- the reference's --getPreds /
    --getAtt output without a copy per batch; rec.read() / rec.instances() at the epoch's end.  The self-check compares the drawn ids'
    table rows between replay and eager launches bit for bit and leaves the tables cleared (NaN).  Out of scope for records=: the
    training step, the cell-level classes, towers with generic modules, several processes.  An epoch is a loop of replays:

        fwd = macx.CapturedTowerForward(net, B=64, S=50, features=store, questions=qstore, score=True, predictions=qstore.predictions())
        order = macx.EpochOrder(qstore, 64)
        for _ in range(order.steps):
            fwd.next_batch(order); fwd.replay()
        qstore.check(); result = fwd.totals.read()

    Out of scope with questions=: image_lengths=True and (training) att_loss=, whose per-image sizes / per-question targets the store
    does not hold.  The self-check draws ids (the store's last row, a repeat, a dead slot where the class has weights) and leaves
    `question_ids` all -1 and the store's `bad` word cleared.

    Evaluation only (train=False: no dropout, nothing kept for a backward pass).  Parameters are read at replay time: an optimizer
    step or a checkpoint load between calls is seen; changing a parameter's storage needs a new capture.  `load()` validates ids
    and lengths on the host as QuestionEncoder.forward does (check_ids=False skips the synchronisation); the graph itself runs
    the net with check_ids=False.  verify / captured / check() / check_every: as CapturedForward.
    Copies on the captured path: none -- every module writes into outputs it allocates from the graph's pool, the cell's final
    state and attentions are views of its `saved` buffer."""
    _WHAT = ("tower", "forward")
    _WEIGHTS_HOW = "score=True"
    answers, loss = None, None

    def __init__(self, net, B, S, H=14, W=14, imageInDim=1024, warmup=2, verify=True, check_every=0, images=None, kb_lengths=False,
                 image_lengths=False, score=False, features=None, questions=None, predictions=None, records=None):
        """score=True: the graph scores its answers -- static int32 [B] `answers`, float32 [B] `weights` (ones) and an
        output.AnswerTotals `totals`, allocated with the other inputs; the argmax launch becomes macx_answer_loss_weighted without a
        gradient, which adds every replay's weighted loss, correct count and weight to `totals`.  load() / __call__ then take
        answers= (required) and weights=, and n <= B questions (g <= G images) by _load_inputs' padding rule; __call__ returns
        logits[:n] (a view, valid until the next call), `fwd.pred` holds -1 behind the n questions, `fwd.loss` the batch's weighted
        mean, `fwd.n` is n.  An evaluation loop synchronises once per epoch:

            fwd.totals.reset()
            for images, questions, lengths, answers in batches: fwd(images, questions, lengths, answers=answers)
            result = fwd.totals.read()                # {"loss": .., "accuracy": .., "weight": ..}

        Out of scope: several processes (the totals are this process's), question length S and cell count N other than the
        capture's, and towers with generic modules (capture stays refused; the eager net.loss_and_pred(logits, answers, weights=,
        totals=) works for them, because it only sees logits).  Without score the class is what it was."""
        self._check_options(net, "CapturedTowerForward", images, kb_lengths, image_lengths, train=False)
        self._check_questions(net, "CapturedTowerForward", questions, B, S, images, kb_lengths, image_lengths, features, None, bool(score),
                              predictions, records)
        dev = _require_fused_tower(net, "CapturedTowerForward")
        self.net = net
        self.check_every = int(check_every)
        self._alloc_inputs(net, B, S, H, W, imageInDim, dev, images=images, kb_lengths=kb_lengths, image_lengths=image_lengths,
                           features=features)
        if score:
            self.answers = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self._alloc_weights(dev, True)
        else:
            self._no_answers = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._alloc_questions(questions, dev, predictions, records)
        self.graph = torch.cuda.CUDAGraph()
        self._capture(dev, warmup, self._eager, [(self.graph, self._issue)])
        try:
            self._self_check(verify)
        finally:
            self._reset_weights()                           # warm-up and verification scored their inputs: the totals start cleared
            self._reset_questions()                         # ... and gathered theirs: every slot dead, the store's bad word cleared
            if self.predictions is not None:
                self.predictions.fill_(-1)
            if self.records is not None:
                self.records.clear()

    @torch.no_grad()
    def _eager(self):
        from .output import _AnswerLoss
        self._gather_questions()                            # (questions=store: the static inputs from question_ids, one launch)
        logits = self.net(self._net_images(), self.questions, self.lengths, train=False, check_ids=False, **self._net_arguments())
        self.cell = self.net.last_cell                      # (status(): the latest run's buffers)
        if self.weights is not None:                        # score=True: the weighted call, dlogits = NULL (no_grad), one kernel
            loss, pred = self.net.loss_and_pred(logits, self.answers, **self._loss_arguments())
            self._scatter_predictions(pred)
            self._file_records(logits)
            return logits, pred, loss
        _, pred = _AnswerLoss.apply(logits, self._no_answers)          # addPredOp's argmax (first maximum), one kernel
        self._scatter_predictions(pred)
        self._file_records(logits)
        return logits, pred

    def _issue(self):
        out = self._eager()
        self.logits, self.pred = out[:2]
        if self.weights is not None:
            self.loss = out[2]
        self.attentions = self.cell.attentions

    def _replays_match_eager(self, replays=3):
        g = torch.Generator().manual_seed(20240521)
        answers = 2 if self.weights is None else self.net.out.answers
        if self.question_store is not None:                 # ids instead of questions; the gather writes the weights too
            self._draw_question_ids(g)
        else:
            (images, q, lengths, ans), ids = self._random_images(g, answers)
            self._load_inputs(images, q, lengths, False, *self._random_groups(g), answers=None if self.weights is None else ans, **ids)
            self._draw_weights()
        written = lambda: [("logits", self.logits), ("pred", self.pred)]
        clear = None
        if self.weights is not None:                        # every run adds to the totals: each starts from cleared ones
            written = lambda: [("logits", self.logits), ("pred", self.pred), ("loss", self.loss), ("totals", self.totals.tensor)]
            clear = self.totals.reset
            clear()
        filed = lambda: []
        if self.records is not None:                        # the drawn ids' rows of every table: cleared in front of every run
            live = self.question_ids[self.question_ids >= 0].long()
            # ("self": row i is its first i + 1 entries; behind them each run's own buffer holds what it held)
            filed = lambda: [("records." + name, torch.tril(t[live]) if name == "self" else t[live]) for name, t in self.records.tables.items()]
            scored, reset_totals = written, clear
            written = lambda: scored() + filed()

            def clear():
                if reset_totals is not None:
                    reset_totals()
                self.records.clear()
            clear()
        want = self._eager_on_captured([], lambda: [t.clone() for t in list(self._eager()) + ([] if self.weights is None else [self.totals.tensor])]
                                       + [t for _, t in filed()])
        return self._compare_replays(replays, written, want, before=clear)

    def load(self, images, questions, lengths, check_ids=True, image_index=None, kb_lengths=None, image_lengths=None, answers=None,
             weights=None, image_ids=None):
        """image_ids: a graph captured with features=store, and such a graph only: load(None, questions, lengths, image_ids=ids) --
        the table rows of the batch's images ([B], or [G] with images=G) in the place of `images`; passing the wrong one is a
        ValueError.  Their range is validated with the ids (check_ids).
        image_index: the [B] integer tensor of a graph captured with images=G (required there, refused otherwise); its range is
        validated with the ids (check_ids).  kb_lengths [B] / image_lengths [G]: the integer sizes of a graph captured with
        kb_lengths=True / image_lengths=True (required there, refused otherwise); 1 <= size <= N is validated with the ids.
        answers [n] / weights [n] (float32, default ones): a graph captured with score=True, and such a graph only; it takes
        n <= B questions (the constructor's docstring)"""
        self._refuse_load()
        _lengths_argument(type(self).__name__, "answers", answers is not None, self.answers is not None, "score=True")
        return self._load_inputs(images, questions, lengths, check_ids, image_index, kb_lengths, image_lengths, answers, weights,
                                 image_ids)

    def replay(self):
        if self.captured:
            self.graph.replay()
        else:                                               # (module docstring: slower where the host is slow, never wrong)
            self._issue()
        self._count_replay()
        return self.logits if self.weights is None else self.logits[:self.n]

    def __call__(self, images, questions, lengths, check_ids=True, image_index=None, kb_lengths=None, image_lengths=None, answers=None,
                 weights=None, image_ids=None):
        self.load(images, questions, lengths, check_ids, image_index, kb_lengths, image_lengths, answers, weights, image_ids)
        return self.replay()


def _check_step_bucket(who, net, opt, bucket):
    """what the tower's training steps require of their bucket and optimizer"""
    if not getattr(bucket, "fused_gather", False):
        raise ValueError("%s needs TowerBuckets(net, fused_gather=True): per-tensor copy_ gathers become memcpy "
                         "nodes, which graph replay does not keep in stream order" % who)
    if bucket.net is not net:
        raise ValueError("the bucket was built over another net")
    own = bucket.tensors()
    if len(opt.params) != len(own) or any(a is not b for a, b in zip(opt.params, own)) or opt.flat.numel() != bucket.flat.numel():
        raise ValueError("the optimizer must be built over bucket.tensors() (FlatAdamEMA(bucket.tensors(), ...)): it steps on "
                         "bucket.flat as it is")


class CapturedTowerTrainStep(_Captured, _TowerInputs, _MaskWord):
    """One whole training step of a macx.MACNet replayed from ONE captured HIP graph: forward (train-mode dropout), mean CE loss,
    backward, the gather of every gradient into the tower's flat buffer, global-norm clip + Adam + EMA.

        bucket = macx.dp.TowerBuckets(net, fused_gather=True)
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4)
        step = macx.CapturedTowerTrainStep(net, opt, bucket, B=64, S=50, H=14, W=14, imageInDim=1024, seed=1234)
        for it in range(steps):
            step.load(images, questions, lengths, answers)
            step.replay(iteration=it)                     # step.loss, step.logits, step.pred, step.norm

    Three things a capture would otherwise freeze travel through device memory and are written by replay(), outside the graph:
    the dropout masks -- every site of the tower (encoder, stem, cell, classifier) XORs `step.mask_word` into its key when the
    kernel runs, replay(iteration=i) sets it to mix32(i), replay() keeps it; the optimizer's bias-corrected rate -- opt.advance()
    counts the step and writes lr * sqrt(1 - b2^t) / (1 - b1^t) from the CURRENT opt.lr (so --lrReduce is followed); and the
    inputs (`load`, which also runs the encoder's id / length validation on the host; check_ids=False skips that sync).

    The graph holds exactly what the eager step issues: net(..., train=True, check_ids=False, mask_word=...), loss_and_pred,
    bucket.begin_step / allreduce_(B, B) for this one process (macx_gather_flat: one launch per gather, its table uploaded after
    the capture) and opt.step(flat_grad=bucket.flat, device_lr=True).  Data parallelism over several processes is not captured
    here: CapturedDPTowerTrainStep cuts this step at its collectives (CapturedDPTrainStep is the cell-level route).  `opt` must be
    built over bucket.tensors(), `bucket` with fused_gather=True.

    images=G / kb_lengths=True / image_lengths=True: CapturedTowerForward's (load() takes image_index / kb_lengths / image_lengths
    accordingly).  With images=G the stem runs once per image and the gather and its backward (macx_kb_gather[_l] / _bwd[_l]) are
    part of the graph; a stem that drops (stemDropout < 1) is refused at construction with the eager path's ValueError.
    features=store: CapturedTowerForward's (load(None, questions, lengths, answers, image_ids=ids); the gather from the table is
    part of the graph and takes no gradient; with weights=True dead slots take slot 0's id).
    questions=qstore: CapturedTowerForward's (the store must hold answers; load_ids(ids) / next_batch(order) in the place of load(),
    a short batch only with weights=True; the gather from the question tables is the first launch of the graph).

    verify=True replays three times against the eager step on random inputs -- loss, logits, pred, norm, the flat gradient, every
    parameter, m, v, ema -- each time from the same restored state, and falls back to eager launches when anything differs
    (`captured` False, a RuntimeWarning; `verify_report` lists what differed).  Parameters, m, v, ema and t are restored
    afterwards: a constructed step has not trained.

    A guarded optimizer (FlatAdamEMA(..., guard=True)): the graph's last launch is the guarded update, which skips the step ON THE
    DEVICE when the gradient norm is not finite (a poisoned question id or feature row, a hand-off that gave up) or above
    skip_above: parameters, m, v and ema keep every bit, the skip is counted, and the next replay trains on sound weights.  The
    guard words are optimizer state here -- saved and restored around warm-up and verification with m and v, compared between replay
    and eager step by the self-check -- so a constructed step reads opt.guard_counts() == (0, 0, 0, 0).  Read the counts once per
    epoch, next to the other once-per-epoch reads: qs.check(); opt.guard_counts().  opt.t and the rate count attempts, skipped ones
    included (FlatAdamEMA).  A NaN loss is still added to `totals`: that is the documented signal, the guard only protects the
    weights.  Several processes need nothing more: the decision is taken on bucket.flat AFTER the all-reduce, every rank holds
    the same reduced buffer, so every rank skips or applies alike.  An unguarded optimizer: the launches and bits of before.

    att_loss= / aux_loss=: CapturedTrainStep's, on net.last_cell.  The loss the step trains on becomes CE + aux with
    aux = lam * sum(aux_rows) / (p * B) (+ aux_loss(cell, state)): `step.loss` is the total, `step.ce` the mean cross-entropy,
    `step.aux` the auxiliary part (None for a class built without either; then loss is ce).  on="kb" masks by the lengths the cell ran
    under: the static kb_lengths, or with image_lengths=True the per-question tensor the captured gather makes on the device.
    load(..., att_target=, att_row_weights=, att_step_weights=) as CapturedTrainStep.load.  Optimizer, bucket and the restore logic
    are the same; a weight of 0 trains exactly as the class without att_loss.

    Copies on the captured path: none issued by the library or by this class.  What autograd adds is torch's own business: it
    adopts each returned gradient as the parameter's .grad without a copy as long as nobody else holds it (the module functions
    return fresh tensors), and sums the two gradients of vecQuestions with a kernel.

    weights=True: per-question answer weights and partial batches from the ONE graph.  A static float32 [B] `step.weights` (ones) is
    allocated with the other inputs and read by the loss kernel when it runs (macx_answer_loss_weighted in the place of
    macx_answer_loss: one launch for one launch, no timing is claimed); the step trains on the weighted mean
    sum_live w_b l_b / sum_live w_b -- all ones: the mean.  load(..., weights=) takes n <= B questions (n = questions.shape[0]; with
    images=G also g <= G images): slots n .. B-1 of every per-question static tensor become copies of slot 0, so they stay finite and in
    range and the graph runs the same launches, and their weights become 0 -- the loss kernel does not read a dead question's logits or
    answer and writes an all +0 gradient row, every backward consumer is linear in that row, so no parameter gradient, loss or
    prediction depends on what the dead slots hold.  `step.loss` / `step.ce` are the weighted means, `step.pred` holds -1 in
    dead slots, `step.n` is n.  With att_loss the att_row_weights of the dead slots become 0 and att_row_weights=None means ones for the
    n questions; the attention loss keeps its p * B normaliser (a short batch's auxiliary part is not rescaled to n).
    totals=True (or an output.AnswerTotals to adopt): every replay adds its weighted loss, correct count and weight to `step.totals`,
    read with one synchronisation per epoch (totals.read()); construction leaves it cleared.
    The self-check draws weights too (one 0, one fraction, the rest ones).  Built without weights the class issues the launches it
    always issued and refuses n != B.  Out of scope: several processes (with global_batch != B the weighted mean would need W summed over
    the ranks: a bucket that spans more than one process is refused with weights=True -- CapturedDPTowerTrainStep(weights=True) is
    the class that sums it), the cell-level classes (their caller owns
    d_memory), S and N other than the capture's, and towers with generic modules (capture stays refused as it is; the eager
    net.loss_and_pred(logits, answers, weights=) works for them, because it only sees logits)."""

    aux = None

    def __init__(self, net, opt, bucket, B, S, H=14, W=14, imageInDim=1024, seed=0, warmup=2, verify=True, check_every=0, images=None,
                 kb_lengths=False, image_lengths=False, att_loss=None, aux_loss=None, weights=False, totals=None, features=None, questions=None):
        self._check_options(net, "CapturedTowerTrainStep", images, kb_lengths, image_lengths, train=True)
        att_loss = _att_loss_spec("CapturedTowerTrainStep", att_loss)
        self._check_questions(net, "CapturedTowerTrainStep", questions, B, S, images, kb_lengths, image_lengths, features, att_loss, True)
        self._check_totals("CapturedTowerTrainStep", weights, totals)
        if weights and getattr(bucket, "_active", lambda: False)():
            raise ValueError("CapturedTowerTrainStep(weights=True): the bucket spans more than one process; the weighted mean over a "
                             "global batch needs the weights summed over the ranks, which the step does not do")
        dev = _require_fused_tower(net, "CapturedTowerTrainStep")
        _check_step_bucket("CapturedTowerTrainStep", net, opt, bucket)
        self.net, self.opt, self.bucket, self.seed = net, opt, bucket, int(seed)
        self.check_every = int(check_every)
        self._alloc_inputs(net, B, S, H, W, imageInDim, dev, images=images, kb_lengths=kb_lengths, image_lengths=image_lengths,
                           features=features)
        self.answers = torch.zeros(self.B, dtype=torch.int32, device=dev)
        if weights:
            self._alloc_weights(dev, totals)
        self._alloc_att_loss(att_loss, net.netLength, self.B, self.S, self.N, dev)
        self.aux_loss = aux_loss
        self._alloc_mask_word(dev)
        self._alloc_questions(questions, dev)
        self.norm = opt.norm
        state = self._state()
        self.graph = torch.cuda.CUDAGraph()

        def warm():
            opt.advance()
            self._eager()
        self._capture(dev, warmup, warm, [(self.graph, self._issue)], before=self._clear_grads)
        try:
            self._self_check(verify, state)
        finally:
            self._reset_weights()                           # ... and scored them: weights back to ones, the totals cleared
            self._reset_questions()
        self._restore(state)                                # warm-up (and verification) trained on zeros: undo

    def _after_capture(self):
        self.bucket.flush_tables()                          # the gathers' tables, which a capture can only point at (dp.TowerBuckets)
        super()._after_capture()

    # ---- the optimizer's state, saved and restored around warm-up and verification
    def _buffers(self):
        """(the guard words of a guarded optimizer are state like m and v: warm-up and verification must not count as attempts)"""
        o = self.opt
        return [b for b in (o.flat, o.m, o.v, o.ema, getattr(o, "guard", None)) if b is not None]

    def _state(self):
        return [b.clone() for b in self._buffers()], self.opt.t, self.opt.lr_t.clone()

    def _restore(self, state):
        bufs, t, lr_t = state
        with torch.no_grad():
            for b, s in zip(self._buffers(), bufs):
                b.copy_(s)
            self.opt.lr_t.copy_(lr_t)
        self.opt.t = t

    def _clear_grads(self):
        for t in self.bucket.tensors():
            t.grad = None

    def _eager(self):
        """the step's launches on the current stream (opt.advance() is the caller's: it is not part of the graph)"""
        self._clear_grads()
        net, B = self.net, self.B
        self._gather_questions()                            # (questions=store: the static inputs from question_ids, one launch)
        logits = net(self._net_images(), self.questions, self.lengths, train=True, seed=self.seed, check_ids=False, mask_word=self.mask_word,
                     **self._net_arguments())
        self.cell = net.last_cell
        ce, pred = net.loss_and_pred(logits, self.answers, **self._loss_arguments())
        loss, aux = ce, None
        if self.att_loss is not None or self.aux_loss is not None:
            cell, p = self.cell, net.netLength
            state = MACCellTuple(cell.state_tensor("controls")[p], cell.state_tensor("memories")[p])      # the run's final state
            terms = self._aux_terms(cell, state)
            aux = terms[0] if len(terms) == 1 else terms[0] + terms[1]
            loss = ce + aux
        self.bucket.begin_step(B, B)
        loss.backward()
        self.bucket.allreduce_(B, B)                        # one process: the gather; nothing is exchanged
        self.opt.step(flat_grad=self.bucket.flat, device_lr=True)
        self._parts = (ce.detach(), None if aux is None else aux.detach())
        return loss.detach(), logits.detach(), pred

    def _issue(self):
        self.loss, self.logits, self.pred = self._eager()
        self.ce, self.aux = self._parts

    def _stepped(self):
        """what a step writes besides its outputs"""
        return [self.opt.norm, self.bucket.flat] + self._buffers()

    def _eager_reference(self):
        """the eager step from the optimizer's state as it is: clones of loss, logits, pred and _stepped(); the captured `.grad`
        tensors and `cell` are put back (CapturedTrainStep.eager_reference)"""
        return self._eager_on_captured(self.bucket.tensors(),
                                       lambda: [t.clone() for t in list(self._eager()) + self._stepped() + self._aux_written(self._parts[1])])

    def _aux_written(self, aux):
        """what a step with an auxiliary loss writes besides: the auxiliary part, and the rows of att_loss; what a step with totals
        adds to"""
        return (([] if aux is None else [aux]) + ([] if self.aux_rows is None else [self.aux_rows])
                + ([] if self.totals is None else [self.totals.tensor]))

    def _replays_match_eager(self, state, replays=3):
        g = torch.Generator().manual_seed(20240522)
        if self.question_store is not None:                 # ids instead of questions; the gather writes answers and weights too
            self._draw_question_ids(g)
        else:
            (images, q, lengths, ans), ids = self._random_images(g, self.net.out.answers)
            index, kbl, iml = self._random_groups(g)
            self._load_inputs(images, q, lengths, False, index, kbl, iml, **ids)
            self.answers.copy_(ans)
            if self.att_loss is not None:
                live = kbl if iml is None else iml[index.long()]     # the per-question sizes the gather makes on the device
                self._randomise_att_loss(g, live if self.att_loss["on"] == "kb" else lengths.cpu())
            self._draw_weights()
        self.set_mask_word(0x5bd1e995)                      # a non-trivial word: the check covers the device-read path as well

        def from_state():                                   # the eager step and every replay start from the same state
            self._restore(state)
            self.opt.advance()
            if self.totals is not None:
                self.totals.reset()
        from_state()
        want = self._eager_reference()
        names = ["loss", "logits", "pred", "norm", "flat_grad", "params", "m", "v"] + (["ema"] if self.opt.ema is not None else [])
        names += ["guard"] if getattr(self.opt, "guard", None) is not None else []
        names += ([] if self.aux is None else ["aux"]) + ([] if self.aux_rows is None else ["aux_rows"])
        names += [] if self.totals is None else ["totals"]
        written = lambda: zip(names, [self.loss, self.logits, self.pred] + self._stepped() + self._aux_written(self.aux))
        return self._compare_replays(replays, written, want, before=from_state)

    def load(self, images, questions, lengths, answers, check_ids=True, image_index=None, kb_lengths=None, image_lengths=None,
             att_target=None, att_row_weights=None, att_step_weights=None, weights=None, image_ids=None):
        """image_index / kb_lengths / image_lengths / image_ids: CapturedTowerForward.load's (image_ids: a class built with
        features=store takes load(None, questions, lengths, answers, image_ids=ids)); att_target / att_row_weights / att_step_weights:
        CapturedTrainStep.load's (a class built with att_loss=).
        weights: a class built with weights=True, and such a class only: [n] float32 (default ones).  Such a class takes n <= B
        questions -- every per-question argument (lengths, answers, images or image_index, kb_lengths, att_target, att_row_weights)
        with that leading size -- by the padding rule of the class docstring; a class built without refuses n != B.  Returns n."""
        self._refuse_load()
        self._refuse_other_size(questions)                  # (ahead of the att_* shapes: a short batch is the first thing to say)
        short = self.weights is not None and torch.is_tensor(questions) and questions.dim() == 2
        n = int(questions.shape[0]) if short else None
        self._check_att_loss(att_target, att_row_weights, att_step_weights, n)
        n = self._load_inputs(images, questions, lengths, check_ids, image_index, kb_lengths, image_lengths, answers, weights, image_ids)
        self._copy_att_loss(att_target, att_row_weights, att_step_weights, n if self.weights is not None else None)
        return n

    def replay(self, iteration=None):
        """iteration: None keeps the current mask word; an int draws the masks of word mix32(iteration).  Counts the optimizer's
        step and refreshes its rate from opt.lr (opt.advance()), then replays."""
        self._set_iteration(iteration)
        self.opt.advance()
        if self.captured:
            self.graph.replay()
        else:
            self._issue()
        self._count_replay()
        return self.loss


class CapturedDPTowerTrainStep(_Captured, _TowerInputs, _MaskWord, TowerExchangeStep):
    """One DATA-PARALLEL training step of a whole macx.MACNet as two or three graph replays with the collectives between them
    (dp.TowerExchangeStep's sequence; this class supplies the parts):

        [ graph Q: W_r, the shard's live weight, into w_local and w_global ]   [ sum all-reduce of that one double ]   weights=True only
          graph A: forward, loss, backward, the gather into the flat buffer      sum all-reduce of the flat buffer
          graph B: global-norm clip + Adam + EMA on the reduced buffer

    No kernel is new: the graphs replay the launches the eager data-parallel step issues (about 200 per rank), and the weighted
    arithmetic is dp.py's torch ops on 1-element device tensors.  What the class buys is the host: a shard of 8 questions is bound
    by the launch rate, not by the GPU.  Nothing here has been measured on more than one GPU (profiles/tower_dp_ab.txt is one
    process).  One process: no collective at all, and with B == global_batch the bits of CapturedTowerTrainStep.

        bucket = macx.dp.TowerBuckets(net, fused_gather=True, exchange=False)       # the step owns the collectives
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-4)
        lo, hi = macx.dp.tower_slice(64, rank, world)
        step = macx.CapturedDPTowerTrainStep(net, opt, bucket, B=hi - lo, S=50, global_batch=64, b0=lo, seed=1234)
        step.load(images[lo:hi], questions[lo:hi], lengths[lo:hi], answers[lo:hi])
        step.step(iteration=it)              # step.loss, .ce, .logits, .pred, .norm; every rank holds the same parameters

    Part A runs net(..., train=True, seed=seed, b0=b0, check_ids=False, mask_word=...) -- b0 is the shard's first global slot, so the
    ranks draw the masks of the full batch -- then net.loss_and_pred, backward and bucket.gather_.  Unweighted it trains on the
    shard's mean and gather_(B, global_batch) scales the buffer by B / global_batch in front of the reduce, as GradBucket does.
    Part B is opt.step(flat_grad=bucket.flat, device_lr=True); opt.advance() and the mask word are step()'s, outside the graphs.  A
    guarded optimizer decides on the reduced buffer, so every rank decides alike.

    After a step: `loss` is this rank's TERM of the global mean (the ranks' terms sum to it: ce * B / global_batch, or weighted
    ce * W_r / W_g), `ce` the shard's own (weighted) mean, `logits`, `pred`, `norm` (of the reduced gradient, the same on every
    rank), `n`, and with totals= this rank's `totals` (dp.reduce_totals sums them, once per epoch).

    weights=True: per-question answer weights and short global batches.  Graph Q writes W_r with kernels into both sums, the
    all-reduce makes w_global W_g, and part A trains on ce * factor() -- the fp64 quotient W_r / W_g cast to fp32 on the device -- and
    calls gather_(1, 1): the factor carries the weight, the buffer is not rescaled.  load() then takes the shard's
    n_r = dp.shard_count(n, lo, hi) <= B questions (CapturedTowerTrainStep.load's padding rule); a shard without a live question
    calls load_dead() and still steps: its buffer is all +0 in front of the reduce, its loss +0, and it issues the same collectives.

    Warm-up, capture and verify=True are local -- construction issues no collective.  The self-check runs Q, A, B back to back with
    w_global = w_local (graph Q writes both) and compares replays with the eager parts over loss, ce, logits, pred, norm, the flat
    gradient, parameters, m, v, ema, guard and totals, each time from the same restored state; a rank whose replays differ falls back
    to the eager parts (`captured` False, a RuntimeWarning) and keeps issuing the same collectives.  capture=False builds that
    eager-parts step directly.  All graphs share one pool.

    images=G / kb_lengths=True / image_lengths=True / features=store / totals= / check_every=: CapturedTowerTrainStep's, per rank.
    Refused: att_loss= / aux_loss= (their p * B normaliser needs a rule for shards) and questions=store (its gather writes the
    weights, so it would have to move in front of graph Q)."""
    _loaded = False
    # the optimizer's state around warm-up and verification, and the cleared .grad tensors: the one-process step's
    _buffers, _state, _restore = CapturedTowerTrainStep._buffers, CapturedTowerTrainStep._state, CapturedTowerTrainStep._restore
    _clear_grads = CapturedTowerTrainStep._clear_grads

    def __init__(self, net, opt, bucket, B, S, H=14, W=14, imageInDim=1024, global_batch=None, b0=0, group=None, seed=0, warmup=2,
                 capture=True, verify=True, check_every=0, images=None, kb_lengths=False, image_lengths=False, att_loss=None, aux_loss=None,
                 weights=False, totals=None, features=None, questions=None):
        who = "CapturedDPTowerTrainStep"
        for name, given in (("att_loss", att_loss), ("aux_loss", aux_loss)):
            if given is not None:
                raise ValueError("%s takes no %s: the auxiliary loss is normalised by p * B, and which B a shard of a global batch "
                                 "divides by is not settled; CapturedTowerTrainStep takes it in one process" % (who, name))
        if questions is not None:
            raise ValueError("%s takes no questions= store: its gather writes the weights, so it would have to move in front of the "
                             "graph that sums them (part Q); load() the shard's questions" % who)
        self._check_options(net, who, images, kb_lengths, image_lengths, train=True)
        self._check_totals(who, weights, totals)
        global_batch = int(B if global_batch is None else global_batch)
        if not (1 <= int(B) and 0 <= int(b0) and int(b0) + int(B) <= global_batch):
            raise ValueError("%s: the shard holds the global slots [b0, b0 + B) = [%d, %d) of a global batch of %d"
                             % (who, int(b0), int(b0) + int(B), global_batch))
        dev = _require_fused_tower(net, who)
        _check_step_bucket(who, net, opt, bucket)
        if getattr(bucket, "exchange", True):
            raise ValueError("%s needs TowerBuckets(net, fused_gather=True, exchange=False): the step issues the collectives between "
                             "its graphs, and a bucket that exchanges from the cell's phase-1 hook would issue one inside part A" % who)
        self.net, self.opt, self.bucket = net, opt, bucket
        self.seed, self.b0, self.global_batch = int(seed), int(b0), global_batch
        self.check_every = int(check_every)
        self._alloc_inputs(net, B, S, H, W, imageInDim, dev, images=images, kb_lengths=kb_lengths, image_lengths=image_lengths,
                           features=features)
        self.answers = torch.zeros(self.B, dtype=torch.int32, device=dev)
        sums = [None, None]
        if weights:
            self._alloc_weights(dev, totals)
            sums = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(2)]      # W_r and W_g: before the capture
        self._alloc_mask_word(dev)
        TowerExchangeStep.__init__(self, bucket.flat, group if group is not None else bucket.group, *sums)
        self.shard_weight = float(self.B) / float(global_batch)
        self.norm = opt.norm
        state = self._state()
        bodies = ([self._part_q] if weights else []) + [self._part_a, self._part_b]
        self.graphs = {body: torch.cuda.CUDAGraph() for body in bodies} if capture else {}
        graphs = [(self.graphs[body], body) for body in bodies if capture]

        def warm():
            opt.advance()
            self._eager_parts()
        self._capture(dev, warmup, warm, graphs, before=self._clear_grads)
        try:
            if capture:
                self._self_check(verify, state)
        finally:
            self._reset_weights()                           # warm-up and verification scored their inputs
        self._restore(state)                                # ... and trained on them: undo

    def _after_capture(self):
        self.bucket.flush_tables()                          # the gather's table, which a capture can only point at (dp.TowerBuckets)
        _Captured._after_capture(self)

    # ---- the parts: their launches on the current stream (the bodies of the captures and the eager fallback)
    def _part_q(self):
        """both sums with kernels (out=): a copy_ from one to the other would be a memcpy node (dp.TowerBuckets)"""
        live_weight_sum(self.weights, self.w_local)
        live_weight_sum(self.weights, self.w_global)

    def _eager_a(self):
        """part A's launches on the current stream: (loss term, ce, logits, pred)"""
        self._clear_grads()
        net = self.net
        logits = net(self._net_images(), self.questions, self.lengths, train=True, seed=self.seed, b0=self.b0, check_ids=False,
                     mask_word=self.mask_word, **self._net_arguments())
        self.cell = net.last_cell                           # (status(): the latest run's buffers)
        ce, pred = net.loss_and_pred(logits, self.answers, **self._loss_arguments())
        if self.w_global is not None:
            loss = ce * self.factor().to(torch.float32).reshape(ce.shape)
            loss.backward()
            self.bucket.gather_(1, 1)                       # the factor carries the weight: the buffer is not rescaled
            term = loss.detach()
        else:
            ce.backward()
            self.bucket.gather_(self.B, self.global_batch)
            term = ce.detach() if self.shard_weight == 1.0 else ce.detach() * self.shard_weight
        return term, ce.detach(), logits.detach(), pred

    def _part_a(self):
        """... published: the body of graph A and of the eager fallback (the self-check's reference run publishes nothing, so the
        attributes stay the tensors the graph writes)"""
        self.loss, self.ce, self.logits, self.pred = self._eager_a()

    def _part_b(self):
        self.opt.step(flat_grad=self.bucket.flat, device_lr=True)

    def _eager_parts(self, part_a=None):
        """Q, A, B back to back without a collective: graph Q has written W_r into w_global as well, so the factor is 1 (or 0).
        Returns what part_a (default: _part_a) returns."""
        if self.w_global is not None:
            self._part_q()
        out = (part_a or self._part_a)()
        self._part_b()
        return out

    def _run_part(self, body):
        if self.captured:
            self.graphs[body].replay()
        else:
            body()

    def run_part_q(self):
        self._run_part(self._part_q)

    def run_part_a(self):
        self._run_part(self._part_a)

    def run_part_b(self):
        self._run_part(self._part_b)

    def _local_step(self):
        """_eager_parts through run_part_*: what the self-check replays"""
        if self.w_global is not None:
            self.run_part_q()
        self.run_part_a()
        self.run_part_b()

    # ---- the self-check
    def _written(self, outputs=None):
        """(label, tensor) of what a step writes; outputs: part A's four of another run than the published one"""
        o = self.opt
        named = list(zip(("loss", "ce", "logits", "pred"), outputs or (self.loss, self.ce, self.logits, self.pred)))
        named += [("norm", o.norm), ("flat_grad", self.bucket.flat), ("params", o.flat), ("m", o.m), ("v", o.v), ("ema", o.ema),
                  ("guard", getattr(o, "guard", None)), ("totals", None if self.totals is None else self.totals.tensor),
                  ("w_local", self.w_local), ("w_global", self.w_global)]
        return [(name, t) for name, t in named if t is not None]

    def _replays_match_eager(self, state, replays=3):
        g = torch.Generator().manual_seed(20240523)
        (images, q, lengths, ans), ids = self._random_images(g, self.net.out.answers)
        self._load_inputs(images, q, lengths, False, *self._random_groups(g), **ids)
        self.answers.copy_(ans)
        self._draw_weights()
        self.set_mask_word(0x5bd1e995)                      # a non-trivial word: the check covers the device-read path as well

        def from_state():                                   # the eager parts and every replay start from the same state
            self._restore(state)
            self.opt.advance()
            if self.totals is not None:
                self.totals.reset()

        def reference():
            return [t.clone() for _, t in self._written(self._eager_parts(self._eager_a))]
        from_state()
        want = self._eager_on_captured(self.bucket.tensors(), reference)
        return self._compare_replays(replays, self._written, want, before=from_state, replay=self._local_step)

    # ---- batches
    def load(self, images, questions, lengths, answers, check_ids=True, image_index=None, kb_lengths=None, image_lengths=None,
             weights=None, image_ids=None):
        """CapturedTowerTrainStep.load on this rank's shard: B questions, or in a class built with weights=True the shard's
        n_r = dp.shard_count(n, lo, hi) questions with 1 <= n_r <= B (n_r == 0: load_dead()).  Returns n_r."""
        n = CapturedTowerTrainStep.load(self, images, questions, lengths, answers, check_ids, image_index, kb_lengths, image_lengths,
                                        weights=weights, image_ids=image_ids)
        self._loaded = True
        return n

    def load_dead(self):
        """A shard without a live question (weights=True): every weight 0.  The per-question inputs stay what the last load() left;
        if there never was one they become ONE valid placeholder -- word id 1, length 1, answer 0, zero image features or image id 0
        -- because a dead row must stay finite: its gradient row is +0, but 0 * NaN in a weight-gradient contraction is NaN."""
        if self.weights is None:
            raise TypeError("%s.load_dead() belongs to a class built with weights=True" % type(self).__name__)
        with torch.no_grad():
            if not self._loaded:
                self.questions.zero_()
                self.questions[:, 0] = 1
                self.lengths.fill_(1)
                self.answers.zero_()
                for t in (self.images, self.image_ids, self.image_index):
                    if t is not None:
                        t.zero_()
                for t in (self.kb_lengths, self.image_lengths):
                    if t is not None:
                        t.fill_(self.N)
            self.weights.zero_()
        self.n = 0
        return 0

    def step(self, iteration=None):
        """one data-parallel step: the mask word (iteration: None keeps it, an int draws the masks of mix32(iteration)),
        opt.advance(), the parts and collectives of dp.TowerExchangeStep.exchange_step().  Returns this rank's loss term."""
        self._set_iteration(iteration)
        self.opt.advance()
        self.exchange_step()
        self._count_replay()
        return self.loss
