"""MACCell -- the host-side mirror of the reference's recurrent cell (mac_cell.py:30-592) over
libmacx.so.

Same constructor arguments, `zero_state`, per-step `__call__`, `.iteration`, `.attentions`,
`.controls/.memories/.infos` as the reference class, so the loop of model.py:453-458 runs
unchanged:

    cell = MACCell(vecQuestions=..., questionWords=..., questionCntxWords=..., questionLengths=...,
                   knowledgeBase=..., memoryDropout=..., readDropout=..., writeDropout=...,
                   batchSize=B, train=True, config=config, params=params)
    state = cell.zero_state(B)
    for i in range(config.netLength):
        cell.iteration = i
        _, state = cell(none, state)

All arithmetic runs in hand-written HIP kernels behind the C ABI of include/macx.h; PyTorch only
owns the device memory and the stream.  There is no CPU or eager fallback: without a loadable
libmacx.so or without a HIP device every entry point raises.
"""
import collections
import ctypes as C
import weakref

import torch

from . import _lib
from .options import freeze, fresh_seed, get
from .params import FlatLayout, MACCellParams
from .unit import _f32c, _kb_lengths, _mask_word

MACCellTuple = collections.namedtuple("MACCellTuple", ("control", "memory"))   # mac_cell.py:8


class _Run:
    """One cell run: shapes, frozen options, buffers, and the ctypes structs that describe them."""

    def __init__(self, cell, keep_activations):
        # the cell's device tensors this run's structs point at, held here: the backward pass of this run may outlive the cell.  NOT
        # the cell itself -- the cell holds the outputs of this run's autograd node (its differentiable histories and attention
        # maps), the node holds the run, and a reference back would close a cycle through the autograd graph that the garbage
        # collector cannot see: every run's `saved` buffer would stay allocated
        self.vecQuestions, self.words, self.knowledgeBase = cell.vecQuestions, cell.words, cell.knowledgeBase
        self.questionLengths, self.mask_word = cell.questionLengths, cell.mask_word
        self._cell_ref = weakref.ref(cell)      # (weak: only to tell the cell that this run's backward pass is over)
        self.keep = int(bool(keep_activations))
        self.L = _lib.lib()
        self.opts = cell.opts
        B, S, d = cell.words.shape
        N = cell.knowledgeBase.shape[1]
        self.shapes = _lib.MacxShapes(B=B, S=S, N=N, d=d, p=cell.netLength, b0=cell.b0, d_logical=int(getattr(cell, "d_logical", 0)))
        _lib.check(self.L.macx_check(C.byref(self.opts), C.byref(self.shapes)), "macx_check")
        self.drop = _lib.MacxDropout(keep_memory=cell.dropouts["memory"], keep_read=cell.dropouts["read"],
                                     keep_write=cell.dropouts["write"], seed=cell.seed & 0xFFFFFFFF,
                                     mask_word=cell.mask_word.data_ptr() if cell.mask_word is not None else None)
        dev = cell.knowledgeBase.device
        self.saved_floats = self.L.macx_saved_floats(C.byref(self.opts), C.byref(self.shapes), self.keep)
        self.saved = torch.empty(self.saved_floats, dtype=torch.float32, device=dev)
        self.ws_fwd = torch.empty(max(4, self.L.macx_ws_floats(C.byref(self.opts), C.byref(self.shapes), 0)),
                                  dtype=torch.float32, device=dev)
        self.params = cell.params
        self.pstruct = _lib.MacxParams()
        self._ptensors = {}
        for f in _lib.PARAM_FIELDS:
            t = getattr(self.params, f, None) if f in self.params.fields else None
            if t is not None:
                t = _f32c(t.detach(), f)
                self._ptensors[f] = t
            setattr(self.pstruct, f, t.data_ptr() if t is not None else None)
        self.inputs = _lib.MacxInputs(vecQuestions=cell.vecQuestions.data_ptr(), words=cell.words.data_ptr(),
                                      questionLengths=cell.questionLengths.data_ptr(),
                                      knowledgeBase=cell.knowledgeBase.data_ptr(),
                                      kbLengths=cell.kb_lengths.data_ptr() if cell.kb_lengths is not None else None)
        self.kb_lengths = cell.kb_lengths          # held here: the backward pass of this run may outlive the cell
        self.stream = _lib.stream_of(dev)
        # the hand-off status words of `saved` are sticky (macx_run_status): zero them once, here.  Not inside a graph capture -- the
        # status must survive replays -- so a run allocated under capture is reset by its capturer afterwards (graph.py)
        self.status_reset_pending = torch.cuda.is_current_stream_capturing()
        if not self.status_reset_pending:
            self.reset_status()

    def _status_args(self):
        return (C.byref(self.opts), C.byref(self.shapes), self.keep, _lib.ptr(self.saved), C.c_size_t(self.saved_floats))

    def reset_status(self):
        """zero the run's hand-off status words: asynchronous, on torch's current stream (the run's own when it is allocated)"""
        stream = _lib.stream_of(self.saved)
        _lib.check(self.L.macx_run_status_reset(*self._status_args(), stream), "macx_run_status_reset")
        self.status_reset_pending = False

    def status(self):
        """(bits, first_step) of macx_run_status: (0, -1) when every in-launch hand-off of the runs on this buffer completed.
        Synchronises torch's current stream."""
        bits, first = C.c_uint32(0), C.c_int32(-1)
        stream = _lib.stream_of(self.saved)
        rc = self.L.macx_run_status(*self._status_args(), stream, C.byref(bits), C.byref(first))
        if rc not in (_lib.MACX_OK, _lib.MACX_EWAIT):
            raise _lib.MacxError(rc, "macx_run_status")
        return int(bits.value), int(first.value)

    def check(self, where="MAC cell run"):
        bits, first = self.status()
        if bits:
            raise _lib.HandoffTimeout(bits, first, where)

    def _common(self):
        return (C.byref(self.opts), C.byref(self.shapes), C.byref(self.drop), C.byref(self.pstruct), C.byref(self.inputs),
                _lib.ptr(self.saved), C.c_size_t(self.saved_floats), _lib.ptr(self.ws_fwd), C.c_size_t(self.ws_fwd.numel()))

    def begin(self):
        _lib.check(self.L.macx_cell_begin(*self._common(), self.keep, self.stream), "macx_cell_begin")

    def step(self, i):
        _lib.check(self.L.macx_cell_step(*self._common(), self.keep, int(i), self.stream), "macx_cell_step")

    def forward(self):
        _lib.check(self.L.macx_cell_forward(*self._common(), self.keep, self.stream), "macx_cell_forward")

    def segment(self, name, shape, alias=False):
        """a viewable segment of `saved` as a tensor of `shape`.  alias=True: a tensor of its own on the same memory instead of a
        view of `saved` (no copy, no launch) -- what the autograd node returns: autograd tracks in-place writes per base tensor, and
        a torch-level write anywhere into `saved` (the status words, say) would otherwise invalidate every output of the node."""
        off, cnt = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self.L.macx_saved_segment(C.byref(self.opts), C.byref(self.shapes), self.keep, _lib.SEG[name],
                                             C.byref(off), C.byref(cnt)), "macx_saved_segment")
        n = 1
        for x in shape:
            n *= x
        if n > cnt.value:
            raise ValueError("segment %s holds %d floats, view wants %d" % (name, cnt.value, n))
        if alias:
            t = torch.empty(0, dtype=torch.float32, device=self.saved.device)
            return t.set_(self.saved.untyped_storage(), self.saved.storage_offset() + off.value, tuple(shape))
        return self.saved[off.value: off.value + n].view(*shape)

    def state_grad_shapes(self):
        """{macx_state_grads field: shape} of this run (the layouts of the viewable segments of `saved`)"""
        s = self.shapes
        return {"d_controls": (s.p + 1, s.B, s.d), "d_memories": (s.p + 1, s.B, s.d), "d_att_question": (s.p, s.B, s.S),
                "d_att_kb": (s.p, s.B, s.N), "d_att_self": (s.p, s.B, s.p), "d_att_gate": (s.p, s.B, s.d)}

    def _state_grads(self, state_grads):
        """{field: tensor | None} -> (MacxStateGrads | None, tensors kept alive).  None when no gradient arrived: the plain call."""
        given = {k: v for k, v in (state_grads or {}).items() if v is not None}
        if not given:
            return None, []
        shapes = self.state_grad_shapes()
        sg, held = _lib.MacxStateGrads(), []
        for k, t in given.items():
            if k not in shapes:
                raise KeyError("no state gradient %r (have %s)" % (k, sorted(shapes)))
            if tuple(t.shape) != shapes[k]:
                raise ValueError("%s must be %s, got %s" % (k, shapes[k], tuple(t.shape)))
            t = _f32c(t, k)
            held.append(t)
            setattr(sg, k, t.data_ptr())
        return sg, held

    def backward_begin(self, d_control, d_memory, state_grads=None):
        """Buffers and argument block of this run's backward pass: (args of macx_cell_backward[_phase]_x without the trailing phase /
        stream, {field: gradient view}, (d vecQuestions, d words, d knowledgeBase), the flat gradient buffer, keep-alive list).
        state_grads: None, or {macx_state_grads field: tensor | None} -- gradients a loss sends to the run's histories and attention
        maps themselves (shapes: state_grad_shapes(); finite values).  None / all None passes a NULL struct: the plain call."""
        if not self.keep:
            raise RuntimeError("this run did not keep its activations (train=False / no_grad)")
        dev = self.saved.device
        sg, sg_held = self._state_grads(state_grads)
        ws_floats = self.L.macx_ws_floats(C.byref(self.opts), C.byref(self.shapes), 1)
        ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
        gstruct = _lib.MacxParamGrads()
        present = [f for f in self.params.fields if f in self._ptensors]
        layout = FlatLayout([self._ptensors[f] for f in present])
        # the parameters' persistent flat gradient buffer (one fill instead of one per parameter; the views below become the
        # parameters' .grad, so a flat all-reduce / optimizer needs no gather) -- only for a registered flat consumer and only
        # once per step: a second cell run inside the same backward pass (micro-batches, two towers on one device), or a
        # caller that keeps torch.autograd.grad results across calls, gets a buffer of its own.
        flat = None
        if hasattr(self.params, "claim_grad_buffer") and present == list(self.params.fields):
            if all(getattr(self.params, f).grad is None for f in present):
                buf = self.params.claim_grad_buffer()          # None: no flat consumer, or already handed out this step
                if buf is not None and buf.numel() == layout.total:
                    flat = buf
        if flat is None:
            flat = torch.zeros(layout.total, dtype=torch.float32, device=dev)
        grads = {f: layout.view(flat, i) for i, f in enumerate(present)}
        for f in _lib.PARAM_FIELDS:
            setattr(gstruct, f, grads[f].data_ptr() if f in grads else None)
        gi_vq = torch.empty_like(self.vecQuestions)
        gi_words = torch.empty_like(self.words)
        gi_kb = torch.empty_like(self.knowledgeBase)
        gistruct = _lib.MacxInputGrads(vecQuestions=gi_vq.data_ptr(), words=gi_words.data_ptr(),
                                       knowledgeBase=gi_kb.data_ptr())
        dm = _f32c(d_memory, "d_memory") if d_memory is not None else None
        dc = _f32c(d_control, "d_control") if d_control is not None else None
        args = (C.byref(self.opts), C.byref(self.shapes), C.byref(self.drop), C.byref(self.pstruct), C.byref(self.inputs),
                _lib.ptr(self.saved), C.c_size_t(self.saved_floats), _lib.ptr(ws), C.c_size_t(ws_floats), _lib.ptr(dm), _lib.ptr(dc),
                C.byref(gstruct), C.byref(gistruct), C.byref(sg) if sg is not None else None)
        return args, grads, (gi_vq, gi_words, gi_kb), flat, (ws, gstruct, gistruct, dm, dc, sg, sg_held)

    def backward_phase(self, args, phase):
        """macx_cell_backward_phase_x on torch's CURRENT stream (1: everything but the read unit's deferred contractions, 2: those)"""
        stream = _lib.stream_of(self.saved)
        _lib.check(self.L.macx_cell_backward_phase_x(*args, int(phase), stream), "macx_cell_backward_phase_x(%d)" % phase)

    def backward(self, d_control, d_memory, state_grads=None):
        args, grads, (gi_vq, gi_words, gi_kb), flat, _keep = self.backward_begin(d_control, d_memory, state_grads)
        stream = _lib.stream_of(self.saved)
        hook = self.params.after_backward_phase1
        if hook is not None and self.params.grad_buffer_state(flat):
            # every gradient except the read unit's big contractions is final: let the data-parallel layer start on it
            self.backward_phase(args, 1)
            hook(flat)
            self.backward_phase(args, 2)
        else:
            _lib.check(self.L.macx_cell_backward_x(*args, stream), "macx_cell_backward_x")
        return grads, gi_vq, gi_words, gi_kb


class _CellFunction(torch.autograd.Function):
    """Autograd node for one whole p-step run.  mode 'run' executes the forward here; mode 'adopt'
    wraps a forward that the per-step API already executed."""

    @staticmethod
    def forward(ctx, run, mode, vecQ, words, kb, *params):
        if mode == "run":
            run.forward()
        ctx.run = run
        # an output nobody differentiates (the final control, when only the memory feeds the classifier) arrives as None instead of a
        # freshly filled zeros tensor: one fill and one copy launch less per step -- macx_cell_backward takes NULL for it
        ctx.set_materialize_grads(False)
        p = run.shapes.p
        # all on the run's own `saved` buffer (nothing writes it after the forward pass): no copy launches.  The final state stays
        # an output of its own, so that a plain training step differentiates exactly what it always did; behind it the histories
        # and the attention maps, in the order of _state_segments -- a loss on any of them arrives in backward() as that output's
        # gradient, an unused one as None
        outs = [run.segment(seg, shape, alias=True) for seg, shape in zip(_state_segments(run), _state_shapes(run))]
        final = [run.segment(seg, (p + 1, run.shapes.B, run.shapes.d))[p] for seg in ("controls", "memories")]
        return tuple(final) + tuple(outs)

    @staticmethod
    def backward(ctx, d_control, d_memory, *d_state):
        run = ctx.run
        fields = ["d_" + seg for seg in _state_segments(run)]
        grads, gvq, gwords, gkb = run.backward(d_control, d_memory, dict(zip(fields, d_state)))
        pgrads = tuple(grads[f] for f in run.params.fields)
        # the pass is over: a cell that still publishes this run's differentiable maps goes back to plain views, so that it does not
        # keep the finished autograd graph -- and with it the AccumulateGrad nodes of the parameters -- alive until its next run.
        # (A captured step keeps its cell; nodes that outlive the capture's side stream cost every later eager backward pass a
        # stream synchronisation per parameter.)
        cell = run._cell_ref()
        if cell is not None and cell._run is run:
            cell._drop_graph()
        return (None, None, gvq, gwords, gkb) + pgrads


def _state_segments(run):
    """the viewable segments a run's autograd node returns behind the final state (the macx_state_grads fields without `d_`)"""
    segs = ["controls", "memories", "att_question", "att_kb"]
    if run.opts.write_self_att:
        segs.append("att_self")
    if run.opts.write_gate:
        segs.append("att_gate")
    return segs


STATE_TENSORS = ("controls", "memories", "att_question", "att_kb", "att_self", "att_gate")      # MACCell.state_tensor's names


def _state_shapes(run):
    shapes = run.state_grad_shapes()
    return [shapes["d_" + seg] for seg in _state_segments(run)]


class MACCell:
    """Drop-in for mac_cell.MACCell.  Extra keyword arguments (all optional):
    config   object with the reference's flag names (default: the reference defaults)
    params   MACCellParams (default: freshly initialised like tf.get_variable would)
    seed     dropout stream seed;  b0  global index of this shard's first question (data parallel)
    mask_word  None, or a 1-element int32 tensor on the device: every dropout site XORs it into its key WHEN THE KERNELS RUN
             (macx.h, macx_dropout.mask_word).  The seed is baked into a captured HIP graph, this word is not: write a new
             value between replays and one capture draws fresh masks per step (graph.CapturedTrainStep).  None == word 0.
    Did the run go wrong?  At d = 512 workgroups of one launch hand results to each other with bounded waits; a wait that runs out
    poisons the run (its final memory and gradients are NaN) and is reported by
    status()  -> (bits, first_step): (0, -1) for a clean run (include/macx.h, macx_run_status);  check()  raises macx.HandoffTimeout.
    Both SYNCHRONISE the current stream -- call them where the loop synchronises anyway (after reading the loss), not per launch.
    kb_lengths  None, or an integer tensor [batchSize] on the device: question b's knowledge base is its first kb_lengths[b] cells
             (1 <= kb_lengths[b] <= N; values outside are clamped by the kernel), the rest of its N rows is padding.  The read
             unit attends over the live cells only: attentions["kb"][i][b, kb_lengths[b]:] are exact zeros and the forward pass
             does not depend on what the padded rows hold.  The backward pass multiplies them by that zero: keep them FINITE
             (zeros) when gradients are taken; their own gradient is exactly 0.  The padded rows are still computed.
    gemm     kernel family of the knowledge-base GEMMs of THIS cell: "h2" | "split" | "native" (None: the process default)
    tune     {key: value} for macx_opts.tune, the per-call A/B hooks (_lib.TUNE; measurement only, never needed for results)
    Auxiliary losses.  When the run keeps its activations (train / grad enabled), attentions["kb" | "question" | "self" | "gate"][i],
    controls and memories carry the autograd edge after run() or after the LAST __call__ of the per-step loop, as the reference's
    graph nodes do: attention supervision, entropy regularisers, per-step heads train the network (macx_cell_backward_x).  In the
    per-step loop the autograd node exists only after the last step: a tensor fetched before it is a constant, so read them
    after the loop.  Their incoming gradients must be finite.  infos is a constant.  state_tensor(name) is the stacked tensor behind
    each of them.  Inside a replayed graph: the captured training steps' att_loss= / aux_loss= (graph.py).
    Once the run's backward pass is over the cell publishes plain views again (the finished graph is not kept alive): build the
    whole loss from tensors fetched BEFORE backward(); with retain_graph=True those keep working, tensors fetched afterwards are constants.
    """

    def __new__(cls, *args, config=None, gemm=None, **kw):
        """Option sets without fused kernels (the reference's default configuration among them) are built on the generic
        one-kernel-per-op path (generic.GenericMACCell, same interface); option values the reference itself rejects raise
        what the reference raises."""
        from types import SimpleNamespace
        from .options import UnsupportedOptions
        if cls is MACCell and config is not None and _needs_padding(config):
            # a width the kernels' 128-column granule does not divide (config.py:294-296 takes any): the same cell, zero-padded --
            # as a whole for the option sets with fused kernels, inside each product on the generic path
            try:
                freeze(config)
            except UnsupportedOptions:
                if gemm is not None:
                    raise
                from .generic import GenericMACCell
                return GenericMACCell(*args, config=config, **kw)
            return PaddedMACCell(*args, config=config, gemm=gemm, **kw)
        try:
            freeze(config if config is not None else SimpleNamespace())
        except UnsupportedOptions:
            if gemm is not None:
                raise UnsupportedOptions("gemm=%r selects the kernel family of the FUSED read unit; this option set runs on the "
                                         "generic one-kernel-per-op path, which has no such choice" % (gemm,))
            from .generic import GenericMACCell
            return GenericMACCell(*args, config=config, **kw)
        return super().__new__(cls)

    def __init__(self, vecQuestions, questionWords, questionCntxWords, questionLengths, knowledgeBase,
                 memoryDropout, readDropout, writeDropout, batchSize, train, reuse=None, *, config=None, params=None,
                 netLength=None, seed=None, b0=0, gemm=None, d_logical=0, mask_word=None, tune=None, kb_lengths=None):
        from types import SimpleNamespace
        self.mask_word = _mask_word(mask_word, knowledgeBase)
        self.kb_lengths = _kb_lengths(kb_lengths, knowledgeBase.shape[0])
        self.d_logical = int(d_logical)        # > 0: this is the zero-padded image of a d_logical-wide cell (PaddedMACCell)
        self.config = config if config is not None else SimpleNamespace()
        self.opts = freeze(self.config, gemm, tune)     # raises for rejected / unsupported option sets
        self.netLength = int(netLength if netLength is not None else get(self.config, "netLength"))
        self.vecQuestions = _f32c(vecQuestions, "vecQuestions")
        self.questionWords = questionWords
        self.questionCntxWords = questionCntxWords
        # word source select, mac_cell.py:570
        words = questionCntxWords if get(self.config, "controlContextual") else questionWords
        self._words_src = words
        self.words = _f32c(words, "question words")
        if not questionLengths.is_cuda:
            raise RuntimeError("questionLengths must live on the HIP device: the MAC cell has no CPU path")
        if questionLengths.dtype != torch.int32:
            questionLengths = questionLengths.to(torch.int32)
        if questionLengths.shape != (self.words.shape[0],):
            raise ValueError("questionLengths must be [batchSize]")
        self.questionLengths = questionLengths.contiguous()
        self._kb_src = knowledgeBase
        self._vq_src = vecQuestions
        self.knowledgeBase = _f32c(knowledgeBase, "knowledgeBase")
        train = bool(train)
        self.train = train
        # evaluation feeds keep = 1.0 to every dropout placeholder (model.py:118-125)
        self.dropouts = {"memory": float(memoryDropout) if train else 1.0,
                         "read": float(readDropout) if train else 1.0,
                         "write": float(writeDropout) if train else 1.0}
        self.batchSize = int(batchSize)
        self.reuse = reuse
        self.seed = fresh_seed(seed, bool(train))
        self.b0 = int(b0)
        self.params = params if params is not None else MACCellParams(self.config, self.netLength, device=self.knowledgeBase.device)
        self._none = None           # the dummy cell input / output (mac_cell.py:75): allocated when first asked for (run() never does)
        self.iteration = 0
        self._run = None

    # mac_cell.py:84-93
    @property
    def state_size(self):
        d = get(self.config, "memDim")
        return MACCellTuple(d, d)

    @property
    def output_size(self):
        return 1

    def _needs_grad(self):
        if not torch.is_grad_enabled():
            return False
        srcs = [self._vq_src, self._words_src, self._kb_src] + self.params.tensors()
        return any(t.requires_grad for t in srcs)

    def _views(self, node_outputs=None):
        """the histories and attention maps as views of the run's `saved`; node_outputs: what the run's autograd node returned behind
        the final state -- the same views WITH the autograd edge (a loss on them reaches the inputs and the parameters)"""
        run, s = self._run, self._run.shapes
        if node_outputs is not None:
            out = dict(zip(_state_segments(run), node_outputs))
        else:
            out = {seg: run.segment(seg, shape) for seg, shape in zip(_state_segments(run), _state_shapes(run))}
        self._stacked = out
        self._controls_all = out["controls"]
        self._memories_all = out["memories"]
        self._infos_all = run.segment("infos", (s.p, s.B, s.d))
        # per step: ONE unbind per map (a single autograd node where the map carries the edge) instead of p slices
        self._att_q = out["att_question"].unbind(0)
        self._att_kb = out["att_kb"].unbind(0)
        self._att_self = out["att_self"].unbind(0) if "att_self" in out else None
        self._att_gate = out["att_gate"].unbind(0) if "att_gate" in out else None

    def _republish(self):
        for k in self.attentions:
            del self.attentions[k][:]
        for j in range(self._steps_done):
            self._publish_step(j)

    def _drop_graph(self):
        """back to plain views of `saved` (same lists, entries replaced): called when the run's backward pass is over"""
        self._views()
        self._republish()

    def state_tensor(self, name):
        """The STACKED output of the run's autograd node in the layout of macx_state_grads: "controls" / "memories" [p + 1, B, d],
        "att_question" [p, B, S], "att_kb" [p, B, N], "att_self" [p, B, p] (row i: its first i + 1 entries), "att_gate" [p, B, d].
        The rules of `attentions`: it carries the autograd edge while the run's graph is alive (after run() / the last step of the
        loop) and is a plain view of the run's buffer afterwards.  A loss on it sends ONE gradient tensor to macx_cell_backward_x;
        the same loss over attentions[...][i] goes through unbind's backward pass, which stacks p slices first
        (losses.attention_loss takes this tensor)."""
        if self._run is None:
            raise RuntimeError("no run yet: call zero_state() or run() first")
        if name not in STATE_TENSORS:
            raise KeyError("no state tensor %r (have %s)" % (name, ", ".join(STATE_TENSORS)))
        if name not in self._stacked:
            raise KeyError("this cell has no %s (the option set runs without it)" % name)
        return self._stacked[name]

    # ---- zero_state (mac_cell.py:539-592)
    @property
    def none(self):
        """tf.zeros((batchSize, 1)): the cell's dummy input and output (mac_cell.py:75, :480)"""
        if self._none is None:
            self._none = torch.zeros((self.batchSize, 1), dtype=torch.float32, device=self.knowledgeBase.device)
        return self._none

    def zero_state(self, batchSize=None, dtype=torch.float32):
        self._run = _Run(self, keep_activations=self._needs_grad())
        self._run.begin()
        self._views()
        self._steps_done = 0
        self.attentions = {"kb": [], "question": [], "self": [], "gate": []}
        return MACCellTuple(self._controls_all[0], self._memories_all[0])

    def _publish_step(self, i):
        self.attentions["question"].append(self._att_q[i])
        self.attentions["kb"].append(self._att_kb[i])
        if self._att_self is not None:      # [B, i+1]: initial state + steps 0..i-1 (mac_cell.py:324-329)
            self.attentions["self"].append(self._att_self[i][:, : i + 1])
        if self._att_gate is not None:
            self.attentions["gate"].append(self._att_gate[i])

    # histories as the reference exposes them: [B, steps+1, d] (mac_cell.py:472-474)
    @property
    def controls(self):
        return self._controls_all[: self._steps_done + 1].transpose(0, 1)

    @property
    def memories(self):
        return self._memories_all[: self._steps_done + 1].transpose(0, 1)

    @property
    def infos(self):
        """[B, steps+1, d].  A CONSTANT on the fused path: no gradient flows from a loss on it (there is no d_infos in the C ABI);
        controls, memories and the attention maps carry the autograd edge."""
        # the reference seeds `infos` with the initial MEMORY (mac_cell.py:551)
        return torch.cat([self._memories_all[:1].detach(), self._infos_all[: self._steps_done]], dim=0).transpose(0, 1)

    # ---- one step (mac_cell.py:420-480)
    def __call__(self, inputs, state, scope=None):
        if self._run is None:
            raise RuntimeError("call zero_state() first (model.py:447)")
        i = int(self.iteration)
        if i != self._steps_done:
            raise RuntimeError("steps must run in order: expected iteration %d, got %d" % (self._steps_done, i))
        self._run.step(i)
        self._steps_done = i + 1
        self._publish_step(i)
        control, memory = self._controls_all[i + 1], self._memories_all[i + 1]
        if i == self.netLength - 1 and self._run.keep:
            # the final state carries the autograd edge of the whole run, and from here on so do the histories and the attention
            # maps: the node exists only now, so the entries published by the earlier steps are replaced in place (a tensor FETCHED
            # before the last step stays a constant)
            control, memory, *outs = _CellFunction.apply(self._run, "adopt", self._vq_src, self._words_src, self._kb_src,
                                                         *self.params.tensors())
            self._views(outs)
            self._republish()
        return self.none, MACCellTuple(control, memory)

    # ---- macx_run_status of the latest run
    def status(self):
        """(bits, first_step) of the latest run's hand-off status words; (0, -1): clean.  Synchronises the current stream."""
        if self._run is None:
            raise RuntimeError("no run yet: call zero_state() or run() first")
        return self._run.status()

    def check(self):
        """raises macx.HandoffTimeout if an in-launch hand-off of the latest run gave up.  Synchronises the current stream."""
        if self._run is None:
            raise RuntimeError("no run yet: call zero_state() or run() first")
        self._run.check()

    def reset_status(self):
        """clears the sticky status of the latest run's buffer (after a HandoffTimeout has been handled)"""
        if self._run is not None:
            self._run.reset_status()

    # ---- the whole loop of model.py:453-458 in one ABI call
    def run(self):
        self._run = _Run(self, keep_activations=self._needs_grad())
        self.attentions = {"kb": [], "question": [], "self": [], "gate": []}
        outs = None
        if self._run.keep:
            control, memory, *outs = _CellFunction.apply(self._run, "run", self._vq_src, self._words_src, self._kb_src,
                                                         *self.params.tensors())
        else:
            self._run.forward()
            control = memory = None
        self._views(outs)
        self._steps_done = self.netLength
        for i in range(self.netLength):
            self._publish_step(i)
        if control is None:
            control, memory = self._controls_all[self.netLength], self._memories_all[self.netLength]
        return MACCellTuple(control, memory)


# ---------------------------------------------------------------------------------------------------------------------------
# widths that are not multiples of 128 (config.py:294-296 takes any int): the same cell, zero-padded
# ---------------------------------------------------------------------------------------------------------------------------
def _needs_padding(config):
    d = int(get(config, "memDim"))
    return d % 128 != 0 and d % 8 == 0 and int(get(config, "ctrlDim")) == d and int(get(config, "attDim")) == d


def _pad_last(t, n):
    return torch.nn.functional.pad(t, (0, n - t.shape[-1]))


def _pad_blocks(t, d, dp):
    """[k * d, d] (k row blocks, one per concatenated input: ops.concat, ops.py:65-78) -> [k * dp, dp], each block padded on its own"""
    k = t.shape[0] // d
    return torch.nn.functional.pad(t.reshape(k, d, d), (0, dp - d, 0, dp - d)).reshape(k * dp, dp)


class _PaddedParams:
    """The zero-padded image of a MACCellParams: same fields, every width d -> dp.  The padded tensors are autograd results of
    the logical parameters (torch.nn.functional.pad), so gradients arrive at the logical tensors, sliced, on their own."""
    after_backward_phase1 = None          # owns no flat gradient buffer (no claim_grad_buffer): its backward pass is never split

    def __init__(self, params, d, dp):
        self.fields = list(params.fields)
        self.p = params.p
        for f in self.fields:
            t = getattr(params, f)
            if t.dim() == 1:
                v = t if t.shape[0] == 1 else _pad_last(t, dp)                       # scalar logit biases stay
            elif f in ("memKbProj_W", "newMemory_W", "contControl_W"):
                v = _pad_blocks(t, d, dp)
            elif t.dim() == 2 and t.shape[0] != d:                                   # [nU, d] stacked biases
                v = _pad_last(t, dp)
            elif t.dim() == 2:
                v = torch.nn.functional.pad(t, (0, dp - d, 0, dp - d))
            else:                                                                    # [nU, d, d]
                v = torch.nn.functional.pad(t, (0, dp - d, 0, dp - d))
            setattr(self, f, v)

    def tensors(self):
        return [getattr(self, f) for f in self.fields]


class PaddedMACCell:
    """MACCell for memDim == ctrlDim == attDim == d with d % 128 != 0 (d % 8 == 0): the cell runs dp = ceil(d / 128) * 128 wide
    on zero-padded weights, biases and inputs (macx_shapes.d_logical = d).  Padded columns stay exact zeros through every
    linear layer (zero weights, zero bias), every unit activation config.py offers (NON / RELU in its --relu variants / TANH:
    act(0) = 0; the gate's sigmoid(0) = 0.5 mixes two zeros), attention logit (zero terms of a dot product) and gradient, and
    the kernels take the dropout element index at the LOGICAL width, so states, attentions and gradients are those of the
    unpadded cell with the unpadded cell's masks.  A unit activation of SIGMOID (ops.activations has it, config.py's choices do
    not) would put 0.5 into the padded columns of H1 / the memory -- harmless after slicing, but no longer 'exact zeros' and a
    different H2 row exponent than the unpadded cell's: refused here (UnsupportedOptions) rather than run untested.  Same
    interface as MACCell; states and histories come back d wide."""

    def __init__(self, vecQuestions, questionWords, questionCntxWords, questionLengths, knowledgeBase,
                 memoryDropout, readDropout, writeDropout, batchSize, train, reuse=None, *, config=None, params=None,
                 netLength=None, seed=None, b0=0, gemm=None, mask_word=None, tune=None, kb_lengths=None):
        import copy
        from .options import UnsupportedOptions
        # the dropout index at the logical width (macx_shapes.d_logical) is implemented by the H2 kernel family: the padded cell runs
        # on it whatever the process default is; asking for another family is refused, not silently overridden
        if gemm not in (None, "h2"):
            raise UnsupportedOptions("gemm=%r: a cell whose width is not a multiple of 128 runs zero-padded on the H2 kernel family only" % (gemm,))
        gemm = "h2"
        for o in ("controlInputAct", "controlContAct", "readMemAct", "readCtrlAct", "writeMemAct"):
            if str(get(config, o)).upper() == "SIGMOID":
                raise UnsupportedOptions("%s=SIGMOID on a zero-padded width: sigmoid(0) = 0.5 would fill the padded columns" % o)
        self.config = config
        d = self.d = int(get(config, "memDim"))
        dp = self.dp = (d + 127) // 128 * 128
        self.netLength = int(netLength if netLength is not None else get(config, "netLength"))
        self.params = params if params is not None else MACCellParams(config, self.netLength, device=knowledgeBase.device)
        wide = copy.copy(config)
        wide.memDim = wide.ctrlDim = wide.attDim = dp
        pad = lambda t: _pad_last(t, dp)
        words_p = pad(questionWords)
        cntx_p = words_p if questionCntxWords is questionWords else pad(questionCntxWords)
        self.inner = MACCell(pad(vecQuestions), words_p, cntx_p, questionLengths, pad(knowledgeBase), memoryDropout, readDropout,
                             writeDropout, batchSize, train, reuse, config=wide, params=_PaddedParams(self.params, d, dp),
                             netLength=self.netLength, seed=seed, b0=b0, gemm=gemm, d_logical=d, mask_word=mask_word, tune=tune,
                             kb_lengths=kb_lengths)
        self.batchSize, self.train, self.seed, self.b0 = self.inner.batchSize, self.inner.train, self.inner.seed, self.inner.b0

    none = property(lambda self: self.inner.none)
    iteration = property(lambda self: self.inner.iteration, lambda self, v: setattr(self.inner, "iteration", v))
    @property
    def attentions(self):
        """the inner cell's maps.  Without a gate: the inner cell's own dict.  With one, the gate -- the one map as wide as the state --
        is cropped to the logical width by ordinary slicing (the autograd edge of the inner tensors is kept): then this is a NEW
        dict with a new gate list on every access, so fetch it once, and do not expect a change made to it to last."""
        a = self.inner.attentions
        if not a["gate"]:
            return a
        return {k: ([t[..., :self.d] for t in v] if k == "gate" else v) for k, v in a.items()}

    @property
    def state_size(self):
        return MACCellTuple(self.d, self.d)

    @property
    def output_size(self):
        return 1

    def _cut(self, state):
        return MACCellTuple(state.control[..., :self.d], state.memory[..., :self.d])

    def zero_state(self, batchSize=None, dtype=torch.float32):
        return self._cut(self.inner.zero_state(batchSize, dtype))

    def __call__(self, inputs, state, scope=None):
        out, st = self.inner(inputs, state, scope)
        return out, self._cut(st)

    def run(self):
        return self._cut(self.inner.run())

    def status(self):
        return self.inner.status()

    def check(self):
        return self.inner.check()

    def reset_status(self):
        return self.inner.reset_status()

    def state_tensor(self, name):
        """MACCell.state_tensor; what is as wide as the state (controls, memories, att_gate) cropped to the logical width by
        ordinary slicing, as the lists are"""
        t = self.inner.state_tensor(name)
        return t[..., :self.d] if name in ("controls", "memories", "att_gate") else t

    controls = property(lambda self: self.inner.controls[..., :self.d])
    memories = property(lambda self: self.inner.memories[..., :self.d])
    infos = property(lambda self: self.inner.infos[..., :self.d])
