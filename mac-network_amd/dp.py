"""Batch data parallelism for the MAC cell: one process per GPU, `torch.distributed` over RCCL/xGMI.

The reference builds one tower per GPU and slices the batch with `initTowerBatch`
(model.py:139-149) but never exchanges gradients -- `averageAcrossTowers` keeps tower 0
(model.py:671-679, "TODO (add back support for multi-gpu..)").  Here every question is independent
in the forward pass, so the only exchange is ONE all-reduce per step of a flat fp32
gradient buffer (cell only: 2.1 M + p * 0.26 M parameters = 21 MB at p = 12).  Each rank computes
the MEAN loss over its shard (model.py:596); shard gradients are combined weighted by shard size so
that the result equals the full-batch gradient.
"""

import contextlib

import torch
import torch.distributed as dist

from .params import FlatLayout


def tower_slice(batch_size, rank, world):
    """model.py:139-149: floor(B/R) questions per tower, the last tower takes the remainder."""
    per = batch_size // world
    start = rank * per
    end = (rank + 1) * per if rank < world - 1 else batch_size
    return start, end


def _world(group):
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


class GradBucket:
    """Flat gradient buffer reused across steps; one all-reduce (sum) per step.

    `flat`: a persistent buffer the backward pass already writes into (MACCellParams.grad_buffer(): macx_cell_backward
    receives pointers into it, and autograd hands the views through as `.grad`).  When every gradient is found to be a
    view of that buffer at its expected offset the all-reduce runs on it in place -- no gather copy; anything else (a
    gradient produced elsewhere, accumulated, or absent) falls back to one gather kernel into the buffer."""

    tensors = property(lambda self: self._tensors)          # (TowerBuckets: a method -- what its optimizer is built over)

    def __init__(self, tensors, flat=None, params=None):
        """params: the MACCellParams whose grad_buffer() `flat` is -- registers this bucket as its flat consumer (the backward
        pass then writes into the buffer, once per step) and releases the buffer again after every all-reduce."""
        self.owner = params
        if params is not None:
            if flat is None:
                flat = params.grad_buffer()
            params.register_grad_buffer_user()
        self._tensors = list(tensors)
        self.layout = FlatLayout(self._tensors)
        self.sizes, self.offsets = self.layout.sizes, self.layout.offsets
        if flat is None:
            flat = torch.zeros(self.layout.total, dtype=torch.float32, device=self._tensors[0].device)
        if flat.numel() < self.layout.total:
            raise ValueError("flat buffer holds %d floats, the gradients need %d" % (flat.numel(), self.layout.total))
        self.flat = flat
        self.zero_copy_steps = 0

    def begin_step(self, shard_size, global_size):
        """One bucket: nothing to prepare.  (The two-bucket classes take the shard weight here: their phase-1 hook needs it.)"""

    def _in_place(self, lo, hi):
        return all(self.layout.is_view(self.flat, i, self._tensors[i].grad) for i in range(lo, hi))

    def _gather(self, lo, hi):
        for i in range(lo, hi):
            g, dst = self._tensors[i].grad, self.layout.view(self.flat, i)
            if g is None:
                dst.zero_()
            elif not self.layout.is_view(self.flat, i, g):
                dst.copy_(g)

    def allreduce_(self, shard_size, global_size, group=None):
        """grads <- sum_r (shard_r / global) * grads_r  == gradient of the full-batch mean loss."""
        if self._in_place(0, len(self._tensors)):
            self.zero_copy_steps += 1
        else:
            self._gather(0, len(self._tensors))
        return self._reduce_all(float(shard_size) / float(global_size), group)

    def _reduce_all(self, w, group):
        if w != 1.0:
            self.flat.mul_(w)
        if _world(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
        return self._publish()

    def _publish(self):
        """The step's gradients are final: every .grad is a view of the reduced buffer, and the next backward pass may take the
        persistent buffer again (the caller drops the .grad views -- zero_grad / an optimizer step -- before it runs, as with any
        accumulate-free training loop)."""
        for i, t in enumerate(self._tensors):
            t.grad = self.layout.view(self.flat, i)
        if self.owner is not None:
            self.owner.release_grad_buffer()
        return self.flat


class _TwoBuckets(GradBucket):
    """What OverlappedBuckets and TowerBuckets share: flat[:early] is final when the cell's backward pass calls
    `after_backward_phase1`, and is scaled and all-reduced from there -- on a side stream on the GPU -- while the rest of the
    backward pass still runs; allreduce_() after backward() exchanges flat[early:] and joins.  A subclass says which range is
    early, when its hook may start it (_phase1 -> _start_early), and what it falls back to (allreduce_ -> _finish only when
    _early_done)."""

    def _two_buckets(self, cell, early, group):
        self.owner, self.early, self.group = cell, early, group
        self.weight = 1.0
        self._early_work, self._early_started = None, False
        self.side = torch.cuda.Stream(device=self.flat.device) if self.flat.is_cuda else None
        self.overlapped_steps = 0
        cell.after_backward_phase1 = self._phase1

    def _active(self):
        return _world(self.group) > 1

    def begin_step(self, shard_size, global_size):
        self.weight = float(shard_size) / float(global_size)
        self._early_started, self._early_work = False, None

    def _start_early(self):
        part = self.flat[:self.early]
        if self.side is not None:
            self.side.wait_stream(torch.cuda.current_stream(self.flat.device))
        with torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext():
            if self.weight != 1.0:
                part.mul_(self.weight)
            self._early_work = dist.all_reduce(part, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._early_started = True

    def _early_done(self, w, lo, hi, whose):
        done = self._early_started and w == self.weight and self._in_place(lo, hi)
        if self._early_started and not done:
            raise RuntimeError("the early bucket is already in flight but %s gradients are not views of the flat buffer" % whose)
        return done

    def _finish(self, w):
        late = self.flat[self.early:]
        if w != 1.0:
            late.mul_(w)
        if late.numel():
            dist.all_reduce(late, op=dist.ReduceOp.SUM, group=self.group)
        if self._early_work is not None:
            self._early_work.wait()
        if self.side is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self.side)
        self._early_started = False
        self.overlapped_steps += 1
        return self._publish()


class OverlappedBuckets(_TwoBuckets):
    """Two buckets over MACCellParams.grad_buffer(), the first in flight while the backward pass is still running.

    The cell's backward pass produces its gradients in two parts (macx_cell_backward_phase): everything except the read
    unit's [B,N,d]-contraction weights is final after phase 1 -- 80 % of the bytes at p = 12 -- and sits in ONE contiguous
    range at the front of the flat buffer (MACCellParams.fields puts the late tensors last).  The cell calls
    `after_backward_phase1` between the phases; this class answers by starting the all-reduce of that range on a side stream
    (RCCL over xGMI), so it overlaps phase 2, the last ~10 % of the backward pass.  `allreduce_()` after backward() reduces the
    rest and joins the side stream.  Falls back to the single all-reduce of GradBucket whenever the gradients are not the
    zero-copy views of the flat buffer.

        bucket = OverlappedBuckets(params)
        bucket.begin_step(shard_size, global_size)     # before backward(): the hook needs the shard weight
        loss.backward()
        bucket.allreduce_(shard_size, global_size)
    """

    def __init__(self, params, group=None):
        super().__init__(params.tensors(), flat=params.grad_buffer(), params=params)
        self._two_buckets(params, params.early_floats(), group)

    def _phase1(self, flat):
        if self._active() and flat.data_ptr() == self.flat.data_ptr() and self.early != 0:
            self._start_early()

    def allreduce_(self, shard_size, global_size, group=None):
        w = float(shard_size) / float(global_size)
        if not self._early_done(w, 0, len(self._tensors), "the"):
            return super().allreduce_(shard_size, global_size, group if group is not None else self.group)
        self.zero_copy_steps += 1
        return self._finish(w)


class TwoPhaseStep:
    """The host side of a data-parallel step whose backward pass is cut at the phase-1 seam (macx_cell_backward_phase): run part A
    (forward + backward phase 1), hand the finished front of the flat gradient buffer to the bucket -- the early all-reduce starts on the
    side stream -- run part B (backward phase 2) under it, then the late bucket and the join.  What the parts ARE is the subclass's
    business: graph.CapturedDPTrainStep replays two captured HIP graphs (2 replays + 2 collectives per step instead of ~125 launches);
    tests/test_dp_gloo.py drives this class with stand-in parts on CPU.  The bucket is driven exactly as the cell's autograd node
    drives it in the eager step (begin_step -> phase-1 hook -> allreduce_), so both give the same bits."""

    def __init__(self, params, bucket, shard, global_batch):
        self.params, self.bucket = params, bucket
        self.shard, self.global_batch = int(shard), int(global_batch)

    def run_part_a(self):          # forward + backward phase 1; returns {field: gradient view of the flat buffer}
        raise NotImplementedError

    def run_part_b(self):          # backward phase 2
        raise NotImplementedError

    def exchange_step(self):
        b = self.bucket
        b.begin_step(self.shard, self.global_batch)
        grads = self.run_part_a()
        for f, g in grads.items():                       # (views of the flat buffer at the bucket's offsets: its zero-copy path)
            getattr(self.params, f).grad = g
        hook = self.params.after_backward_phase1
        if hook is not None:
            hook(b.flat)                                 # early bucket: scale + all-reduce (side stream on the GPU)
        self.run_part_b()
        return b.allreduce_(self.shard, self.global_batch)      # late bucket (or the one bucket), join; releases the flat buffer


def shard_count(n, lo, hi):
    """Of the n live questions of a short global batch -- global slots 0 .. n-1 are live, the slots are dealt by tower_slice -- the
    rank that holds slots [lo, hi) has clamp(n - lo, 0, hi - lo), at the front of its shard."""
    return max(0, min(int(n) - int(lo), int(hi) - int(lo)))


def live_weight_sum(weights, out):
    """out[0] <- the sum in fp64 of the live weights of a [B] float32 tensor: live means w > 0, everything else counts 0, as
    macx_answer_loss_weighted defines it.  `out` is a 1-element float64 tensor; kernels only (capturable), no host read."""
    live = torch.where(weights > 0, weights, torch.zeros_like(weights))
    return torch.sum(live.to(torch.float64), dim=0, keepdim=True, out=out)


def shard_factor(w_local, w_global):
    """W_r / W_g as a 1-element float64 tensor, exactly 0 where W_g == 0 (no division by zero: the quotient is taken over 1 there) and
    exactly 1 where the two are equal: what a rank's locally normalised weighted mean is multiplied by so that the ranks' terms SUM to
    the weighted mean over the global batch.  Torch ops on 1-element tensors, read when they run."""
    some = w_global > 0
    return torch.where(some, w_local / torch.where(some, w_global, torch.ones_like(w_global)), torch.zeros_like(w_global))


def reduce_totals(totals, group=None):
    """The dict output.AnswerTotals.read() returns, for the whole job: ONE sum all-reduce of the three doubles of every rank's `totals`
    (loss, accuracy and weight are then those of all the questions the ranks scored).  A collective: every rank of the group calls it,
    once per epoch; it synchronises.  The rank's own totals are left as they are.  One process: totals.read()."""
    t = totals.tensor.clone()
    if _world(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    loss, hit, w = t.tolist()
    return dict(loss=loss / w if w > 0 else 0.0, accuracy=hit / w if w > 0 else 0.0, weight=w)


class TowerExchangeStep:
    """The host side of a data-parallel step of the WHOLE tower that is cut at its collectives, not inside its backward pass:

        [ part Q: W_r, the sum of the shard's live weights ]   [ sum all-reduce of that one double: W_g ]      weighted steps only
          part A: forward, loss, backward, gather into the flat buffer      sum all-reduce of the flat buffer
          part B: the optimizer step on the reduced buffer

    What the parts ARE is the subclass's business, as with TwoPhaseStep: the sequence is made for parts that are captured HIP graphs
    (two or three replays and one or two collectives per step in the place of every launch of the eager step; torch.distributed calls
    cannot sit inside a graph, and the tower's backward pass is an autograd pass that cannot be cut in two as the cell's library
    calls can).  graph.CapturedDPTowerTrainStep is that subclass (existing kernels replayed, none added);
    tests/test_dp_tower_exchange_gloo.py drives this class with stand-in parts on CPU.
    Every rank issues the same collectives in the same order whatever its parts do -- a rank whose shard is all dead, or whose
    parts fell back to eager launches, stays in lock step.  One process: no collective at all.

    Weighted steps (w_local / w_global given: 1-element float64 tensors): part Q writes W_r into BOTH, the all-reduce turns w_global
    into W_g, and part A trains on  ce_r * factor()  with ce_r the rank's own weighted mean -- so the plain SUM of the ranks' gradients
    is the gradient of the weighted mean over the global batch, the buffer is not rescaled, and a rank without a live question
    contributes zeros.  Unweighted steps scale by shard / global inside part A, as GradBucket._reduce_all does in front of its all-reduce."""

    def __init__(self, flat_grad, group=None, w_local=None, w_global=None):
        self.flat_grad, self.group = flat_grad, group
        self.w_local, self.w_global = w_local, w_global

    def run_part_q(self):          # w_local, w_global <- the shard's live weight (live_weight_sum)
        raise NotImplementedError

    def run_part_a(self):          # forward .. the gathered (unweighted: scaled) flat gradient buffer
        raise NotImplementedError

    def run_part_b(self):          # the optimizer step on the reduced buffer
        raise NotImplementedError

    def factor(self):
        """shard_factor of the step's two sums (1-element float64)"""
        return shard_factor(self.w_local, self.w_global)

    def exchange_step(self):
        world = _world(self.group)
        if self.w_global is not None:
            self.run_part_q()
            if world > 1:
                dist.all_reduce(self.w_global, op=dist.ReduceOp.SUM, group=self.group)
        self.run_part_a()
        if world > 1:
            dist.all_reduce(self.flat_grad, op=dist.ReduceOp.SUM, group=self.group)
        self.run_part_b()
        return self.flat_grad


class TowerBuckets(_TwoBuckets):
    """Data parallelism for the WHOLE tower the reference builds per GPU (model.py:775-826: embeddings, question encoder, stem,
    MAC cell, output unit + classifier -- 57 MB of fp32 gradients at p = 12), two buckets over ONE flat buffer:

        [ output unit + classifier | cell, early fields | cell, late fields | stem | question encoder ]
          `--------- early bucket ---------'             `------------ late bucket -------------'

    Backward order decides the split: the classifier's gradients exist before the cell's backward pass starts and the cell's
    early fields are final after its phase 1 (macx_cell_backward_phase), so that range is all-reduced on a side stream from the
    cell's phase-1 hook while phase 2 -- and then the stem's and the encoder's backward passes, which need the cell's input
    gradients -- still run; the rest follows after backward().  The cell's gradient buffer IS its range of the flat buffer
    (MACCellParams.adopt_grad_buffer), the other modules' gradients are gathered into theirs.  Clipping comes
    after the exchange, as in model.py:645-650: hand `flat` to optim.FlatAdamEMA(bucket.tensors()).step(flat_grad=bucket.flat).
    So does a guarded optimizer's decision (FlatAdamEMA(guard=True)): it is taken on `flat` AFTER the all-reduce, every rank holds
    the same reduced buffer -- a NaN on one rank is a NaN on all -- so every rank skips or applies alike, with no code of its own.

        bucket = TowerBuckets(net); opt = FlatAdamEMA(bucket.tensors(), ...)
        bucket.begin_step(shard, global_batch); loss.backward(); bucket.allreduce_(shard, global_batch); opt.step(bucket.flat)

    fused_gather=True gathers with ONE launch of macx_gather_flat per gather instead of one copy_ per tensor (17 outside the cell):
    a table of (gradient pointer, offset, count) in device memory, uploaded when the gradients' addresses change -- in a steady
    training loop the allocator hands the same blocks back, so once.  It is also what makes the gather capturable: a per-tensor
    copy_ becomes a memcpy node, which HIP graph replay does not keep in stream order with kernel nodes (graph.py).  Under a
    capture the gradients live in the graph's pool and nothing can be uploaded, so the capture only points the kernel at a
    SPARE table and flush_tables() fills it once the capture has ended.  The spares are allocated here, in ordinary memory,
    zeroed (an unflushed table gathers nothing): a buffer allocated under the capture would sit in a block of the graph's
    pool that an earlier temporary of the same graph has given back, and that temporary's kernels write it again on every
    replay -- behind the upload, in front of the gather.  Two spares per captured step (reserve_tables() adds more).

    exchange=False: the bucket gathers and the STEP exchanges (TowerExchangeStep; graph.CapturedDPTowerTrainStep captures the
    gather inside its part A, where a collective must never be issued).  The phase-1 hook then starts nothing, whatever the world
    size, and gather_(shard, global_batch) is allreduce_ without its collectives: gather, flat *= shard / global, publish.  One
    gather, so one spare table per captured step.  exchange=True, the default, is the class as it always was.
    """

    def __init__(self, net, group=None, fused_gather=False, exchange=True):
        self.net = net
        self.fused_gather = bool(fused_gather)
        self.exchange = bool(exchange)
        self._tables = {}                    # (lo, hi) -> [host rows, device table]: the eager gathers
        self._captured_tables = []           # [host rows, device table, uploaded]: one per gather issued under a capture
        self._spare_tables = []              # device tables for gathers issued under a capture (see the class docstring)
        cell = net.cell
        if not hasattr(cell, "early_floats"):
            raise TypeError("TowerBuckets needs the fused cell's parameters (MACCellParams); a generic-path cell is exchanged with "
                            "GradBucket(net.tensors())")
        enc = list(net.enc.tensors()) if hasattr(net, "enc") else []
        groups = [list(net.out.tensors()), list(cell.tensors()), list(net.stem.tensors()), enc]
        super().__init__([t for g in groups for t in g])
        self.n_out, self.n_cell = len(groups[0]), len(groups[1])
        self.cell_lo, self.cell_hi = self.layout.prefix(self.n_out), self.layout.prefix(self.n_out + self.n_cell)
        cell.adopt_grad_buffer(self.flat[self.cell_lo:self.cell_hi])      # the cell's backward pass writes straight into its range
        self._two_buckets(cell, self.cell_lo + cell.early_floats(), group)
        self.allreduce_ms = None
        if self.fused_gather:
            self.reserve_tables(4)

    def tensors(self):
        """the parameters in the flat buffer's order (what optim.FlatAdamEMA must be built over to take `flat` as it is)"""
        return list(self._tensors)

    def _gather_fused(self, lo, hi):
        from . import _lib
        base = self.flat.data_ptr()
        rows = []
        for t, o, n in zip(self._tensors[lo:hi], self.offsets[lo:hi], self.sizes[lo:hi]):
            g = t.grad
            if g is None:
                rows.append((0, o, n))                               # no gradient: the slice is zero-filled
                continue
            if g.dtype != torch.float32 or g.device != self.flat.device or g.numel() != n:
                raise TypeError("fused gather: a gradient that is not a float32 tensor of its parameter's size on the buffer's device")
            if not g.is_contiguous():
                g = g.contiguous()
            if g.data_ptr() != base + 4 * o:
                rows.append((g.data_ptr(), o, n))
        if not rows:
            return
        flatrows = [x for r in rows for x in r]
        if torch.cuda.is_current_stream_capturing():
            if not self._spare_tables:
                raise RuntimeError("fused gather under a capture: no spare table left (call bucket.reserve_tables(k) before capturing)")
            table = self._spare_tables.pop()
            self._captured_tables.append([flatrows, table, False])
        else:
            slot = self._tables.get((lo, hi))
            if slot is None or slot[0] != flatrows:
                table = torch.tensor(flatrows, dtype=torch.int64).to(self.flat.device)
                self._tables[(lo, hi)] = [flatrows, table]
            table = self._tables[(lo, hi)][1]
        _lib.check(_lib.lib().macx_gather_flat(_lib.ptr(table), len(rows), base, _lib.stream_of(self.flat)), "macx_gather_flat")

    def reserve_tables(self, k):
        """k more spare device tables for gathers issued under a capture; call it outside any capture"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("reserve_tables() inside a capture: the tables must not live in the graph's pool")
        for _ in range(int(k)):
            self._spare_tables.append(torch.zeros(3 * len(self._tensors), dtype=torch.int64, device=self.flat.device))

    def flush_tables(self):
        """upload the tables of the gathers issued under a capture (call once the capture has ended, before the first replay)"""
        for slot in self._captured_tables:
            if not slot[2]:
                slot[1][:len(slot[0])].copy_(torch.tensor(slot[0], dtype=torch.int64))
                slot[2] = True

    def _gather(self, lo, hi):
        return self._gather_fused(lo, hi) if self.fused_gather else super()._gather(lo, hi)

    def _phase1(self, flat):
        if not self.exchange:
            return                                    # the step owns the collectives (gather_): none is ever started from here
        if flat.data_ptr() != self.flat.data_ptr() + 4 * self.cell_lo:
            return                                    # this backward pass got a buffer of its own: everything goes late
        if any(t.grad is None for t in self._tensors[:self.n_out]):
            return                                    # the classifier's gradients are not there yet (unusual graph): all late
        if not self._active():
            return                                    # single process: allreduce_ gathers and scales the WHOLE buffer (like OverlappedBuckets)
        self._gather(0, self.n_out)
        self._start_early()

    def allreduce_(self, shard_size, global_size):
        w = float(shard_size) / float(global_size)
        n = self.n_out + self.n_cell
        early_done = self._early_done(w, self.n_out, n, "the cell's")
        if not early_done:
            self._gather(0, n)
        self._gather(n, len(self._tensors))
        return self._finish(w) if early_done else self._reduce_all(w, self.group)

    def gather_(self, shard_size, global_size):
        """exchange=False: what allreduce_ does around its collectives and nothing else -- every gradient into `flat` (fused: one
        macx_gather_flat launch), flat *= shard / global where that is not 1.0 (the same mul_, in the same place in front of the
        reduce, as _reduce_all and _start_early), the .grad views published and the cell's buffer released.  The caller reduces `flat`."""
        if self.exchange:
            raise RuntimeError("gather_() belongs to a bucket built with exchange=False; this one exchanges from its phase-1 hook and "
                               "in allreduce_()")
        w = float(shard_size) / float(global_size)
        self._gather(0, len(self._tensors))
        if w != 1.0:
            self.flat.mul_(w)
        return self._publish()
