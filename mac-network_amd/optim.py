"""Training step of the reference (model.py:615-669): tf.clip_by_global_norm(8) -> tf.train.AdamOptimizer
-> tf.train.ExponentialMovingAverage(0.999), as ONE multi-tensor HIP pass over a flat fp32 buffer.

The parameters are re-pointed at slices of one flat tensor; gradients are gathered into (or, after
macx.dp.GradBucket.allreduce_, already live in) one flat tensor; Adam moments and the EMA shadow are flat
buffers too.  SURVEY.md 8f row 3."""
import collections
import ctypes as C
import math

import torch

from . import _lib
from .params import FlatLayout, grad_buffer_owner


GuardCounts = collections.namedtuple("GuardCounts", "applied skipped first last")


class FlatAdamEMA:
    def __init__(self, params, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, clip_norm=8.0, ema_decay=0.999, grad_owner=None,
                 guard=False, skip_above=None):
        """guard: True -- the guarded step (macx_adam_ema_step_g / _pg): the update kernel itself skips a step whose gradient norm
        is not finite (a NaN or an infinity anywhere in the flat gradient, or a sum of squares that overflows fp32) or, with
        skip_above=x > 0, greater than x; a skipped step writes no byte of flat, m, v, ema, and is counted in self.guard, four
        int32 words on the device (guard_counts()).  The decision is the device's: the host learns of it only by reading the
        words, so self.t and the rate advance() writes count ATTEMPTS, skipped ones included, while `applied` is the number of
        updates the moments have seen.  (Deliberately: an applied guarded step stays bit-identical to the unguarded one, and the
        rate stays a host computation.)  False -- the launches and bits of before.  skip_above without guard=True is a ValueError.
        grad_owner: the MACCellParams whose grad_buffer() will be handed to step(flat_grad=...) by a cell-only training loop
        with no data-parallel bucket in between -- this optimizer then is the buffer's flat consumer: it registers (the backward
        pass writes into the persistent buffer only for a registered consumer) and releases the buffer at the end of every
        step.  With a dp.GradBucket / OverlappedBuckets / TowerBuckets the bucket is the consumer: leave this None."""
        if skip_above is not None and not guard:
            raise ValueError("skip_above= is the guarded step's threshold: it needs guard=True")
        if skip_above is not None and not float(skip_above) >= 0.0:
            raise ValueError("skip_above must be >= 0 (0 or None: no threshold), got %r" % (skip_above,))
        self.skip_above = float(skip_above) if skip_above is not None else 0.0
        self.grad_owner = grad_owner
        if grad_owner is not None:
            grad_owner.register_grad_buffer_user()
        self.params = [p for p in params]
        if not self.params or not self.params[0].is_cuda:
            raise RuntimeError("FlatAdamEMA needs parameters on the HIP device")
        # the layout of MACCellParams.grad_buffer() and dp.GradBucket.flat, so that either can be handed to step(flat_grad=...) as
        # it is (pad floats stay zero: gradient, moments and update)
        self.layout = FlatLayout(self.params)
        self.sizes, self.offsets, n = self.layout.sizes, self.layout.offsets, self.layout.total
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        for i, p in enumerate(self.params):                                   # parameters become views of the flat buffer
            self.layout.view(self.flat, i).copy_(p.data)
            p.data = self.layout.view(self.flat, i)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ema = self.flat.clone() if ema_decay is not None and ema_decay >= 0 else None   # shadow starts at the initial value
        self.ws = torch.empty(1024, dtype=torch.float32, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps
        self.clip_norm = clip_norm if clip_norm else 0.0
        self.ema_decay = ema_decay if self.ema is not None else -1.0
        self.t = 0
        # the bias-corrected rate of step t in DEVICE memory (macx_adam_ema_step_p reads it when the kernel runs): written by advance()
        self.lr_t = torch.zeros(1, dtype=torch.float32, device=dev)
        # the guarded step's words (include/macx.h): applied, skipped, first and last skipped attempt; None: the unguarded step
        self.guard = torch.zeros(4, dtype=torch.int32, device=dev) if guard else None

    @staticmethod
    def bias_corrected_lr(lr, beta1, beta2, t):
        """(float) (lr * sqrt(1 - beta2^t) / (1 - beta1^t)) as macx_adam_ema_step computes it: lr, beta1, beta2 arrive there as C
        floats, the expression is evaluated in double and rounded to float once."""
        f = lambda x: C.c_float(x).value
        return f(f(lr) * math.sqrt(1.0 - math.pow(f(beta2), t)) / (1.0 - math.pow(f(beta1), t)))

    def advance(self):
        """The host half of a step(device_lr=True): t += 1, and the rate of step t from the CURRENT self.lr into the device scalar.
        Call it outside a captured graph, before each replay: the captured update kernel then follows the step count and any
        change of self.lr (--lrReduce)."""
        self.t += 1
        self.lr_t.fill_(self.bias_corrected_lr(self.lr, self.beta1, self.beta2, self.t))
        return self.t

    def step(self, flat_grad=None, device_lr=False):
        """device_lr: False -- the step of before: t += 1 here, lr and t travel by value (macx_adam_ema_step).  True -- this call only
        ENQUEUES the update (macx_adam_ema_step_p): the kernel reads the rate advance() wrote, t is not touched; the pair
        advance(); step(device_lr=True) gives the bits of step().  What a captured graph holds (graph.CapturedTowerTrainStep).
        Built with guard=True both go through the guarded exports (_g / _pg): see __init__ and guard_counts().
        flat_grad: an already flat gradient in THIS layout (params.FlatLayout over the parameters in order): dp.GradBucket.flat /
        TowerBuckets.flat after the all-reduce, or MACCellParams.grad_buffer() for a cell-only optimizer built with grad_owner=
        (without a registered consumer the backward pass does not write into that buffer: a stale or zero gradient would be
        stepped on -- refused below; a dp bucket over the parameters is such a consumer).  A buffer of any other size is
        rejected.  Without flat_grad the .grad of every parameter is gathered."""
        if flat_grad is not None and self.grad_owner is None:
            # a cell's own buffer is only ever written for a REGISTERED consumer: a dp bucket built over it (GradBucket(params=...),
            # OverlappedBuckets) is one, and hands its `flat` -- this very tensor -- over after the exchange
            owner = grad_buffer_owner(flat_grad)
            if owner is not None and not owner.grad_buffer_state(flat_grad):
                raise ValueError("this is a MACCellParams.grad_buffer() nobody is registered for: build the optimizer with "
                                 "grad_owner=params (or a dp bucket over the parameters) so that the backward pass writes into it")
        if flat_grad is None:
            for i, p in enumerate(self.params):
                if p.grad is None:
                    self.layout.view(self.grad, i).zero_()
                else:
                    self.layout.view(self.grad, i).copy_(p.grad)
            flat_grad = self.grad
        elif flat_grad.numel() != self.flat.numel() or flat_grad.dtype != torch.float32:
            raise ValueError("flat_grad holds %d floats, this optimizer's layout %d (segments padded to 4 floats, parameters in "
                             "the order given at construction)" % (flat_grad.numel(), self.flat.numel()))
        L = _lib.lib()
        ptr = _lib.ptr
        head = (self.flat.numel(), ptr(self.flat), ptr(flat_grad), ptr(self.m), ptr(self.v), ptr(self.ema))
        guarded = self.guard is not None
        tail = (self.clip_norm, self.ema_decay) + ((self.skip_above, ptr(self.guard)) if guarded else ())
        tail += (ptr(self.ws), ptr(self.norm), _lib.stream_of(self.flat))
        # (two calls, not one with a suffix: for the plain one the LIBRARY computes the bias-corrected rate from lr and the step count)
        if device_lr:
            name = "macx_adam_ema_step_pg" if guarded else "macx_adam_ema_step_p"
            _lib.check(getattr(L, name)(*head, ptr(self.lr_t), self.beta1, self.beta2, self.eps, *tail), name)
        else:
            self.t += 1
            name = "macx_adam_ema_step_g" if guarded else "macx_adam_ema_step"
            _lib.check(getattr(L, name)(*head, self.lr, self.beta1, self.beta2, self.eps, self.t, *tail), name)
        if self.grad_owner is not None:
            self.grad_owner.release_grad_buffer()          # the step's gradients are consumed: the next backward may claim the buffer
        return self.norm

    def guard_counts(self):
        """GuardCounts(applied, skipped, first, last) of a guarded optimizer: steps applied (= the updates m and v have seen), steps
        skipped, and the 1-based attempt index of the first and the last skipped step (0: none); applied + skipped is the number
        of attempts since construction or reset_guard().  One device-to-host copy, i.e. one synchronisation: read it once per
        epoch, next to QuestionStore.check()."""
        if self.guard is None:
            raise ValueError("this optimizer was built without guard=True: it counts nothing")
        return GuardCounts(*(int(x) & 0xFFFFFFFF for x in self.guard.tolist()))        # (uint32 words in an int32 tensor)

    def reset_guard(self):
        """zero the guard words (stream-ordered, no synchronisation)"""
        if self.guard is None:
            raise ValueError("this optimizer was built without guard=True")
        self.guard.zero_()

    def ema_state(self):
        """{index: tensor} views of the EMA shadow, shaped like the parameters (what emaSaver restores, main.py:711-729)."""
        return [self.layout.view(self.ema, i) for i in range(len(self.params))]
