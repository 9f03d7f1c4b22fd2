"""Gradient accumulation (train.py --accum_steps N; rd_grad_accum, csrc/accum.hip): the fused step runs forward, losses and backward
on every iteration exactly as without it and the optimizer tail on every N-th iteration only, on the MEAN of the N micro-batch
gradients -- the effective batch is N times the reference's per-domain tables (code/train.py:35-45), which the launch plans, lane
budgets and tuned routes are built for and which therefore stay as they are.

It cannot be had by "not zeroing the gradient": the writers of the gradient arena overwrite (csrc/wgrad.hip's split reduction stores
with beta baked into its descriptors) and rd_zero at the head of every step is part of the contract of the writers that add.  So the
running sum lives in a second fp32 arena, and ONE launch per iteration stands between the encoder backward and the tail: a copy at
the window's first micro-batch, a sum in between, and at the last one the mean written IN PLACE into the gradient arena, where
rd_adam_step, the guarded tail (ramdsir/guard.py) and the grouped Adam (ramdsir/optim.py) read it as they always did.

What follows from it: the device iteration counter, the schedule, the bias corrections and --avg_start count UPDATES; BatchNorm
normalises every micro-batch by its own statistics and moves its running statistics at every iteration (what a torch loop with
(loss / N).backward() does); with the guard on, norm, clip and verdict are those of the mean gradient and a skipped window rolls the
BatchNorm buffers back over all N forward passes.  The launch is the first call of TrainStep.enqueue_tail (ramdsir/step.py, which says
where the native call is cut and in which order the tail runs): within an open window it is the only one.

    GradAccum.enqueue(stream) -> bool   one rd_grad_accum call (one launch); True at the window's last micro-batch
    GradAccum.next_is_boundary()        whether the next enqueue() completes a window
    model(grads_list)                   the numpy model of a whole window, in the kernel's order: bit for bit
    window(grads_list)                  the same launch by launch: the accumulator behind every micro-batch, then the mean
    updates_of(iterations, steps)       (optimizer updates, trailing iterations that complete no window)
    GradAccum.named_ranges()            [('accum/arena', acc)] for a training-state snapshot (ramdsir/ckpt.py)
"""
import numpy as np
import torch

from . import _lib as L
from .range_table import stream_handle

MAX_STEPS = L.ACCUM_MAX_STEPS


def check_steps(steps):
    """steps as the kernel receives it: an integer in 1..65536."""
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= MAX_STEPS:
        raise ValueError('grad accum: steps %r (a number of micro-batches per update, 1..%d)' % (steps, MAX_STEPS))
    return int(steps)


def inv_steps(steps):
    """(float)(1.0 / steps): the factor of the window's last launch, formed once in float64 and rounded once."""
    return np.float32(1.0 / float(int(steps)))


def updates_of(iterations, steps):
    """(optimizer updates, trailing iterations that complete no window and are never applied) of a run of `iterations`."""
    return int(iterations) // int(steps), int(iterations) % int(steps)


def model(grads_list):
    """rd_grad_accum over one window, in numpy: what the gradient arena holds behind the launch of the last micro-batch, from the N
    micro-batch gradients in their order.  The three cases as the kernel runs them -- acc = g_0 (the bits); acc = acc + g_k for
    0 < k < N - 1; (acc + g_{N-1}) * float32(1 / N) -- every sum and the product a float32 operation rounded on its own.  N == 1:
    the gradient itself (nothing is launched)."""
    return window(grads_list)[-1]


def window(grads_list):
    """model() launch by launch: a list of N arrays -- entry k < N - 1 is what the accumulator arena holds behind the launch of
    micro-batch k, entry N - 1 what the gradient arena holds behind the last one (model()'s result)."""
    f32 = np.float32
    gs = [np.asarray(g, f32) for g in grads_list]
    n = check_steps(len(gs))
    if n == 1:
        return [gs[0].copy()]
    out = [gs[0].copy()]                                    # k == 0: the bits as they are
    with np.errstate(all='ignore'):
        for g in gs[1:-1]:
            out.append((out[-1] + g).astype(f32))           # 0 < k < N - 1
        s = (out[-1] + gs[-1]).astype(f32)                  # k == N - 1: the sum, then the product, each rounded on its own
        out.append((s * inv_steps(n)).astype(f32))
    return out


def run(grad_ptr, acc_ptr, n, k, steps, inv, stream=None):
    """One rd_grad_accum call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_grad_accum(grad_ptr, acc_ptr, n, k, steps, float(inv), stream_handle(stream))


class GradAccum:
    """The accumulator arena of a FusedTrainer, the host-side position in the window and the one launch per iteration.  The position
    is host state: every launch argument but k is the same at every iteration, and k is a function of the number of enqueue() calls."""

    def __init__(self, trainer, steps):
        self.steps = check_steps(steps)
        self.inv = inv_steps(self.steps)
        self.trainer, self.bank = trainer, trainer.bank
        self.acc = torch.zeros_like(self.bank.grads)
        self.micro = 0

    def settings(self):
        """What a snapshot records and --resume compares."""
        return dict(steps=self.steps)

    def position(self):
        """The number of micro-batches of the open window that have been accumulated: 0 at a window's start."""
        return self.micro

    def set_position(self, micro):
        """After a restore: the position the snapshotted process had reached (the arena comes from the file)."""
        if not 0 <= int(micro) < self.steps:
            raise ValueError('grad accum: position %r is outside a window of %d' % (micro, self.steps))
        self.micro = int(micro)

    def next_is_boundary(self):
        """Whether the next enqueue() is the window's last micro-batch, the one behind which the optimizer tail runs."""
        return self.micro == self.steps - 1

    def enqueue(self, stream):
        """The launch behind whatever `stream` holds (the encoder backward, every lane joined).  True at the window's last micro-batch:
        the gradient arena then holds the mean and the caller (TrainStep.enqueue_tail) goes on with the tail."""
        k = self.micro
        L.check(L.lib().rd_grad_accum(self.bank.grads.data_ptr(), self.acc.data_ptr(), self.bank.n, k, self.steps, float(self.inv), stream),
                'rd_grad_accum')
        self.micro = (k + 1) % self.steps
        return k == self.steps - 1

    def model(self, grads_list):
        """model() over a window of this object's length."""
        if len(grads_list) != self.steps:
            raise ValueError('grad accum: %d gradients for a window of %d' % (len(grads_list), self.steps))
        return model(grads_list)

    def named_ranges(self):
        """[(name, tensor)] for ckpt.TrainState's extra ranges: the arena, which a snapshot in mid-window must carry."""
        return [('accum/arena', self.acc)]
