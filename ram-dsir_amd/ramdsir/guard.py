"""The guarded optimizer step (train.py --clip_grad_norm / --skip_nonfinite; rd_grad_guard, rd_guard_sync in csrc/guard.hip,
rd_adam_step_guarded in csrc/loss.hip).  The reference steps on whatever gradient `loss.backward()` leaves (code/train.py:285-287);
here, on request, the gradient of the whole arena is clipped by its global norm -- all three Adam groups jointly, as
torch.nn.utils.clip_grad_norm_ over the one optimizer: scale = min(1, max_norm / (norm + 1e-6)) -- and a step whose gradient holds a
NaN or an infinity, or whose norm is not finite as a float, leaves no trace in the model state: parameters and both moments stay, every
BatchNorm buffer the forward pass has moved is rolled back, Adam's bias corrections count the updates applied.  The iteration counter
still advances (the reference's lr is a function of iter_num, code/train.py:289).

Everything is decided on the device: the launches communicate through one 40-byte state word (rd_guard_state_t), every launch argument
is the same at every step, and the host reads the word only where it synchronises anyway.  The guard owns its own two calls only:
TrainStep.enqueue_tail (ramdsir/step.py: the one place that says where the native call is cut and in which order the tail runs) puts
the verdict in front of Adam and the sync behind the weight repack, and hands Adam the state word.

    GradGuard.enqueue_verdict(stream)   rd_grad_guard: norm, scale and skip into the state word
    GradGuard.enqueue_sync(stream)   rd_guard_sync: the roll-back of the BatchNorm buffers or the refresh of their shadows
    GradGuard.read()                 the state word as a dict (synchronises)
    GradGuard.sync_shadow()          shadow <- live, outside the step (at enable time, after a restore)
    model(grad, max_norm, state)     the numpy model of rd_grad_guard's two launches, in the summation order of ramdsir/sumsq.py
    GradGuard.named_ranges()         [('guard/state', tensor)] for a training-state snapshot (ramdsir/ckpt.py)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import range_table as R
from .sumsq import CHUNK, fold, partial_sums       # noqa: F401  (the summation order lives there; re-exported for the tests)

EPS = np.float32(1e-6)
STATE_FIELDS = tuple(name for name, _ in L.RdGuardState._fields_)
STATE_BYTES = C.sizeof(L.RdGuardState)


def workspace_bytes(n):
    """rd_grad_guard_workspace(n): one {double, int64} pair per chunk."""
    return -(-max(int(n), 0) // CHUNK) * 16


def check_max_norm(max_norm):
    """max_norm as the kernel receives it (float32): 0 switches clipping off; negative, NaN and infinite values are refused."""
    m = float(max_norm)
    if not 0.0 <= m <= float(np.finfo(np.float32).max):             # NaN fails both comparisons
        raise ValueError('grad guard: max_norm %r (0 for no clipping, or a positive finite number)' % (max_norm,))
    return m


def scale_of(norm, max_norm):
    """What a step that is not skipped multiplies its gradient by: min(1, max_norm / (norm + 1e-6)) as separately rounded float32
    operations; 1 with max_norm 0."""
    f32 = np.float32
    if not f32(max_norm) > 0:
        return f32(1)
    with np.errstate(all='ignore'):
        return min(f32(f32(max_norm) / f32(f32(norm) + EPS)), f32(1))


def model(grad, max_norm=0.0, state=None, align_words=0):
    """rd_grad_guard in numpy: the state word after the call, as a dict, from the word before it (None: all zero).  The norm is the
    float32 of the fp64 square root of the fp64 sum in the kernels' order (ramdsir/sumsq.py, over the arena as one group); scale is
    formed from separately rounded float32 operations."""
    f32 = np.float32
    sums, counts = partial_sums(grad, align_words)
    with np.errstate(all='ignore'):
        norm = f32(np.sqrt(fold(sums)))
    nonfinite = int(counts.sum())
    skip = nonfinite > 0 or not np.isfinite(norm)
    scale = f32(1) if skip else scale_of(norm, max_norm)
    prev = dict.fromkeys(STATE_FIELDS, 0) if state is None else state
    return dict(norm=float(norm), scale=float(scale), skip=int(skip), nonfinite=nonfinite, steps=int(prev['steps']) + 1,
                clipped=int(prev['clipped']) + int(scale < 1 and not skip), skipped=int(prev['skipped']) + int(skip))


def state_dict_of(raw):
    """40 bytes (bytes, or a uint8 / int64 array) -> the fields of rd_guard_state_t as Python numbers."""
    raw = bytes(raw) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).tobytes()
    s = L.RdGuardState.from_buffer_copy(raw[:STATE_BYTES])
    return {k: getattr(s, k) for k in STATE_FIELDS}


def bank_ranges(bank, shadows):
    """[(name, live tensor, shadow tensor)]: every BatchNorm buffer of the bank -- running_mean, running_var and the int64
    num_batches_tracked of all three modules -- in the bank's order.  The roll-back is a byte copy: the dtype does not matter."""
    return [('guard/shadow/%s/%s' % (m, key), t, shadows[(m, key)]) for (m, key), t in bank.buffers.items()]


def build_table(entries):
    """[(live pointer, shadow pointer, bytes)] -> (the rd_guard_range_t array with its chunk0 column filled in, total chunks)."""
    return R.build(L.RdGuardRange, L.GUARD_CHUNK, [dict(live=live, shadow=shadow, bytes=nbytes) for live, shadow, nbytes in entries], 'bytes')


upload_table = R.upload


def run_guard(desc, stream=None):
    """One rd_grad_guard call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_grad_guard(C.byref(desc) if desc is not None else None, R.stream_handle(stream))


def run_sync(arr, table_dev, n, chunks, state_ptr, stream=None):
    """One rd_guard_sync call; returns its code."""
    return L.lib().rd_guard_sync(arr, table_dev.data_ptr() if table_dev is not None else None, n, chunks, state_ptr, R.stream_handle(stream))


class GradGuard:
    """The state word, the workspace, the shadow copies of the BatchNorm buffers with their range table, and the two calls they serve in
    the tail of a FusedTrainer's step.  max_norm 0: the guard without clipping (--skip_nonfinite alone).  An active guard always skips non-finite
    steps.  Data parallel: the gradients are bit-identical on every rank behind the exchange, so every rank takes the same decision
    without a collective; the shadows are rank-local like the buffers they copy."""

    def __init__(self, trainer, max_norm=0.0):
        self.trainer, self.max_norm = trainer, check_max_norm(max_norm)
        self.bank = bank = trainer.bank
        if bank.n > L.GUARD_MAX_N:
            raise ValueError('grad guard: an arena of %d elements (rd_grad_guard takes up to %d)' % (bank.n, L.GUARD_MAX_N))
        dev = bank.device
        self.state = torch.zeros(STATE_BYTES // 8, dtype=torch.int64, device=dev)
        self.workspace = torch.empty(workspace_bytes(bank.n) // 8, dtype=torch.float64, device=dev)
        d = L.RdGradGuard()
        d.grad, d.n, d.max_norm = bank.grads.data_ptr(), bank.n, self.max_norm
        d.workspace, d.state = self.workspace.data_ptr(), self.state.data_ptr()
        self.desc = d
        self.shadows = {k: t.detach().clone() for k, t in bank.buffers.items()}
        self.ranges = bank_ranges(bank, self.shadows)
        self.n = len(self.ranges)
        self.arr, self.chunks = build_table([(a.data_ptr(), b.data_ptr(), R.check_words(name, a, b)) for name, a, b in self.ranges])
        self.table_dev = upload_table(self.arr, self.n, dev)            # once: the pointers never move

    def settings(self):
        """What a snapshot records and --resume compares."""
        return dict(max_norm=self.max_norm)

    def sync_shadow(self):
        """shadow <- live outside the step: the buffers as they are become what a skipped step rolls back to."""
        for _, live, shadow in self.ranges:
            shadow.copy_(live)

    def enqueue_verdict(self, stream):
        """The verdict on the gradient arena as `stream` (a raw stream handle) leaves it, into the state word: norm, scale, skip."""
        L.check(L.lib().rd_grad_guard(C.byref(self.desc), stream), 'rd_grad_guard')

    def enqueue_sync(self, stream):
        """Behind Adam and the repack: the roll-back of the BatchNorm buffers (a skipped step) or the refresh of the shadows."""
        L.check(L.lib().rd_guard_sync(self.arr, self.table_dev.data_ptr(), self.n, self.chunks, self.state.data_ptr(), stream), 'rd_guard_sync')

    def read(self):
        """The state word as a dict: norm, scale, skip, nonfinite of the last step; steps, clipped, skipped so far.  Synchronises."""
        return state_dict_of(self.state.cpu().numpy())

    def model(self, grad, state=None):
        """model() with this object's max_norm and the alignment of the trainer's gradient arena."""
        return model(grad, self.max_norm, state, align_words=(self.bank.grads.data_ptr() >> 2) & 3)

    def named_ranges(self):
        """[(name, tensor)] for ckpt.TrainState's extra ranges: the state word, whose `skipped` count Adam's bias corrections depend on.
        The shadows are not state: behind a completed step they equal the live buffers (sync_shadow() after a restore)."""
        return [('guard/state', self.state)]

    def shadow_ranges(self):
        """[(name, tensor)] of the shadow copies, 'guard/shadow/<module>/<key>': state only under gradient accumulation
        (ramdsir/accum.py), where a snapshot in mid-window finds them at the window's start while the live buffers have moved."""
        return [(name, shadow) for name, _, shadow in self.ranges]
