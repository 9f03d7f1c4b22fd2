"""The grouped Adam (train.py --weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult; rd_optim_step in
csrc/optim.hip).  The reference's optimizer is one hard-coded line -- Adam without weight decay, lr / 2 on the encoder, the poly
schedule with power 0.9 (code/train.py:573-576, 289-293; rd_adam_step) -- and the iteration counter and the schedule live on the
device.  Here torch's param_groups become a device table of contiguous ranges of the parameter arena, each with its own learning-rate
multiplier and weight decay, and the schedule is chosen by a field of the descriptor and evaluated on the device from the counter.  The
reference's optimizer is the two-range special case of this table, bit for bit.

The decay rule: tensors with more than one dimension (the convolution kernels) decay; 1-D tensors (biases, BatchNorm weight and bias)
are exempt.

The grouped step is not part of a launch list: it is the Adam of TrainStep.enqueue_tail (ramdsir/step.py, which says where the native
call is cut and in which order the tail runs), under the guard's state word where the guard (ramdsir/guard.py) is on as well.

    build_table(bank, enc_lr_mult, weight_decay)        the rd_optim_range_t array of a ParamBank (CPU or GPU) and its chunk count
    make_table(entries)                                 the same from [(first, count, lr_mult, weight_decay)]
    schedule_model(it, base_lr, total, schedule, warmup)    the prepare launch's hyper_out[0] in numpy float64
    decay_model(param, grad, lr, lr_mult, decay, wd_mode)   the two decay expressions in numpy float32
    GroupedAdam.enqueue(stream, guard_state_ptr)        one rd_optim_step call (two launches)
    GroupedAdam.settings()                              what a training-state snapshot records (ramdsir/ckpt.py compare_optim)
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from . import range_table as R

CHUNK = L.OPT_CHUNK
SCHEDULES = {'poly': L.OPT_POLY, 'cosine': L.OPT_COSINE, 'constant': L.OPT_CONSTANT}
WD_MODES = {'decoupled': L.OPT_DECOUPLED, 'l2': L.OPT_L2}
DEFAULTS = dict(weight_decay=0.0, wd_mode='decoupled', lr_schedule='poly', warmup_iters=0, enc_lr_mult=0.5)
SETTINGS = tuple(DEFAULTS)
F32_MAX = float(np.finfo(np.float32).max)


def check_settings(weight_decay, wd_mode, lr_schedule, warmup_iters, enc_lr_mult, total_iters=None):
    """The five settings as the kernel receives them (the two factors as float32): ValueError on what rd_optim_step would refuse."""
    if not 0.0 <= float(weight_decay) <= F32_MAX:                       # NaN fails both comparisons
        raise ValueError('optim: weight_decay %r (0, or a positive finite number)' % (weight_decay,))
    if wd_mode not in WD_MODES:
        raise ValueError('optim: wd_mode %r (one of %s)' % (wd_mode, ', '.join(WD_MODES)))
    if lr_schedule not in SCHEDULES:
        raise ValueError('optim: lr_schedule %r (one of %s)' % (lr_schedule, ', '.join(SCHEDULES)))
    if int(warmup_iters) < 0:
        raise ValueError('optim: warmup_iters %r (0, or a number of iterations)' % (warmup_iters,))
    if not 0.0 < float(enc_lr_mult) <= F32_MAX or float(np.float32(enc_lr_mult)) == 0.0:
        raise ValueError('optim: enc_lr_mult %r (a positive finite number)' % (enc_lr_mult,))
    if total_iters is not None and int(warmup_iters) >= int(total_iters):
        raise ValueError('optim: warmup_iters %d is not below the %d iterations of the run' % (warmup_iters, total_iters))


def make_table(entries):
    """[(first, count, lr_mult, weight_decay)] -> (the rd_optim_range_t array with its chunk0 column filled in, total chunks)."""
    return R.build(L.RdOptimRange, CHUNK, [dict(first=int(first), count=int(count), lr_mult=float(lr_mult), weight_decay=float(wd))
                                           for first, count, lr_mult, wd in entries], 'count')


def bank_entries(bank, enc_lr_mult=0.5, weight_decay=0.0):
    """One (first, count, lr_mult, weight_decay) per parameter tensor of bank.index in arena order -- lr_mult is enc_lr_mult inside
    module_range['enc'] and 1 elsewhere; weight_decay applies to tensors with more than one dimension (the conv kernels) and is 0 for
    1-D tensors (biases, BatchNorm weight / bias) -- with neighbours of equal settings merged.  Works on a CPU ParamBank."""
    e0, e1 = bank.module_range['enc']
    f32 = lambda x: float(np.float32(x))
    out = []
    for off, shape in sorted(bank.index.values(), key=lambda v: v[0]):
        count = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        if count < 1:
            continue
        mult = f32(enc_lr_mult) if e0 <= off < e1 else 1.0
        wd = f32(weight_decay) if len(shape) > 1 else 0.0
        if out and out[-1][0] + out[-1][1] == off and out[-1][2] == mult and out[-1][3] == wd:
            out[-1] = (out[-1][0], out[-1][1] + count, mult, wd)
        else:
            out.append((off, count, mult, wd))
    return out


def build_table(bank, enc_lr_mult=0.5, weight_decay=0.0):
    """bank_entries as (the rd_optim_range_t array, total chunks); len(array) is the number of ranges."""
    return make_table(bank_entries(bank, enc_lr_mult, weight_decay))


def upload_table(arr, device):
    return R.upload(arr, len(arr), device)


def schedule_model(it, base_lr, total, schedule='poly', warmup=0):
    """hyper_out[0] of the prepare launch at counter value `it`, as np.float32: everything in float64 (base_lr as the float32 the
    descriptor holds), rounded once.  poly carries the reference's one-iteration lag (the rate of iteration it was written behind
    iteration it - 1 from ITS number, code/train.py:289); cosine and constant do not."""
    it, total = int(it), int(total)
    sched = SCHEDULES[schedule] if isinstance(schedule, str) else int(schedule)
    s = 1.0
    if sched == L.OPT_POLY:
        if it > 0:
            s = math.pow(1.0 - float(it - 1) / float(total), 0.9)
    elif sched == L.OPT_COSINE:
        s = 0.5 * (1.0 + math.cos(math.pi * float(min(it, total)) / float(total)))
    w = min(1.0, float(it + 1) / float(warmup)) if warmup > 0 else 1.0
    return np.float32(float(np.float32(base_lr)) * s * w)


def decay_model(param, grad, lr, lr_mult, decay, wd_mode='decoupled'):
    """What the update launch does to (param, grad) of a range with multiplier lr_mult and decay > 0 in front of Adam's arithmetic,
    as float32 arrays: decoupled -- param * (1 - lr_g * decay) with lr_g = lr_mult * lr, three separately rounded float32 operations
    (torch.optim.AdamW); l2 -- grad = fma(decay, param, grad), formed in float64 (the product of two float32 is exact there) and
    rounded once (torch.optim.Adam(weight_decay)).  lr: hyper_out[0] of the step.  decay 0: both unchanged."""
    f32 = np.float32
    p, g = np.asarray(param, f32), np.asarray(grad, f32)
    d = f32(decay)
    if not d > 0:
        return p.copy(), g.copy()
    mode = WD_MODES[wd_mode] if isinstance(wd_mode, str) else int(wd_mode)
    with np.errstate(all='ignore'):
        if mode == L.OPT_DECOUPLED:
            lr_g = f32(lr_mult) * f32(lr)
            keep = f32(1) - f32(lr_g * d)
            return (p * keep).astype(f32), g.copy()
        return p.copy(), (np.float64(d) * p.astype(np.float64) + g.astype(np.float64)).astype(f32)


def run_step(desc, arr, table_dev, n_ranges, chunks, guard_ptr=None, stream=None):
    """One rd_optim_step call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_optim_step(C.byref(desc) if desc is not None else None, arr, table_dev.data_ptr() if table_dev is not None else None,
                                 n_ranges, chunks, guard_ptr, R.stream_handle(stream))


class GroupedAdam:
    """The descriptor, the range table and its device copy over a FusedTrainer's arenas, counter and schedule words (the ones
    rd_adam_step uses: the ring, the checkpoint's `hyper` range and FusedTrainer.lr() read them as ever).  Data parallel: behind the
    exchange the gradients are bit-identical on every rank, so there is no collective."""

    def __init__(self, trainer, weight_decay=0.0, wd_mode='decoupled', lr_schedule='poly', warmup_iters=0, enc_lr_mult=0.5):
        self.trainer, self.bank, self.ts = trainer, trainer.bank, trainer.ts
        ad = self.ts.ad
        check_settings(weight_decay, wd_mode, lr_schedule, warmup_iters, enc_lr_mult, ad.total_iters)
        self._settings = dict(weight_decay=float(weight_decay), wd_mode=wd_mode, lr_schedule=lr_schedule, warmup_iters=int(warmup_iters),
                              enc_lr_mult=float(enc_lr_mult))
        d = L.RdOptim()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n = ad.param, ad.grad, ad.exp_avg, ad.exp_avg_sq, ad.n
        d.iter, d.hyper_out = ad.iter, ad.hyper_out
        d.base_lr, d.total_iters, d.beta1, d.beta2, d.eps = ad.base_lr, ad.total_iters, ad.beta1, ad.beta2, ad.eps
        d.schedule, d.warmup_iters, d.wd_mode = SCHEDULES[lr_schedule], int(warmup_iters), WD_MODES[wd_mode]
        self.desc = d
        self.entries = bank_entries(self.bank, enc_lr_mult, weight_decay)
        self.n = len(self.entries)
        if self.n > L.OPT_MAX_RANGES:
            raise ValueError('optim: a table of %d ranges (rd_optim_step takes up to %d)' % (self.n, L.OPT_MAX_RANGES))
        self.arr, self.chunks = make_table(self.entries)
        self.table_dev = upload_table(self.arr, self.bank.device)       # once: the arena never moves

    def settings(self):
        """What a snapshot records and --resume compares."""
        return dict(self._settings)

    def decayed_elements(self):
        return sum(c for _, c, _, wd in self.entries if wd > 0)

    def enqueue(self, stream, guard_state_ptr=None):
        """The optimizer step behind whatever `stream` holds: the prepare launch and the update launch; under a guard's state word
        (TrainStep.enqueue_tail hands it over) with its scale, its skip and its count of applied updates."""
        L.check(L.lib().rd_optim_step(C.byref(self.desc), self.arr, self.table_dev.data_ptr(), self.n, self.chunks, guard_state_ptr, stream),
                'rd_optim_step')
