"""Weight averaging along the training trajectory (train.py --avg_weights; rd_avg_step, csrc/avg.hip): a second copy of the model that
one HIP launch behind every training step moves towards the live one -- an exponential moving average, or the uniform average of every
iterate from a start iteration on (SWAD's dense averaging).  The reference has no counterpart: it keeps the last iterate and selects
model_%.2f.pth from single-iterate Dice figures on the held-out domain (code/train.py:331-350).

The pass only reads the trainer's buffers (parameters, BatchNorm buffers, the device-side iteration counter): the trained model is
bit-identical with and without it.  BatchNorm running statistics are averaged like parameters, num_batches_tracked is copied.  A
BatchNorm re-estimation pass is made on request only (train.py --avg_bn_recal K, ramdsir/avg_bn.py): it re-estimates the statistics
of the averaged encoder and seg decoder from the last K batches of an epoch into a third set of buffers, which the averaged model's
validation and checkpoints then read; the buffers averaged here, and a training-state snapshot of them, are not touched by it.

    WeightAverage.enqueue(stream)   one rd_avg_step call (one launch); every argument is the same at every step
    model(avg, live, s, ...)        the numpy model of the kernel's fp32 arithmetic: bit for bit
    WeightAverage.state_dicts()     the reference's three state_dicts of the averaged model
    WeightAverage.eval_forward()    infer.EvalForward over the averaged bank (its own weight pack)
    WeightAverage.named_ranges()    the averaged ranges for a training-state snapshot (ramdsir/ckpt.py)
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import engine as E
from . import range_table as R

MODES = {'ema': L.AVG_EMA, 'uniform': L.AVG_UNIFORM}


def one_minus_decay(decay):
    """The EMA weight as the kernel receives it: formed in float32 from the float32 of `decay`."""
    return np.float32(1) - np.float32(decay)


def model(avg, live, s, mode, decay=0.999, start=0):
    """rd_avg_step on one fp32 (kind 0) range, in numpy: the averaged words after the pass that follows the s-th completed step.
    k = s - 1 - start.  k <= 0: a copy of `live` (the bits as they are).  k > 0: d = p - a; t = w * d; a + t -- three float32 operations,
    each rounded on its own (no fma) -- with w = 1 - decay in float32 ('ema') or float32(1) / float32(k + 1) ('uniform')."""
    f32 = np.float32
    p, a = np.asarray(live, f32), np.asarray(avg, f32)
    k = int(s) - 1 - int(start)
    if k <= 0:
        return p.copy()
    w = one_minus_decay(decay) if MODES[mode] == L.AVG_EMA else f32(1) / f32(k + 1)
    with np.errstate(all='ignore'):
        d = (p - a).astype(f32)
        t = (w * d).astype(f32)
        return (a + t).astype(f32)


def build_table(entries):
    """[(src pointer, dst pointer, bytes, kind)] -> (the rd_avg_range_t array with its chunk0 column filled in, total chunks)."""
    return R.build(L.RdAvgRange, L.AVG_CHUNK, [dict(src=src, dst=dst, bytes=nbytes, kind=kind) for src, dst, nbytes, kind in entries], 'bytes')


upload_table = R.upload


def run(arr, table_dev, n, chunks, iter_ptr, mode, w, start, stream=None):
    """One rd_avg_step call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_avg_step(arr, table_dev.data_ptr() if table_dev is not None else None, n, chunks, iter_ptr, mode, float(w), start,
                               R.stream_handle(stream))


class AveragedBank(E.ParamBank):
    """The second bank: the live bank's layout (index, module ranges, buffer keys) over a parameter arena and BatchNorm buffers of its
    own, initialised as copies.  No gradient and no Adam arenas: nothing trains on it.  What infer.EvalForward, engine.WeightPack and
    step.state_dict_of read of a ParamBank is here."""

    def __init__(self, live):
        self.device, self.index, self.module_range, self.n = live.device, live.index, live.module_range, live.n
        self.params = live.params.detach().clone()
        self.grads = self.exp_avg = self.exp_avg_sq = None
        self.buffers = {k: t.detach().clone() for k, t in live.buffers.items()}


def bank_ranges(live, avg):
    """[(name, live tensor, averaged tensor, kind)]: the parameter arena as ONE fp32 range, then every buffer -- fp32 buffers (the running
    statistics) are averaged, other dtypes (the int64 num_batches_tracked) are copied."""
    out = [('avg/params', live.params, avg.params, L.AVG_F32)]
    for (m, key), t in live.buffers.items():
        out.append(('avg/buffer/%s/%s' % (m, key), t, avg.buffers[(m, key)], L.AVG_F32 if t.dtype == torch.float32 else L.AVG_COPY))
    return out


class WeightAverage:
    """The averaged copy of a FusedTrainer's model and the one launch that maintains it.  mode: 'ema' (decay in (0, 1)) or 'uniform';
    start: the iteration count from which on iterates are averaged -- until then, and for the first averaged point, the copy equals the
    live model.  Data parallel: rank-local, like the BatchNorm buffers; no collective."""

    def __init__(self, trainer, mode='ema', decay=0.999, start=0):
        if mode not in MODES:
            raise ValueError('avg_weights: mode %r (ema or uniform)' % (mode,))
        if mode == 'ema' and not 0.0 < float(one_minus_decay(decay)) < 1.0:
            raise ValueError('avg_weights: decay %r is outside (0, 1) in float32' % (decay,))
        if int(start) < 0 or int(start) >= 1 << 31:
            raise ValueError('avg_weights: start %r' % (start,))
        self.trainer, self.mode, self.decay, self.start = trainer, mode, float(decay), int(start)
        self.w = one_minus_decay(decay) if mode == 'ema' else np.float32(0)
        self.live, self.iter = trainer.bank, trainer.ts.iter
        self.bank = AveragedBank(self.live)
        self.ranges = bank_ranges(self.live, self.bank)
        self.n = len(self.ranges)
        self.arr, self.chunks = build_table([(a.data_ptr(), b.data_ptr(), R.check_words(name, a, b), kind) for name, a, b, kind in self.ranges])
        self.table_dev = upload_table(self.arr, self.n, self.live.device)       # once: the pointers never move
        self._forward = {}
        self.bn_recal = None                    # FusedTrainer.enable_avg_bn_recal: the avg_bn.BnRecal that re-estimates this model's BatchNorm

    def settings(self):
        """What a snapshot records and --resume compares (bn_recal: the K of --avg_bn_recal, recorded only where the pass is on)."""
        out = dict(mode=self.mode, decay=self.decay if self.mode == 'ema' else None, start=self.start)
        if self.bn_recal is not None:
            out['bn_recal'] = self.bn_recal.settings()
        return out

    def enqueue(self, stream=None):
        """The pass behind whatever `stream` holds: one rd_avg_step call."""
        L.check(run(self.arr, self.table_dev, self.n, self.chunks, self.iter.data_ptr(), MODES[self.mode], self.w, self.start, stream),
                'rd_avg_step')

    def model(self, avg, live, s):
        """model() with this object's mode, decay and start."""
        return model(avg, live, s, self.mode, self.decay, self.start)

    def state_dicts(self):
        """The reference's three state_dicts of the averaged model: save_checkpoint's keys, each module's entries in its state_dict
        order with the live model's shapes and dtypes (copies).  With --avg_bn_recal the encoder / seg-decoder BatchNorm buffers are the
        re-estimated ones (avg_bn.BnRecal.state_dicts(): the same keys and order, the same parameters)."""
        if self.bn_recal is not None:
            return self.bn_recal.state_dicts()
        from .ckpt import MODULE_KEYS
        from .step import state_dict_of
        return OrderedDict((key, state_dict_of(self.bank, m, self.trainer.modules[m]._specs)) for m, key in MODULE_KEYS)

    def eval_forward(self, dtype=None):
        """infer.EvalForward over the averaged bank, one per storage dtype (default: the module path's, as EvalForward.from_trainer).
        It owns its weight pack: refresh() repacks the averaged weights and recomputes the frozen BatchNorm coefficients once per pass.
        With --avg_bn_recal: the forward over the re-estimated statistics (avg_bn.BnRecal.eval_forward())."""
        if self.bn_recal is not None:
            return self.bn_recal.eval_forward(dtype)
        from . import infer, modules as M
        dtype = M.storage_dtype() if dtype is None else dtype
        fwd = self._forward.get(dtype)
        if fwd is None:
            enc, dec = self.trainer.modules['enc'], self.trainer.modules['dec']
            infer.EvalForward._check_modules(enc, dec)
            wpack = E.WeightPack(self.bank, [('enc', enc._specs), ('dec', dec._specs)], dtype)
            fwd = self._forward[dtype] = infer.EvalForward(self.bank, wpack, True, dtype, enc._c, enc._n, dec._k, enc._slope)
        return fwd

    def named_ranges(self):
        """[(name, tensor)] of the averaged copy, for ckpt.TrainState's extra ranges: 'avg/params', then 'avg/buffer/<module>/<key>'."""
        return [(name, b) for name, _, b, _ in self.ranges]
