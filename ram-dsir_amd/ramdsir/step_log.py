"""Per-step records from a device-resident ring (train.py --tb_every_iter / --tb_health; rd_step_log, csrc/step_log.hip).

The reference writes lr and its six loss scalars at EVERY iteration (code/train.py:298-304 Fundus, :467-473 Prostate), each read with
.item().  The fused step keeps them on the device; reading them every step would put a host synchronisation behind every step and end
the one-batch look-ahead of train.py.  Instead one small launch behind each step appends a row (losses, Adam's hyper parameters -- the lr
and the iteration number among them -- the restoration terms and, with health=True, the gradient norm of each Adam group plus the number of
non-finite gradient elements) to a ring on the device, and the host drains the ring where it synchronises anyway.

    StepLog.append(stream)   one rd_step_log call; the host owns the row counter
    StepLog.drain()          one device-to-host copy of the pending rows -> one record per iteration
    model_row(...)           the numpy model of the kernel (float64 sums in the order of ramdsir/sumsq.py, non-finite elements masked)
    rank_mean(rows, group)   data parallel: the mean over the ranks of the loss columns, as FusedTrainer.losses() forms it
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .step import loss_dict_of
from .sumsq import fold, partial_sums

ROW = L.LOG_ROW
LOSS, HYPER, REC, NORM, NONFINITE = slice(0, 8), slice(8, 12), slice(12, 28), slice(28, 31), 31       # the words of a row (include/ramdsir.h)
HEALTH_TAGS = ('health/grad_norm_encoder', 'health/grad_norm_seg_decoder', 'health/grad_norm_rec_decoder', 'health/nonfinite_grads')


def model_row(losses, rec_mse, hyper, grads=None, ranges=None, align_words=0):
    """The row rd_step_log writes, in numpy: grads None -> words 28..31 zero; otherwise per group the float32 of the float64 square root of
    the float64 sum of squares of its finite elements in the kernels' order (ramdsir/sumsq.py; chunks are counted from the start of the
    group), and the number of non-finite elements of all three groups.  align_words: (address of grads / 4) % 4."""
    row = np.zeros(ROW, np.float32)
    row[LOSS] = np.asarray(losses, np.float32)
    row[HYPER] = np.asarray(hyper, np.float32)
    rec = np.asarray(rec_mse, np.float32)
    assert rec.size <= L.LOG_MAX_REC
    row[12:12 + rec.size] = rec
    if grads is not None:
        g = np.asarray(grads, np.float32)
        bad = 0
        for k in range(3):
            part = g[ranges[k]:ranges[k + 1]]
            finite = np.isfinite(part)
            bad += int(part.size - finite.sum())
            sums, _ = partial_sums(part, (align_words + ranges[k]) & 3)
            row[28 + k] = np.float32(np.sqrt(fold(sums)))
        row[NONFINITE] = np.float32(bad)
    return row


def records_of(rows, dataset, lambda_rec, n_rec):
    """rows: float32 [n][32] on the host -> one record per row.  The loss dict goes through step.loss_dict_of on the same Python floats
    TrainStep.loss_dict() would read back (float32 widened to double), lr is what FusedTrainer.lr() returns: the records are EQUAL to those
    reads, not close to them."""
    out = []
    for row in np.asarray(rows, np.float32).reshape(-1, ROW):
        out.append({'iteration': int(row[11]), 'losses': loss_dict_of(dataset, lambda_rec, row[LOSS].tolist(), row[12:12 + n_rec].tolist()),
                    'lr': float(row[8]), 'norms': tuple(float(v) for v in row[NORM]), 'nonfinite': int(row[NONFINITE])})
    return out


def rank_mean(rows, group=None):
    """In place, collective: the loss and restoration columns of rows [n][32] become their mean over the ranks -- one all-reduce (sum) and
    a division by the world size, element for element what FusedTrainer.losses() does to the row of one step.  The hyper and health
    columns are left alone: they are computed from the averaged gradients and identical on every rank."""
    import torch.distributed as dist
    buf = torch.cat([rows[:, LOSS], rows[:, REC]], 1).contiguous()
    dist.all_reduce(buf, group=group)
    buf /= dist.get_world_size(group)
    rows[:, LOSS] = buf[:, :8]
    rows[:, REC] = buf[:, 8:]
    return rows


class StepLog:
    """The ring, the workspace of the health pass and the row counter.  losses [8], rec_mse [n_rec <= 16] and hyper [4] are the step's own
    device tensors; grads / ranges (the arena and the four offsets of its three Adam groups) switch the health pass on."""

    def __init__(self, losses, rec_mse, hyper, grads=None, ranges=None, rows=256):
        if rec_mse.numel() > L.LOG_MAX_REC:
            raise ValueError('a row holds %d restoration terms, got %d' % (L.LOG_MAX_REC, rec_mse.numel()))
        if rows < 1:
            raise ValueError('the ring needs at least one row')
        self.rows, self.n_rec = int(rows), rec_mse.numel()
        self.ring = torch.zeros(self.rows, ROW, dtype=torch.float32, device=losses.device)
        self._keep = (losses, rec_mse, hyper, grads)
        d = L.RdStepLog()
        d.losses, d.rec_mse, d.hyper, d.ring = losses.data_ptr(), rec_mse.data_ptr(), hyper.data_ptr(), self.ring.data_ptr()
        d.rows, d.n_rec = self.rows, self.n_rec
        self.partial = None
        if grads is not None:
            ranges = [int(v) for v in ranges]
            assert len(ranges) == 4 and 0 <= ranges[0] and ranges[3] <= grads.numel() and grads.dtype == torch.float32
            self.partial = torch.empty(L.lib().rd_step_log_workspace(ranges[3] - ranges[0]) // 8, dtype=torch.float64, device=grads.device)
            d.grads, d.partial = grads.data_ptr(), self.partial.data_ptr()
            for k in range(4):
                d.range[k] = ranges[k]
        self.desc = d
        self.appended = self.drained = 0

    @property
    def pending(self):
        return self.appended - self.drained

    def full(self):
        return self.pending >= self.rows

    def append(self, stream):
        """One row behind whatever `stream` holds.  A full ring is refused: the oldest row has not been read."""
        if self.full():
            raise RuntimeError('step log: %d rows pending in a ring of %d: drain() before the next step' % (self.pending, self.rows))
        self._launch(self.appended % self.rows, stream)
        self.appended += 1

    def _launch(self, row, stream):
        self.desc.row = row
        L.check(L.lib().rd_step_log(C.byref(self.desc), stream), 'rd_step_log')

    def spans(self):
        """The pending rows as at most two [first, last) spans of the ring, oldest first (two when they wrap)."""
        if self.pending > self.rows:
            raise RuntimeError('step log: %d rows pending in a ring of %d: rows have been overwritten' % (self.pending, self.rows))
        if not self.pending:
            return []
        a, n = self.drained % self.rows, self.pending
        return [(a, a + n)] if a + n <= self.rows else [(a, self.rows), (0, a + n - self.rows)]

    def take(self):
        """The pending rows, oldest first, as ONE tensor on the ring's device (a copy); the ring is empty afterwards."""
        sp = self.spans()
        self.drained = self.appended
        if not sp:
            return self.ring[:0].clone()
        return torch.cat([self.ring[a:b] for a, b in sp]) if len(sp) > 1 else self.ring[sp[0][0]:sp[0][1]].clone()

    def drain(self, dataset, lambda_rec, world=1, group=None):
        """Synchronises: one device-to-host copy.  world > 1: data parallel, collective -- the rows become the rank mean first (every rank
        holds the same number of pending rows: the drain points depend on the iteration number alone)."""
        rows = self.take()
        if world > 1 and rows.shape[0]:
            rank_mean(rows, group)
        return records_of(rows.cpu().numpy(), dataset, lambda_rec, self.n_rec)
