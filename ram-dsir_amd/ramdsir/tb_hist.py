"""TensorBoard histograms of the training state (train.py --tb_hist): one histogram per parameter tensor of the four flat arenas of
engine.ParamBank -- weights, gradients and the two Adam moments -- counted by ONE HIP entry point (rd_hist, csrc/hist.hip) where the
arenas live, copied to pinned host memory behind an event, trimmed on the event-file writer's thread and written as HistogramProto
records (utils/tfevents.py add_histogram_raw).  No reference counterpart: the reference writes scalars and images only
(code/train.py:298-329).

TensorFlow, tensorboard and tensorboardX are not dependencies here and cannot be pinned, so what they do is RESTATED (parity
unpinned), as tb_images.py restates make_grid and add_image:

  * the bucket table (`default_limits`): TensorFlow's default histogram buckets in float64 -- v = 1e-12; while v < 1e20: append v,
    v *= 1.1; then DBL_MAX; the negated list reversed in front, 0.0 between the halves: 774 + 1 limits per sign, 1551 in all;
  * the bucket rule (`model`, the kernel): a value v lies in bucket min(#{i : limits[i] <= v}, len - 1) -- upper_bound, bucket b
    has the upper edge limits[b]; NaN and +-Inf are counted apart and enter nothing (TensorFlow would refuse them);
  * the trimming (`trim`): buckets [max(lo - 1, 0), hi] with lo / hi the first / last non-empty bucket, tensorboardX's rule for a
    raw histogram; a histogram without a finite value is written as the single bucket limit [0.0], count [0].

Tags are `<kind>/<module>.<key>`: kind in weights / grads / adam_m / adam_v, <module>.<key> the reference's state_dict names under
encoder. / seg_decoder. / rec_decoder. (tests/golden/state_manifest.json)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import range_table as R

CHUNK = L.HIST_CHUNK
KINDS = ('weights', 'grads', 'adam_m', 'adam_v')
DEFAULT_WHAT = ('weights', 'grads')
ARENA = dict(weights='params', grads='grads', adam_m='exp_avg', adam_v='exp_avg_sq')
MODULE = dict(enc='encoder', dec='seg_decoder', rec='rec_decoder')
STATS_FIELDS = tuple(name for name, _ in L.RdHistStats._fields_)
STATS_BYTES = C.sizeof(L.RdHistStats)
STATS_DTYPE = np.dtype([(f, '<f8') for f in STATS_FIELDS[:4]] + [(f, '<i8') for f in STATS_FIELDS[4:]])
assert STATS_DTYPE.itemsize == STATS_BYTES


def default_limits():
    """TensorFlow's default bucket limits as a float64 array (restated, parity unpinned)."""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(float(np.finfo(np.float64).max))
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, np.float64)


def check_limits(limits):
    a = np.ascontiguousarray(limits, np.float64)
    if a.ndim != 1 or not 2 <= a.size <= L.HIST_MAX_LIMITS or not np.isfinite(a).all() or not (a[1:] > a[:-1]).all():
        raise ValueError('bucket limits are 2 to %d finite, strictly ascending doubles' % L.HIST_MAX_LIMITS)
    return a


def parse_what(text):
    """'weights,grads' -> ('weights', 'grads'), in the order given; ValueError for an unknown, repeated or empty kind."""
    kinds = tuple(k.strip() for k in text.split(','))
    for k in kinds:
        if k not in KINDS:
            raise ValueError('--tb_hist_what takes a comma list over %s: %r holds %s' % (','.join(KINDS), text,
                                                                                          'the unknown kind %r' % k if k else 'an empty kind'))
    if len(set(kinds)) != len(kinds):
        raise ValueError('--tb_hist_what names a kind twice: %r' % text)
    return kinds


# ------------------------------------------------------------------------------------------------------------- the numpy model
def model(values, limits):
    """What rd_hist writes for one range, in numpy: {counts (uint32, one per limit), min, max, sum, sum_squares (float64, over the
    finite elements), num, nonfinite}."""
    limits = np.asarray(limits, np.float64)
    v = np.asarray(values, np.float32).reshape(-1)
    finite = np.isfinite(v)
    d = v[finite].astype(np.float64)
    b = np.minimum(np.searchsorted(limits, d, side='right'), len(limits) - 1)
    counts = np.bincount(b, minlength=len(limits)).astype(np.uint32)
    any_ = d.size > 0
    return dict(counts=counts, min=float(d.min()) if any_ else 0.0, max=float(d.max()) if any_ else 0.0,
                sum=float(d.sum()) if any_ else 0.0, sum_squares=float((d * d).sum()) if any_ else 0.0,
                num=int(d.size), nonfinite=int(v.size - d.size))


def trim(limits, counts):
    """tensorboardX's trimming of a raw histogram: -> (bucket limits, bucket counts) as lists over buckets [max(lo - 1, 0), hi]; an
    all-empty histogram is the single bucket ([0.0], [0])."""
    nz = np.flatnonzero(counts)
    if nz.size == 0:
        return [0.0], [0]
    lo, hi = max(int(nz[0]) - 1, 0), int(nz[-1]) + 1
    return [float(x) for x in limits[lo:hi]], [int(x) for x in counts[lo:hi]]


# ------------------------------------------------------------------------------------------------------------- the table
def entries(bank, what=DEFAULT_WHAT):
    """[(kind, tag, arena name, first element, elements)]: one entry per parameter tensor of bank.index in arena order, repeated for
    every kind of `what`.  Tensors are never merged."""
    out = []
    for kind in what:
        if kind not in KINDS:
            raise ValueError('unknown kind %r (one of %s)' % (kind, ', '.join(KINDS)))
        for (m, key), (off, shape) in bank.index.items():
            out.append((kind, '%s/%s.%s' % (kind, MODULE[m], key), ARENA[kind], off, int(np.prod(shape, dtype=np.int64))))
    return out


def build_table(bank, what=DEFAULT_WHAT):
    """-> (ctypes array of rd_hist_range_t, total chunks, [tag], [kind]).  src is the absolute address of the tensor in its arena,
    so the table is tied to the bank's allocations (they are never reallocated).  Works on a CPU bank (the tests)."""
    ent = entries(bank, what)
    if not 1 <= len(ent) <= L.HIST_MAX_RANGES:
        raise ValueError('rd_hist takes 1 to %d ranges, got %d' % (L.HIST_MAX_RANGES, len(ent)))
    if any(ARENA[k] in ('exp_avg', 'exp_avg_sq') for k in what):
        bank.ensure_adam()
    rows = [dict(src=getattr(bank, arena).data_ptr() + 4 * off, count=count) for _, _, arena, off, count in ent]
    arr, chunks = R.build(L.RdHistRange, CHUNK, rows, 'count')
    return arr, chunks, [e[1] for e in ent], [e[0] for e in ent]


def run(arr, table_dev, n, chunks, limits, limits_dev, out_stats_ptr, out_counts_ptr, ws_ptr, stream=None):
    """One rd_hist call (asynchronous on `stream`, a raw handle; the current stream's by default); returns the code."""
    return L.lib().rd_hist(arr, table_dev, n, chunks, limits.ctypes.data, limits_dev, len(limits), out_counts_ptr, out_stats_ptr, ws_ptr,
                           R.stream_handle(stream))


class Pending:
    """The histograms of one logging iteration on their way to the host.  `fetch()` (the writer thread) waits for the copy's event and
    returns (histograms, scalars): [(tag, min, max, num, sum, sum_squares, bucket limits, bucket counts)], trimmed, and
    [('hist_nonfinite/<kind>', total)] for every kind with a non-finite element in this iteration.  `raw()` returns the untrimmed
    (stats, counts) arrays.  Either hands the pinned buffer back to its TbHist."""

    def __init__(self, owner, host, event):
        self.owner, self.host, self.event, self._raw = owner, host, event, None

    def raw(self):
        """(stats: structured array of n records with rd_hist_stats_t's fields, counts: uint32 (n, n_limits)), copies."""
        if self._raw is None:
            o = self.owner
            self.event.synchronize()
            a = self.host.numpy()
            stats = a[:o.n * STATS_BYTES].view(STATS_DTYPE).copy()
            counts = a[o.n * STATS_BYTES:].view(np.uint32).reshape(o.n, o.n_limits).copy()
            host, self.host = self.host, None
            o._free.append(host)                                # the next enqueue reuses it
            self._raw = stats, counts
        return self._raw

    def fetch(self):
        o = self.owner
        stats, counts = self.raw()
        histos = []
        for i, tag in enumerate(o.tags):
            s = stats[i]
            lim, cnt = trim(o.limits, counts[i])
            histos.append((tag, float(s['min']), float(s['max']), int(s['num']), float(s['sum']), float(s['sum_squares']), lim, cnt))
        kinds = np.array(o.kinds)
        scalars = [('hist_nonfinite/%s' % k, int(stats['nonfinite'][kinds == k].sum())) for k in o.what]
        return histos, [(t, v) for t, v in scalars if v > 0]

    __call__ = fetch


class TbHist:
    """The table and its device copy, the uploaded limits, the device output (every range's statistics record, then every range's
    counts: one allocation, so one copy), the workspace and one pinned host buffer (a second one appears only while the writer
    thread still holds the first).  enqueue() is one rd_hist call, one asynchronous device-to-host copy and an event."""

    def __init__(self, bank, what=DEFAULT_WHAT, limits=None):
        self.what = tuple(what)
        self.limits = check_limits(default_limits() if limits is None else limits)
        self.n_limits = len(self.limits)
        self.arr, self.chunks, self.tags, self.kinds = build_table(bank, self.what)
        self.n, dev = len(self.tags), bank.device
        self.table_dev = R.upload(self.arr, self.n, dev)
        self.limits_dev = torch.from_numpy(self.limits.copy()).to(dev)
        self.out = torch.zeros(self.n * STATS_BYTES + self.n * self.n_limits * 4, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(max(L.lib().rd_hist_workspace(self.chunks) // 8, 1), dtype=torch.float64, device=dev)
        self._free = []
        self.copy_bytes = self.out.numel()

    def launch(self, stream=None):
        """The rd_hist call alone (scripts/tb_hist_bench.py times it)."""
        p = self.out.data_ptr()
        L.check(run(self.arr, self.table_dev.data_ptr(), self.n, self.chunks, self.limits, self.limits_dev.data_ptr(), p,
                    p + self.n * STATS_BYTES, self.ws.data_ptr(), stream), 'rd_hist')

    def enqueue(self, stream=None, copy=True):
        """rd_hist on `stream` (a raw handle: torch's current stream, where the copy goes, or None for it), then -- unless copy is
        False (a data-parallel rank that does not write) -- the copy of statistics and counts and an event.  Returns the Pending."""
        self.launch(stream)
        if not copy:
            return None
        host = self._free.pop() if self._free else torch.empty(self.out.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(self.out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return Pending(self, host, ev)
