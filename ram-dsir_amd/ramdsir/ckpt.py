"""Resumable training (train.py --ckpt_every / --resume): the whole state of a FusedTrainer -- parameters, both Adam moments, every
BatchNorm buffer, the device-side iteration counter and the schedule words -- gathered by ONE HIP entry point (rd_snapshot,
csrc/snapshot.hip) into one contiguous device buffer with two 64-bit checksums per range, copied to pinned memory on a side stream
beside the next epoch's steps, and written by a thread: <path>.tmp, flush, fsync, os.replace -- a process killed at any time leaves
either the previous complete file or the new one.  The reference has no counterpart: it writes three state_dicts (code/train.py:342-360)
and never reads one back into a trainer.

The file (torch.save of plain containers): format / version, the range table (name, dtype, shape, offset, bytes, the two checksums),
the blob as one uint8 tensor, the host meta (epoch, iter_num, previous_best, the three host generators, the replay state of every
cycled loader, the byte length of the validation CSV) and the fingerprint of the run (arguments, geometry, parameter manifest).
`state_dicts(state)` turns it into the reference's three state_dicts without a GPU.  With train.py --avg_weights the ranges of the
averaged model ('avg/...', ramdsir/avg.py) follow the trainer's and its settings sit under meta['avg_weights'] (compare_avg_weights);
with --clip_grad_norm / --skip_nonfinite the guard's state word ('guard/state', ramdsir/guard.py) follows those and its max_norm sits
under meta['grad_guard'] (compare_grad_guard); the settings of the grouped Adam (--weight_decay, --wd_mode, --lr_schedule,
--warmup_iters, --enc_lr_mult; ramdsir/optim.py) sit under meta['optim'] (compare_optim) -- it adds no range: its state is the
arenas, the counter and the schedule words; with --accum_steps N > 1 the accumulator arena ('accum/arena', ramdsir/accum.py) goes behind
the other extra ranges (with the guard on, its shadow copies of the BatchNorm buffers too: in mid-window they differ from the live
ones) and N and the position in the window sit under meta['grad_accum'] (compare_grad_accum).

Checksums of the little-endian uint32 words w[0 .. m) of a range: s1 = sum w[i], s2 = sum (i + 1) w[i], both mod 2^64 (`checksums`
is the numpy model the kernel equals bit for bit; s2 depends on the order of the words, s1 does not).
"""
import os
import queue
import random
import threading
import time
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import range_table as R
from .optim import DEFAULTS as OPTIM_DEFAULTS               # the reference's optimizer: what a file without the record was taken under

FORMAT, VERSION = 'ramdsir-train-state', 1
SUM_BYTES = 8 * L.SNAP_SUM_STRIDE         # of the sums buffer per range
ALIGN = 16                      # every range starts on a 16-byte boundary of the blob: the kernel's wide path on both sides
MODULE_KEYS = (('enc', 'encoder_state_dict'), ('dec', 'seg_decoder_state_dict'), ('rec', 'rec_decoder_state_dict'))   # save_checkpoint's
FINGERPRINT_FIELDS = ('dataset', 'domain_idxs', 'test_domain_idx', 'batch_sizes', 'H', 'W', 'total_iters', 'dtype', 'consistency',
                      'lambda_rec', 'lr', 'num_classes', 'in_channels', 'activation', 'manifest')


# ------------------------------------------------------------------------------------------------------------- the numpy model
def checksums(data):
    """(s1, s2) of a buffer whose length is a multiple of 4 bytes, as Python ints in [0, 2^64)."""
    w = np.frombuffer(data, dtype='<u4') if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view('<u4').reshape(-1)
    s1 = s2 = 0
    # block by block, so that the widened words and their products stay in the cache: with the words v[j] of the block that starts at
    # word b, sum (b + j + 1) v[j] = b sum v[j] + sum (j + 1) v[j]; uint64 array arithmetic wraps mod 2^64 by itself
    for b in range(0, w.size, _BLOCK):
        v = w[b:b + _BLOCK].astype(np.uint64)
        a = int(v.sum(dtype=np.uint64))
        s1 += a
        s2 += b * a + int(np.dot(v, _WEIGHTS[:v.size]))
    return s1 % (1 << 64), s2 % (1 << 64)


_BLOCK = 1 << 15
_WEIGHTS = np.arange(1, _BLOCK + 1, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------- rd_snapshot
def build_table(entries):
    """[(device pointer, bytes, staging offset)] -> (the rd_snap_range_t array with its chunk0 column filled in, total chunks)."""
    return R.build(L.RdSnapRange, L.SNAP_CHUNK, [dict(ptr=ptr, bytes=nbytes, offset=off) for ptr, nbytes, off in entries], 'bytes')


upload_table = R.upload


def run(arr, table_dev, n, chunks, staging_ptr, staging_bytes, sums_ptr, direction, stream=None):
    """One rd_snapshot call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_snapshot(arr, table_dev.data_ptr() if table_dev is not None else None, n, chunks, staging_ptr, staging_bytes,
                               sums_ptr, direction, R.stream_handle(stream))


def read_sums(buf, n):
    """[(s1, s2)] of n ranges out of rd_snapshot's sums buffer (a uint8 or int64 tensor on any device): one line of SNAP_SUM_STRIDE
    64-bit words per range, the first two of them the sums."""
    a = buf.contiguous().view(torch.uint8)[:SUM_BYTES * n].cpu().numpy().view('<u8').reshape(n, L.SNAP_SUM_STRIDE)
    return [(int(r[0]), int(r[1])) for r in a]


def layout(named):
    """[(name, tensor)] -> the range table without sums: name, dtype, shape, offset (rounded up to ALIGN), bytes; and the blob size."""
    table, off = [], 0
    for name, t in named:
        nbytes = R.check_words(name, t)
        table.append(dict(name=name, dtype=str(t.dtype).replace('torch.', ''), shape=list(t.shape), offset=off, bytes=nbytes))
        off = (off + nbytes + ALIGN - 1) // ALIGN * ALIGN
    return table, off


def trainer_ranges(trainer):
    """The range set of a FusedTrainer, in the file's fixed order."""
    bank, ts = trainer.bank, trainer.ts
    return ([('params', bank.params), ('exp_avg', bank.exp_avg), ('exp_avg_sq', bank.exp_avg_sq)] +
            [('buffer/%s/%s' % k, t) for k, t in bank.buffers.items()] + [('iter', ts.iter), ('hyper', ts.hyper)])


def trainer_manifest(trainer):
    """[module, key, shape, kind, dtype] of every state_dict entry, modules in arena order, keys in the specs' (= state_dict) order."""
    mods = (('enc', trainer.modules['enc']), ('dec', trainer.modules['dec']), ('rec', trainer.modules['rec']))
    return [[m, key, list(shape), kind, str(dt).replace('torch.', '')] for m, mod in mods for key, shape, kind, dt in mod._specs]


def fingerprint(args, trainer, bsl, domain_idx_list, H, W, total_iters):
    """What a snapshot can be resumed under: train.py's arguments that shape the run, and the geometry.  --epochs is in it through
    total_iters (the poly schedule and the stopping point both depend on it)."""
    return OrderedDict([
        ('dataset', args.dataset), ('domain_idxs', [int(d) for d in domain_idx_list]), ('test_domain_idx', int(args.test_domain_idx)),
        ('batch_sizes', [int(b) for b in bsl]), ('H', int(H)), ('W', int(W)), ('total_iters', int(total_iters)),
        ('dtype', 'bf16' if trainer.ts.dtype == torch.bfloat16 else 'f32'),
        ('consistency', args.consistency_type if args.consistency else None), ('lambda_rec', float(args.lambda_rec)),
        ('lr', float(args.lr)), ('num_classes', int(args.num_classes)), ('in_channels', int(args.in_channels)),
        ('activation', args.activation), ('manifest', trainer_manifest(trainer))])


def compare_fingerprints(saved, current):
    """ValueError naming the FIRST field (in FINGERPRINT_FIELDS order) in which the file and this run differ."""
    for f in FINGERPRINT_FIELDS:
        a, b = saved.get(f), current.get(f)
        if a != b:
            if f == 'manifest':
                a, b = next(((x, y) for x, y in zip(a or [], b or []) if x != y), (len(a or []), len(b or [])))
            raise ValueError('--resume: the snapshot was taken with %s = %r, this run has %r' % (f, a, b))


AVG_PREFIX = 'avg/'             # the ranges of the averaged model (ramdsir/avg.py named_ranges)
AVG_SETTINGS = ('mode', 'decay', 'start')
GUARD_PREFIX = 'guard/'         # the state word of the guarded step (ramdsir/guard.py named_ranges)
GUARD_SETTINGS = ('max_norm',)


def _compare_ranged(state, current, key, prefix, fields, noun, a_noun, flags):
    """The rule of a stage that brings ranges of its own (`prefix`) and a record of settings (meta[key], `fields`): ValueError naming
    `key` where the file has no such ranges and the run wants them, has them and the run does not, or was taken under other settings.
    noun / a_noun: what the ranges hold, without and with its article; flags: the command-line flags that switch the stage on."""
    saved = (state.get('meta') or {}).get(key)
    has = any(e['name'].startswith(prefix) for e in state['table'])
    if current is not None and not (has and saved):
        raise ValueError('--resume: the snapshot holds no %s (it was taken without %s); this run has %s = %r' % (noun, flags, key, dict(current)))
    if current is None and (has or saved):
        raise ValueError('--resume: the snapshot holds %s (%s = %r); this run was started without %s'
                         % (a_noun, key, {k: saved.get(k) for k in fields} if saved else None, flags))
    if current is not None:
        for k in fields:
            if saved.get(k) != current.get(k):
                raise ValueError('--resume: the snapshot was taken with %s %s = %r, this run has %r' % (key, k, saved.get(k), current.get(k)))


def compare_avg_weights(state, current):
    """--resume with / without --avg_weights.  current: the run's settings (avg.WeightAverage.settings()) or None when the flag is off.
    An average cannot be made up, dropped or continued under another rule in the middle of a run.  --avg_bn_recal K travels in the
    same record (bn_recal; absent = 0, the pass off): it brings no range -- every epoch's pass uses that epoch's own batches -- but it
    shapes <target>_val_log_avg.csv and the keep-best of the averaged model, so a file and a run that disagree about K are refused."""
    _compare_ranged(state, current, 'avg_weights', AVG_PREFIX, AVG_SETTINGS, 'averaged model', 'an averaged model', '--avg_weights')
    saved = ((state.get('meta') or {}).get('avg_weights') or {}).get('bn_recal') or 0
    now = (current or {}).get('bn_recal') or 0
    if saved != now:
        raise ValueError('--resume: the snapshot was taken with avg_weights bn_recal = %r (--avg_bn_recal), this run has %r' % (saved, now))


def compare_grad_guard(state, current):
    """--resume with / without --clip_grad_norm / --skip_nonfinite.  current: the run's settings (guard.GradGuard.settings()) or None
    when the guard is off.  The count of skipped steps shapes Adam's bias corrections and cannot be made up or dropped, and a changed
    clipping norm is another optimizer in the middle of a run."""
    _compare_ranged(state, current, 'grad_guard', GUARD_PREFIX, GUARD_SETTINGS, 'guard state', 'a guard state',
                    '--clip_grad_norm / --skip_nonfinite')


def compare_optim(state, current):
    """--resume with / without the optimizer flags (--weight_decay, --wd_mode, --lr_schedule, --warmup_iters, --enc_lr_mult).
    current: the run's settings (optim.GroupedAdam.settings()) or None when every flag has its default.  The settings travel under
    meta['optim']; a file without the record was taken under the defaults and resumes only under them.  ValueError naming the first
    field in which file and run differ: another decay, schedule or multiplier is another optimizer in the middle of a run."""
    saved = dict(OPTIM_DEFAULTS, **((state.get('meta') or {}).get('optim') or {}))
    now = dict(OPTIM_DEFAULTS, **(current or {}))
    for k in OPTIM_DEFAULTS:
        if saved[k] != now[k]:
            raise ValueError('--resume: the snapshot was taken with optim %s = %r, this run has %r' % (k, saved[k], now[k]))


ACCUM_PREFIX = 'accum/'         # the accumulator arena of --accum_steps (ramdsir/accum.py named_ranges)


def compare_grad_accum(state, current):
    """--resume with / without --accum_steps.  current: the run's settings (accum.GradAccum.settings()) or None when N is 1.  The
    record travels under meta['grad_accum'] = dict(steps=N, micro=k) -- k the position in the window the snapshot was taken at, which
    the restore hands to GradAccum.set_position; a file without the record was taken with N = 1 and resumes only so.  ValueError
    naming grad_accum where file and run differ in N (the counter, the schedule and a half-filled arena all mean something else under
    another N), or where the record and the file's ranges contradict one another.  Returns the position to continue at."""
    saved = (state.get('meta') or {}).get('grad_accum')
    has = any(e['name'].startswith(ACCUM_PREFIX) for e in state['table'])
    was = int(saved['steps']) if saved else 1
    now = int(current['steps']) if current else 1
    if was != now:
        raise ValueError('--resume: the snapshot was taken with grad_accum steps = %d, this run has %d' % (was, now))
    if has != (was > 1):
        raise ValueError('--resume: the snapshot records grad_accum steps = %d but %s' % (was, 'holds an accumulator arena' if has else
                                                                                          'holds no accumulator arena'))
    micro = int(saved.get('micro', 0)) if saved else 0
    if not 0 <= micro < was:
        raise ValueError('--resume: the snapshot records grad_accum micro = %d in a window of %d' % (micro, was))
    return micro


# ------------------------------------------------------------------------------------------------------------- the file
def check_version(state):
    if not isinstance(state, dict) or state.get('format') != FORMAT:
        raise ValueError('not a training-state snapshot (format %r)' % (state.get('format') if isinstance(state, dict) else type(state)))
    if state.get('version') != VERSION:
        raise ValueError('training-state snapshot of format version %r; this build reads version %d' % (state.get('version'), VERSION))


def verify_blob(table, blob):
    """Recompute both checksums of every range from the blob's bytes; ValueError naming the first range that differs."""
    a = blob.numpy() if isinstance(blob, torch.Tensor) else np.asarray(blob)
    for e in table:
        if e['offset'] + e['bytes'] > a.size:
            raise ValueError('range %s ends at byte %d of a blob of %d' % (e['name'], e['offset'] + e['bytes'], a.size))
        got = checksums(a[e['offset']:e['offset'] + e['bytes']])
        if got != (e['s1'], e['s2']):
            raise ValueError('training-state snapshot: range %s is corrupt (checksums %x %x, recorded %x %x)'
                             % (e['name'], got[0], got[1], e['s1'], e['s2']))


def make_state(table, blob, meta, fp):
    return dict(format=FORMAT, version=VERSION, table=table, blob=blob, meta=meta, fingerprint=fp)


def write_file(path, state, seconds=None):
    """<path>.tmp, flush, fsync, os.replace: `path` is the previous complete file or the new one at every instant."""
    t0 = time.perf_counter()
    tmp = path + '.tmp'
    torch.save(state, tmp)              # by NAME: the archive writer then copies the blob out of the tensor without the interpreter lock
    t1 = time.perf_counter()
    fd = os.open(tmp, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)
    os.replace(tmp, path)
    if seconds is not None:
        seconds['serialise'] += t1 - t0
        seconds['write'] += time.perf_counter() - t1


def load_file(path):
    """The state of `path`, version and every range's checksums verified (the file is this program's own pickle: replay lists hold
    whatever the loaders yielded)."""
    state = torch.load(path, map_location='cpu', weights_only=False)
    check_version(state)
    verify_blob(state['table'], state['blob'])
    return state


def range_tensor(state, name):
    """A range of the blob as a tensor VIEW of its dtype and shape."""
    e = next(e for e in state['table'] if e['name'] == name)
    return state['blob'][e['offset']:e['offset'] + e['bytes']].view(getattr(torch, e['dtype'])).view(e['shape'])


def state_dicts(state):
    """The reference's three state_dicts (save_checkpoint's keys, each in its module's state_dict order) as views of the blob."""
    params, off = range_tensor(state, 'params'), 0
    out = OrderedDict((k, OrderedDict()) for _, k in MODULE_KEYS)
    names = dict(MODULE_KEYS)
    for m, key, shape, kind, dt in state['fingerprint']['manifest']:
        if kind == 'param':
            n = int(np.prod(shape, dtype=np.int64))
            out[names[m]][key] = params[off:off + n].view(shape)
            off += n
        else:
            out[names[m]][key] = range_tensor(state, 'buffer/%s/%s' % (m, key))
    return out


# ------------------------------------------------------------------------------------------------------------- host generators
def host_rng_state():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return dict(python=random.getstate(), numpy=(kind, keys.tolist(), int(pos), int(has_gauss), float(cached)), torch=torch.get_rng_state())


def set_host_rng_state(s):
    random.setstate(tuple(tuple(x) if isinstance(x, list) else x for x in s['python']))
    kind, keys, pos, has_gauss, cached = s['numpy']
    np.random.set_state((kind, np.asarray(keys, dtype=np.uint32), pos, has_gauss, cached))
    torch.set_rng_state(s['torch'])


# ------------------------------------------------------------------------------------------------------------- the cycled loaders
class ReplayCycle:
    """itertools.cycle with a state that can be saved: the same observable sequence -- iter(iterable) is taken at construction, the
    first pass yields and remembers the iterable's items, every later pass replays them -- and the same persistence across epochs.
    The reference's loop keeps one quirk alive through it: zip(*loaders) pulls one item from the cycled loaders in front of the longest
    loader in the round in which the longest one ends, and that item is lost; the position below simply moves on, as cycle's does.

    state() -> (saved items, position of the next item).  It raises while the first pass has yielded fewer than len(iterable) items:
    the live iterator of a first pass cannot be saved.  That cannot happen at an epoch boundary -- an epoch pulls at least
    len(longest loader) >= len(this loader) items from every cycled loader -- which is where train.py snapshots.  A cycle that has
    yielded exactly len(iterable) items has not yet SEEN its iterator end; from_state builds a cycle over an exhausted iterator, and the
    two continue alike: the next item is saved[0]."""

    def __init__(self, iterable, length=None):
        self._it = iter(iterable)
        self._saved, self._pos = [], 0
        self._len = len(iterable) if length is None else length

    @classmethod
    def from_state(cls, state):
        saved, pos = state
        self = cls((), length=len(saved))
        self._it, self._saved, self._pos = None, list(saved), int(pos) % max(len(saved), 1)
        return self

    def __iter__(self):
        return self

    def __next__(self):
        if self._it is not None:
            try:
                item = next(self._it)
                self._saved.append(item)
                return item
            except StopIteration:
                self._it = None
        if not self._saved:
            raise StopIteration
        item = self._saved[self._pos]
        self._pos = (self._pos + 1) % len(self._saved)
        return item

    def state(self):
        if self._it is not None and len(self._saved) < self._len:
            raise RuntimeError('ReplayCycle.state: the first pass has yielded %d of %d items' % (len(self._saved), self._len))
        return list(self._saved), self._pos


# ------------------------------------------------------------------------------------------------------------- the trainer's state
class TrainState:
    """The ranges of one FusedTrainer with everything a snapshot needs, allocated once: the device staging buffer (the blob, then the
    n lines of sums behind it, so ONE copy brings both to the host), its pinned twin, the device range table, a side stream and the writer
    thread.  snapshot() costs the training stream one rd_snapshot; restore() is upload() + scatter()."""

    def __init__(self, trainer, fp=None, extra=None):
        """extra: [(name, tensor)] appended behind trainer_ranges(trainer) -- device ranges that belong to the run's state without
        belonging to the trainer (the averaged model of --avg_weights: avg.WeightAverage.named_ranges())."""
        if getattr(trainer, '_graphs', False):
            raise RuntimeError('TrainState: a captured hipGraph replays a fixed launch list (use_graph=True)')
        self.trainer, self.fingerprint = trainer, fp
        self.named = trainer_ranges(trainer) + list(extra or ())
        self.table, self.blob_bytes = layout(self.named)
        self.n = n = len(self.named)
        dev = trainer.bank.device
        self.dev = torch.zeros(self.blob_bytes + SUM_BYTES * n, dtype=torch.uint8, device=dev)
        self.host = torch.zeros(self.blob_bytes + SUM_BYTES * n, dtype=torch.uint8).pin_memory()
        self.arr, self.chunks = build_table([(t.data_ptr(), e['bytes'], e['offset']) for (_, t), e in zip(self.named, self.table)])
        self.table_dev = upload_table(self.arr, n, dev)
        with torch.cuda.device(dev):
            self.side = torch.cuda.Stream(device=dev)
        self.seconds = dict(calls=0, gather=0.0, wait=0.0, checksum=0.0, serialise=0.0, write=0.0)
        self._q, self._thread, self._error = queue.Queue(), None, None

    # ---- device side
    def _run(self, direction):
        L.check(run(self.arr, self.table_dev, self.n, self.chunks, self.dev.data_ptr(), self.blob_bytes,
                    self.dev.data_ptr() + self.blob_bytes, direction), 'rd_snapshot')

    def gather(self):
        self._run(0)

    def device_sums(self):
        """[(s1, s2)] of the last gather / scatter (synchronises)."""
        return read_sums(self.dev[self.blob_bytes:], self.n)

    # ---- snapshot
    def snapshot(self, path, meta):
        """Wait until the previous snapshot's file is durable (one staging buffer: back-pressure), gather on the current stream, start
        the copy to pinned memory on the side stream behind the gather, hand the rest to the writer thread.  Only reads the trainer's
        buffers: training is bit-identical with and without it."""
        self.wait()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        self.gather()
        ev1.record()
        self.side.wait_event(ev1)
        done = torch.cuda.Event()
        with torch.cuda.stream(self.side):
            self.host.copy_(self.dev, non_blocking=True)
            done.record()
        if self._thread is None:
            self._thread = threading.Thread(target=self._writer, name='ckpt-writer', daemon=True)
            self._thread.start()
        self._q.put((done, ev0, ev1, path, meta))

    def host_state(self, meta):
        """The file's containers over the PINNED buffer (no copy), every range's host checksum compared with the device's."""
        host_sums = read_sums(self.host[self.blob_bytes:], self.n)
        blob = self.host[:self.blob_bytes]
        table = [dict(e, s1=s[0], s2=s[1]) for e, s in zip(self.table, host_sums)]
        verify_blob(table, blob)
        return make_state(table, blob, meta, self.fingerprint)

    def _writer(self):
        while True:
            item = self._q.get()
            try:
                if item is None:
                    return
                done, ev0, ev1, path, meta = item
                sec = self.seconds
                t0 = time.perf_counter()
                done.synchronize()
                t1 = time.perf_counter()
                state = self.host_state(meta)
                t2 = time.perf_counter()
                write_file(path, state, sec)
                sec['calls'] += 1
                sec['gather'] += ev0.elapsed_time(ev1) * 1e-3
                sec['wait'] += t1 - t0
                sec['checksum'] += t2 - t1
            except BaseException as e:              # noqa: BLE001 -- reported by the next wait() on the training thread
                self._error = e
            finally:
                self._q.task_done()

    def wait(self):
        """Until every handed-over snapshot is durable; re-raises what the writer thread met."""
        self._q.join()
        if self._error is not None:
            e, self._error = self._error, None
            raise RuntimeError('the snapshot writer failed: %r' % (e,)) from e

    def close(self):
        self.wait()
        if self._thread is not None:
            self._q.put(None)
            self._thread.join()
            self._thread = None

    def report(self):
        s, n = self.seconds, max(self.seconds['calls'], 1)
        return ('ckpt: %d snapshots of %.1f MB in %d ranges; per snapshot: gather (device) %.3f ms, wait for the copy %.2f ms, checksums '
                '%.2f ms, serialise + write %.2f ms, fsync + replace %.2f ms'
                % (s['calls'], self.blob_bytes / 1e6, self.n, 1e3 * s['gather'] / n, 1e3 * s['wait'] / n, 1e3 * s['checksum'] / n,
                   1e3 * s['serialise'] / n, 1e3 * s['write'] / n))

    # ---- restore
    def check(self, state):
        check_version(state)
        if self.fingerprint is not None and state.get('fingerprint') is not None:
            compare_fingerprints(state['fingerprint'], self.fingerprint)
        mine = [(e['name'], e['dtype'], e['shape'], e['offset'], e['bytes']) for e in self.table]
        theirs = [(e['name'], e['dtype'], list(e['shape']), e['offset'], e['bytes']) for e in state['table']]
        if mine != theirs or state['blob'].numel() != self.blob_bytes:
            bad = next((b for a, b in zip(mine, theirs) if a != b), None)
            raise ValueError('the snapshot\'s range table does not fit this trainer (%d ranges against %d; first difference: %r)'
                             % (len(theirs), len(mine), bad))

    def upload(self, state):
        """The manifest checked, the blob in the device staging buffer (stream-ordered on the current stream)."""
        self.wait()
        self.check(state)
        self.host[:self.blob_bytes].copy_(state['blob'])
        self.dev[:self.blob_bytes].copy_(self.host[:self.blob_bytes], non_blocking=True)

    def scatter(self, state):
        """Staging -> the trainer's buffers; the checksums of the words written against the file's (ValueError naming the range), the
        packed weights rebuilt, the module parameters aliased to the arena again where something replaced one."""
        self._run(1)
        for e, got in zip(state['table'], self.device_sums()):
            if got != (e['s1'], e['s2']):
                raise ValueError('restore: range %s arrived corrupt on the device (checksums %x %x, recorded %x %x)'
                                 % (e['name'], got[0], got[1], e['s1'], e['s2']))
        tr = self.trainer
        tr.ts.wpack.refresh()
        for mname, m in tr.modules.items():
            cur = m._named_tensors()
            for key, shape, kind, dt in m._specs:
                dst = tr.bank.p(mname, key) if kind == 'param' else tr.bank.b(mname, key)
                if cur[key].data_ptr() != dst.data_ptr():
                    cur[key].data = dst

    def restore(self, state):
        self.upload(state)
        self.scatter(state)
