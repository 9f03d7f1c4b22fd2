"""CPU-only tests of train.py --tb_hist (ramdsir/tb_hist.py; rd_hist in csrc/hist.hip; the histogram records of utils/tfevents.py):
the struct layouts against the C compiler, the exported symbols, the restated default bucket table, the numpy model against
np.histogram and against rows worked out by hand, the trimming rule, the event-file record byte by byte, the range table over a CPU
ParamBank of the real three modules, every validation code of the entry point (they come back before anything is launched, so no GPU
is needed) and train.py's refusals.  No GPU call."""
import ctypes
import importlib.util
import json
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, engine as E, tb_hist as H       # noqa: E402
from utils import tfevents as T                                 # noqa: E402

F32, F64 = np.float32, np.float64
RANGE_FIELDS = [n for n, _ in L.RdHistRange._fields_]
STATS_FIELDS = [n for n, _ in L.RdHistStats._fields_]
FLT_MAX = float(np.finfo(F32).max)
DBL_MAX = float(np.finfo(F64).max)


def _train_module():
    spec = importlib.util.spec_from_file_location('rd_train_hist', os.path.join(ROOT, 'ram-dsir_amd', 'train.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------------------- descriptors
def test_struct_layouts_match_the_c_compiler(tmp_path):
    offs = ''.join('printf("%%zu ", offsetof(rd_hist_range_t, %s));' % f for f in RANGE_FIELDS) + \
        ''.join('printf("%%zu ", offsetof(rd_hist_stats_t, %s));' % f for f in STATS_FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%%zu %%zu %%d %%d %%d ", sizeof(rd_hist_range_t), '
           'sizeof(rd_hist_stats_t), RD_HIST_CHUNK, RD_HIST_MAX_LIMITS, RD_HIST_MAX_RANGES);%s return 0;}' % offs)
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    assert ctypes.sizeof(L.RdHistRange) == out[0] == 24 and ctypes.sizeof(L.RdHistStats) == out[1] == 48 == H.STATS_BYTES
    assert (L.HIST_CHUNK, L.HIST_MAX_LIMITS, L.HIST_MAX_RANGES) == tuple(out[2:5]) and L.HIST_MAX_LIMITS == 4096 and H.CHUNK == L.HIST_CHUNK
    assert RANGE_FIELDS == ['src', 'count', 'chunk0'] and STATS_FIELDS == ['min', 'max', 'sum', 'sum_squares', 'num', 'nonfinite']
    assert [getattr(L.RdHistRange, f).offset for f in RANGE_FIELDS] == out[5:8] == [0, 8, 16]
    assert [getattr(L.RdHistStats, f).offset for f in STATS_FIELDS] == out[8:] == [0, 8, 16, 24, 32, 40]
    assert [H.STATS_DTYPE.fields[f][1] for f in STATS_FIELDS] == out[8:]


def test_the_symbols_are_exported():
    for name in ('rd_hist', 'rd_hist_workspace'):
        assert name in L.exported_symbols()
        assert getattr(L.lib(), name) is not None
    assert L.lib().rd_hist_workspace(0) == 0 and L.lib().rd_hist_workspace(-3) == 0 and L.lib().rd_hist_workspace(7) == 7 * 48


# ------------------------------------------------------------------------------------------------------------- the bucket table
def test_default_limits_restate_tensorflows_table():
    lim = H.default_limits()
    assert lim.dtype == F64 and len(lim) == 1551 and (lim[1:] > lim[:-1]).all()
    assert lim[775] == 0.0 and np.array_equal(lim[:775], -lim[:775:-1])
    assert lim[776] == 1e-12 and lim[-1] == DBL_MAX and lim[0] == -DBL_MAX and lim[-2] < 1e20 <= lim[-2] * 1.1
    pos = lim[776:-1]
    assert len(pos) == 774
    # every step is one rounded multiplication by the double nearest 1.1: the ratio is 1.1 within a few ulp
    assert (np.abs(pos[1:] / pos[:-1] - 1.1) <= 4 * np.finfo(F64).eps).all()
    assert len(H.check_limits(lim)) == 1551
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, np.inf], [np.nan, 1.0], np.zeros(4097)):
        with pytest.raises(ValueError):
            H.check_limits(bad)


# ------------------------------------------------------------------------------------------------------------- the model
def test_model_equals_np_histogram_on_random_data():
    rng = np.random.RandomState(5)
    lim = H.default_limits()
    v = (rng.standard_normal(20000) * 10.0 ** rng.uniform(-9, 3, 20000)).astype(F32)
    m = H.model(v, lim)
    ref, _ = np.histogram(v.astype(F64), bins=lim)
    # numpy's bin i is [lim[i], lim[i + 1]): the model's bucket i + 1 (upper edge lim[i + 1]); nothing lies below -DBL_MAX
    assert m['counts'].dtype == np.uint32 and m['counts'][0] == 0 and np.array_equal(m['counts'][1:], ref)
    assert m['num'] == 20000 == int(m['counts'].sum()) and m['nonfinite'] == 0
    d = v.astype(F64)
    assert (m['min'], m['max'], m['sum'], m['sum_squares']) == (d.min(), d.max(), d.sum(), (d * d).sum())


def test_model_rows_worked_out_by_hand():
    lim = H.default_limits()
    up = lambda v: int(np.flatnonzero(H.model(np.array([v], F32), lim)['counts'])[0])           # noqa: E731
    # +0.0 and -0.0: 776 limits (the negative ones and 0.0) are <= 0: bucket 776, whose upper edge is 1e-12
    assert up(0.0) == up(-0.0) == 776 and lim[776] == 1e-12
    both = H.model(np.array([0.0, -0.0], F32), lim)
    assert both['counts'][776] == 2 and both['num'] == 2 and both['min'] == both['max'] == both['sum'] == 0.0
    # a positive subnormal lies above 0.0 and below 1e-12: the same bucket; a negative one below 0.0: the bucket with upper edge 0.0
    assert up(1e-45) == 776 and up(-1e-45) == 775
    # FLT_MAX lies above the last limit below 1e20: every limit but DBL_MAX is <= it, the last bucket (upper edge DBL_MAX) without the
    # clamp; -FLT_MAX has only -DBL_MAX below it: bucket 1 (the table is antisymmetric, the rule is not: bucket 0 stays empty)
    assert up(FLT_MAX) == 1550 and lim[1549] < 1e20 < FLT_MAX < lim[1550] == DBL_MAX
    assert up(-FLT_MAX) == 1 and lim[0] == -DBL_MAX < -FLT_MAX < lim[1]
    # the float nearest 1e-12 lies below the double 1e-12, the next float above it: the comparison is made in double
    f = F32(1e-12)
    assert float(f) < 1e-12 < float(np.nextafter(f, F32(1))) and up(f) == 776 and up(np.nextafter(f, F32(1))) == 777
    # a small table of powers of two: a float that EQUALS a limit belongs to the bucket above it
    p2 = np.array([-2.0, -0.5, 0.25, 1.0, 4.0])
    m = H.model(np.array([0.25, 1.0, -2.0, -0.5], F32), p2)
    assert list(m['counts']) == [0, 1, 1, 1, 1]             # -2 -> 1, -0.5 -> 2, 0.25 -> 3, 1 -> 4
    # the two clamps: below the first limit -> bucket 0; above (or at) the last limit -> the last bucket
    m = H.model(np.array([-3.0, 5.0, 4.0, 3.0], F32), p2)
    assert list(m['counts']) == [1, 0, 0, 0, 3]
    # non-finite elements are counted apart and enter nothing else
    m = H.model(np.array([np.nan, np.inf, -np.inf, 1.5, -0.75], F32), p2)
    assert m['nonfinite'] == 3 and m['num'] == 2 and list(m['counts']) == [0, 1, 0, 0, 1]
    assert (m['min'], m['max'], m['sum'], m['sum_squares']) == (-0.75, 1.5, 0.75, 2.8125)
    m = H.model(np.array([np.nan, np.inf], F32), p2)
    assert m['nonfinite'] == 2 and m['num'] == 0 and not m['counts'].any() and m['min'] == m['max'] == m['sum'] == m['sum_squares'] == 0.0
    # an empty array
    m = H.model(np.zeros(0, F32), p2)
    assert m['num'] == m['nonfinite'] == 0 and len(m['counts']) == 5 and not m['counts'].any() and m['min'] == m['max'] == 0.0


def test_trimming_keeps_one_leading_empty_bucket():
    lim = np.arange(8, dtype=F64)
    assert H.trim(lim, np.array([0, 0, 0, 3, 0, 2, 0, 0])) == ([2.0, 3.0, 4.0, 5.0], [0, 3, 0, 2])
    assert H.trim(lim, np.array([4, 0, 1, 0, 0, 0, 0, 0])) == ([0.0, 1.0, 2.0], [4, 0, 1])           # starts at bucket 0: nothing in front
    assert H.trim(lim, np.array([0, 7, 0, 0, 0, 0, 0, 0])) == ([0.0, 1.0], [0, 7])
    assert H.trim(lim, np.array([0, 0, 0, 0, 0, 0, 0, 9])) == ([6.0, 7.0], [0, 9])
    assert H.trim(lim, np.zeros(8, np.uint32)) == ([0.0], [0])                                       # num == 0
    lims, counts = H.trim(lim, np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint32))
    assert all(type(x) is float for x in lims) and all(type(x) is int for x in counts)


# ------------------------------------------------------------------------------------------------------------- the event file
def _vint(n):
    assert 0 <= n < 1 << 14
    return bytes([n]) if n < 128 else bytes([n & 0x7f | 0x80, n >> 7])


HISTO = ('grads/encoder.convd1.conv1.weight', -1.5, 2.25, 5, 3.0, 9.5, [-1.0, 0.0, 1.0, 4.0], [1, 0, 3, 1])


def test_histogram_record_bytes_by_hand_and_round_trip(tmp_path):
    tag, mn, mx, num, total, sq, limits, counts = HISTO
    ev = T.encode_event(12.5, step=7, histos=[HISTO])
    d = lambda v: struct.pack('<d', float(v))                                                       # noqa: E731
    histo = (b'\x09' + d(mn) + b'\x11' + d(mx) + b'\x19' + d(num) + b'\x21' + d(total) + b'\x29' + d(sq) +      # fields 1..5, wire type 1
             b'\x32' + _vint(32) + b''.join(map(d, limits)) + b'\x3a' + _vint(32) + b''.join(map(d, counts)))   # fields 6, 7, packed
    value = b'\x0a' + _vint(len(tag)) + tag.encode() + b'\x2a' + _vint(len(histo)) + histo           # Value{tag = 1, histo = 5}
    summary = b'\x0a' + _vint(len(value)) + value                                                   # Summary{value = 1}
    want = b'\x09' + d(12.5) + b'\x10\x07' + b'\x2a' + _vint(len(summary)) + summary                 # Event{1, 2, summary = 5}
    assert ev == want
    with pytest.raises(ValueError):
        T.encode_histo(0, 0, 0, 0, 0, [0.0, 1.0], [1])
    # through the writer and the reader, mixed with scalar records, in order
    wr = T.SummaryWriter(str(tmp_path))
    wr.add_scalar('lr', 0.5, 3)
    wr.add_histogram_raw(tag, mn, mx, num, total, sq, limits, counts, 3)
    wr.add_histogram_raw('weights/x', min=0.0, max=0.0, num=0, sum=0.0, sum_squares=0.0, bucket_limits=[0.0], bucket_counts=[0], global_step=4)
    wr.add_scalar('lr', 0.25, 4)
    wr.close()
    evs = T.read_events(wr.path)
    assert [(e['step'], e['scalars'], e['images'], e['histos']) for e in evs[1:]] == [
        (3, [('lr', 0.5)], [], []),
        (3, [], [], [(tag, mn, mx, 5.0, total, sq, tuple(map(float, limits)), tuple(map(float, counts)))]),
        (4, [], [], [('weights/x', 0.0, 0.0, 0.0, 0.0, 0.0, (0.0,), (0.0,))]),
        (4, [('lr', 0.25)], [], [])]
    assert evs[0]['histos'] == [] and evs[0]['file_version'] == 'brain.Event:2'
    # a flipped byte inside the packed limits is caught by the record's checksum
    data = bytearray(open(wr.path, 'rb').read())
    data[data.index(d(4.0)) + 3] ^= 0x40
    bad = tmp_path / 'bad'
    bad.write_bytes(bytes(data))
    with pytest.raises(ValueError, match='corrupt record'):
        T.read_events(str(bad))


def test_queued_writer_keeps_the_order_of_scalars_images_and_histograms(tmp_path):
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    wr = T.QueuedWriter(str(tmp_path))
    fetched = []

    def fetch():
        fetched.append(1)
        return [HISTO, ('weights/b',) + HISTO[1:]], [('hist_nonfinite/grads', 3)]
    wr.add_scalars_at(0, [('lr', 1.0)])
    wr.add_images_at(0, lambda: [('train/Image', img)])
    wr.add_histograms_at(0, fetch)
    wr.add_scalars_at(2, [('lr', 0.5)])
    wr.add_histogram_raw('weights/c', *HISTO[1:], global_step=2)
    wr.add_images_at(2, lambda: [('train/GT', img)])
    wr.close()
    evs = T.read_events(wr.path)
    assert fetched == [1]
    assert [(e['step'], [s[0] for s in e['scalars']], [i[0] for i in e['images']], [h[0] for h in e['histos']]) for e in evs[1:]] == [
        (0, ['lr'], [], []), (0, [], ['train/Image'], []), (0, [], [], [HISTO[0]]), (0, [], [], ['weights/b']),
        (0, ['hist_nonfinite/grads'], [], []), (2, ['lr'], [], []), (2, [], [], ['weights/c']), (2, [], ['train/GT'], [])]
    assert evs[5]['scalars'] == [('hist_nonfinite/grads', 3.0)] and evs[3]['histos'][0][6:] == ((-1.0, 0.0, 1.0, 4.0), (1.0, 0.0, 3.0, 1.0))
    # the image timings keep their keys; the histogram ones have a key of their own
    assert wr.seconds['records'] == 2 and wr.seconds['calls'] == 2
    assert wr.seconds['histo']['records'] == 4 and wr.seconds['histo']['calls'] == 2
    # an error in the thread surfaces at close()
    wr = T.QueuedWriter(str(tmp_path / 'e'))
    wr.add_histograms_at(0, lambda: ([('x', 0, 0, 0, 0, 0, [0.0, 1.0], [1])], []))
    with pytest.raises(ValueError):
        wr.close()


# ------------------------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope='module')
def bank():
    mods = [('enc', E.encoder_specs()), ('dec', E.decoder_specs()), ('rec', E.rec_decoder_specs(16, 3, 3))]
    return E.ParamBank(mods, 'cpu')


def test_build_table_over_a_cpu_bank_of_the_real_modules(bank, golden_dir):
    man = json.load(open(os.path.join(golden_dir, 'state_manifest.json')))
    # the reference's state_dict names of the PARAMETERS (the BatchNorm buffers are no part of the arenas), in its order
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    names = ['%s.%s' % (m, k) for m in ('encoder', 'seg_decoder', 'rec_decoder') for k, _, _ in man[m] if not k.endswith(buffers)]
    assert len(names) == len(bank.index) > 100
    what = ('weights', 'grads', 'adam_m', 'adam_v')
    arr, chunks, tags, kinds = H.build_table(bank, what)
    n = len(names)
    assert len(arr) == len(tags) == len(kinds) == 4 * n <= L.HIST_MAX_RANGES
    arenas = dict(weights=bank.params, grads=bank.grads, adam_m=bank.exp_avg, adam_v=bank.exp_avg_sq)
    run = 0
    for j, kind in enumerate(what):
        assert tags[j * n:(j + 1) * n] == ['%s/%s' % (kind, nm) for nm in names] and set(kinds[j * n:(j + 1) * n]) == {kind}
        nxt = 0
        for e, ((m, key), (off, shape)) in zip(arr[j * n:(j + 1) * n], bank.index.items()):
            # arena order, every tensor exactly once, never merged: the ranges tile the arena
            assert off == nxt and e.count == int(np.prod(shape)) and e.src == arenas[kind].data_ptr() + 4 * off
            assert e.chunk0 == run
            run += -(-e.count // L.HIST_CHUNK)
            nxt += e.count
        assert nxt == bank.n
    assert chunks == run
    arr2, chunks2, tags2, _ = H.build_table(bank)
    assert tags2 == tags[:2 * n] and chunks2 * 2 == chunks
    assert [t for _, t, _, _, _ in H.entries(bank, ('grads',))] == tags[n:2 * n]
    with pytest.raises(ValueError):
        H.build_table(bank, ('weights', 'momentum'))
    assert H.parse_what('weights, adam_v') == ('weights', 'adam_v')
    for bad in ('', 'weights,', 'weights,grads,weights', 'grad'):
        with pytest.raises(ValueError):
            H.parse_what(bad)


# ------------------------------------------------------------------------------------------------------------- validation codes
class HostRig:
    """A table, limits and outputs whose pointers are HOST arrays: every call below is refused before a launch, nothing is
    dereferenced on the device side."""

    def __init__(self):
        Cn = L.HIST_CHUNK
        self.data = np.zeros(3 * Cn + 64, F32)
        base = self.data.ctypes.data
        self.rows = [dict(src=base, count=5), dict(src=base + 4 * 5, count=0), dict(src=base + 4 * 5, count=2 * Cn + 1), dict(src=base + 4, count=Cn)]
        self.arr, self.chunks = H.R.build(L.RdHistRange, Cn, self.rows, 'count')
        self.limits = np.array([-1.0, 0.0, 0.5, 8.0])
        self.out = [np.full(4 * 4, 7, np.uint32), np.full(4 * 6, 7.0, F64), np.full(self.chunks * 6, 7.0, F64)]
        self.dev = np.zeros(4 * 3, np.int64)                   # stands for the device copies: never read on a refusal

    def code(self, table=True, dev=True, n=4, chunks=None, limits=None, lim_host=True, lim_dev=True, n_limits=None, counts=0, stats=0, ws=0,
             rng=None):
        arr = (L.RdHistRange * 4).from_buffer_copy(self.arr)
        for i, k, v in rng or ():
            setattr(arr[i], k, v)
        lim = self.limits if limits is None else np.asarray(limits, F64)
        ptr = lambda a, off: None if off is None else a.ctypes.data + off                           # noqa: E731
        return L.lib().rd_hist(arr if table else None, self.dev.ctypes.data if dev else None, n, self.chunks if chunks is None else chunks,
                               lim.ctypes.data if lim_host else None, self.dev.ctypes.data if lim_dev else None,
                               len(lim) if n_limits is None else n_limits, ptr(self.out[0], counts), ptr(self.out[1], stats),
                               ptr(self.out[2], ws), None)


def test_every_validation_code_comes_back_before_a_launch():
    r = HostRig()
    assert r.chunks == 1 + 0 + 3 + 1 and [e.chunk0 for e in r.arr] == [0, 1, 1, 4]
    # -1: null pointers, n outside its interval, misaligned pointers
    assert r.code(table=False) == -1 and r.code(dev=False) == -1 and r.code(lim_host=False) == -1 and r.code(lim_dev=False) == -1
    assert r.code(counts=None) == -1 and r.code(stats=None) == -1 and r.code(ws=None) == -1
    assert r.code(n=0) == -1 and r.code(n=-1) == -1 and r.code(n=L.HIST_MAX_RANGES + 1) == -1
    assert r.code(counts=2) == -1 and r.code(stats=4) == -1 and r.code(ws=4) == -1
    # -2: the limits
    assert r.code(n_limits=1) == -2 and r.code(n_limits=0) == -2 and r.code(n_limits=L.HIST_MAX_LIMITS + 1) == -2
    for bad in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [-np.inf, 0.0], [np.nan, 1.0]):
        assert r.code(limits=bad) == -2, bad
    # -3: a range's pointer and count
    assert r.code(rng=[(0, 'src', None)]) == -3 and r.code(rng=[(1, 'src', None)]) == -3        # (an empty range's pointer counts too)
    assert r.code(rng=[(2, 'src', r.data.ctypes.data + 2)]) == -3 and r.code(rng=[(3, 'src', r.data.ctypes.data + 1)]) == -3
    assert r.code(rng=[(0, 'count', -1)]) == -3 and r.code(rng=[(3, 'count', 2 ** 31)]) == -3
    # -5: the chunk0 column and the total
    assert r.code(rng=[(1, 'chunk0', 0)]) == -5 and r.code(rng=[(2, 'chunk0', 2)]) == -5 and r.code(rng=[(0, 'chunk0', 1)]) == -5
    assert r.code(rng=[(0, 'count', L.HIST_CHUNK + 1)]) == -5 and r.code(rng=[(3, 'count', L.HIST_CHUNK + 1)]) == -5
    assert r.code(chunks=4) == -5 and r.code(chunks=6) == -5 and r.code(chunks=0) == -5 and r.code(n=3) == -5
    assert r.code(rng=[(3, 'count', 2 ** 31 - 1)]) == -5                                        # the largest count is admissible: the total is not
    # the order of the checks: pointers, limits, ranges
    assert r.code(counts=None, n_limits=1) == -1 and r.code(n_limits=1, rng=[(0, 'count', -1)]) == -2
    # nothing was written
    assert (r.out[0] == 7).all() and (r.out[1] == 7.0).all() and (r.out[2] == 7.0).all() and not r.data.any() and not r.dev.any()


# ------------------------------------------------------------------------------------------------------------- flags
BASE_ARGS = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
REFUSALS = [
    (['--tb_hist', '-1'], '--tb_hist takes a positive interval'),
    (['--tb_hist', '--tb_hist_what', 'weights,momentum'], "the unknown kind 'momentum'"),
    (['--tb_hist', '--tb_hist_what', 'weights,,grads'], 'an empty kind'),
    (['--tb_hist', '--tb_hist_what', ''], 'an empty kind'),
    (['--tb_hist', '--tb_hist_what', 'grads,grads'], 'names a kind twice'),
    (['--tb_hist_what', 'weights'], 'it needs --tb_hist'),
    (['--tb_hist', '0', '--tb_hist_what', 'weights'], 'it needs --tb_hist'),
    (['--tb_hist', '--norm', 'gn'], '--norm gn trains through the modules, which have no arenas'),
    (['--tb_hist', '5', '--norm', 'in'], '--norm in trains through the modules, which have no arenas'),
    (['--tb_hist', '--accum_steps', '2'], '--tb_hist does not go with --accum_steps'),
]


def test_parse_defaults_and_the_flags_it_goes_with(capsys):
    M = _train_module()
    a = M.parse_args(BASE_ARGS)
    assert a.tb_hist == 0 and a.tb_hist_what is None and not M.uses_tb_hist(a)
    M.check_args(a, 1)
    a = M.parse_args(BASE_ARGS + ['--tb_hist'])
    assert a.tb_hist == 100 and M.uses_tb_hist(a) and M.tb_hist_what(a) == ('weights', 'grads') == H.DEFAULT_WHAT
    a = M.parse_args(BASE_ARGS + ['--tb_hist', '7', '--tb_hist_what', 'weights,grads,adam_m,adam_v'])
    assert a.tb_hist == 7 and M.tb_hist_what(a) == H.KINDS
    M.check_args(a, 1)
    M.check_args(a, 8)                                                  # not refused under data parallelism
    M.check_args(M.parse_args(BASE_ARGS + ['--tb_hist', '--accum_steps', '1']), 1)
    a = M.parse_args(BASE_ARGS + ['--tb_hist', '2', '--tb_images', '--tb_every_iter', '--tb_health', '--clip_grad_norm', '1', '--skip_nonfinite',
                                  '--weight_decay', '0.01', '--enc_lr_mult', '0.25', '--avg_weights', 'ema', '--ckpt_every', '1'])
    M.check_args(a, 1)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        M.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--tb_hist [N]' in text and '--tb_hist_what LIST' in text and 'weights,grads,adam_m,adam_v' in text


@pytest.mark.parametrize('flags,match', REFUSALS)
def test_check_args_refusals_directly_and_through_main(flags, match, monkeypatch):
    M = _train_module()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match=match):
        M.check_args(M.parse_args(BASE_ARGS + flags), 1)
    # main() refuses before it touches the data root (which does not exist), a process group or the GPU
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: pytest.fail('a GPU call was made'))
    with pytest.raises(ValueError, match=match):
        M.main(M.parse_args(BASE_ARGS + flags))


def test_a_captured_graph_refuses_the_histograms_in_the_existing_wording():
    """FusedTrainer.enable_tb_hist under use_graph=True goes through TrainStep.refuse_fixed_list; neither needs a GPU to refuse."""
    from ramdsir import step as S, trainer as TR
    t = TR.FusedTrainer.__new__(TR.FusedTrainer)
    t._graphs, t.ts = True, S.TrainStep.__new__(S.TrainStep)
    with pytest.raises(RuntimeError, match='a captured hipGraph replays a fixed launch list, which has no place for the per-tensor histograms'):
        t.enable_tb_hist()
    with pytest.raises(RuntimeError, match='a captured hipGraph replays a fixed launch list'):
        t.arm_tb_hist()
    t._graphs, t._hist = False, None
    with pytest.raises(RuntimeError, match='enable_tb_hist\\(\\) first'):
        t.arm_tb_hist()
    t._hist_pending = None
    with pytest.raises(RuntimeError, match='no armed step'):
        t.take_tb_hist()
