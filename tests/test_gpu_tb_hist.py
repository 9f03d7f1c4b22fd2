"""-m gpu: per-tensor histograms (train.py --tb_hist) -- rd_hist (csrc/hist.hip) against the numpy model of ramdsir/tb_hist.py on
ranges at every word alignment and at the chunk edges, in tables of 1, 7, 33 and 200 ranges over two arenas; twin trainers with and
without the histograms; the data-parallel step on one rank; the CLI against the same run without the flag and across a resume.

Every equality is exact.  The one bound, for `sum` and `sum_squares` on data whose sums are not exact in fp64: kernel and model add the
same n exact fp64 terms (a widened float; the square of one, 48 bits) in different orders; any order's error is at most
gamma(n - 1) * S with gamma(k) = k u / (1 - k u), u = 2^-53, S = the sum of the magnitudes (Higham, Accuracy and Stability, 4.2), so the
two differ by at most 2 gamma(n) S; S itself is computed in fp64, within a factor 1 + gamma(n) of the true one."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, tb_hist as H, range_table as R       # noqa: E402

F32, F64 = np.float32, np.float64
CH = L.HIST_CHUNK
SENT = 1024                                                 # words of a sentinel: 4 KiB
EDGES = [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 7]
LIMITS = {'default': H.default_limits(), 'two': np.array([-1.0, 1.0]),
          'pow2': np.array([-16.0, -2.0, -0.5, -2.0 ** -30, 0.0, 2.0 ** -30, 0.25, 1.0, 4.0, 16.0])}


def _sum_bound(n, magnitude):
    g = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    return 2 * g * magnitude * (1 + g)


# ------------------------------------------------------------------------------------------------------------- data
def _one_bucket(n, rng):
    return np.full(n, 0.5, F32)


def _dyadic(n, rng):
    return (rng.randint(-4096, 4097, n) * 2.0 ** -6).astype(F32)      # |k| <= 2^12: sums and sums of squares of 2^16 such values are exact


def _normal(n, rng):
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F32)     # twelve decades


def _planted(n, rng):
    v = _normal(n, rng)
    if n == 0:
        return v
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(sorted({0, n - 1, n // 2, min(CH - 1, n - 1), min(CH, n - 1), min(CH + CH // 2, n - 1)})):
        v[i] = bad[k % 3]                                   # a chunk's first, last and a middle element (and the range's)
    return v


DATA = dict(one_bucket=_one_bucket, dyadic=_dyadic, normal=_normal, planted=_planted)
EXACT = ('one_bucket', 'dyadic')


def _reachable():
    """One float32 per bucket of the default table that a finite float32 can reach: the smallest float >= the bucket's lower edge."""
    lim = LIMITS['default']
    vals, buckets = [], []
    with np.errstate(over='ignore'):
        for b in range(1, len(lim)):
            f = F32(lim[b - 1])
            if not float(f) >= lim[b - 1]:
                f = np.nextafter(f, F32(np.inf))
            if np.isfinite(f) and float(f) < lim[b]:
                vals.append(f)
                buckets.append(b)
    return np.array(vals, F32), buckets


# ------------------------------------------------------------------------------------------------------------- the rig
def _tables():
    """name -> [(elements, word alignment of src, arena)]: the edge lengths at the four alignments; 1, 7 and 200 ranges with an empty
    range in the middle and ranges that point into two arenas."""
    edges = [(n, a, (i + a) % 2) for a in range(4) for i, n in enumerate(EDGES)]
    edges.insert(16, (0, 2, 1))
    seven = [(5, 1, 0), (CH + 1, 3, 1), (3, 0, 0), (0, 2, 1), (CH - 1, 2, 0), (1, 3, 1), (3 * CH + 7, 1, 0)]
    small = [1, 3, 4, 5, 17, 257, 1000, 0, 4099, 64, 2, 7]
    many = [((EDGES[4 + (i // 25) % 4] if i % 25 == 24 else small[i % len(small)]), i % 4, (i // 3) % 2) for i in range(200)]
    many[100] = (0, 1, 0)
    return dict(one=[(3 * CH + 7, 1, 0)], seven=seven, edges=edges, many=many)


TABLES = _tables()


class Rig:
    """Two source arenas whose gaps and 4 KiB borders hold NaN (a read outside a range would show in `nonfinite`), and ONE output
    allocation [sentinel | stats | sentinel | counts | sentinel | workspace | sentinel] pre-filled with garbage."""

    def __init__(self, layout, data, limits, seed=3):
        rng = np.random.RandomState(seed)
        self.limits = np.ascontiguousarray(limits, F64)
        self.values = [DATA[data](n, rng) if isinstance(data, str) else np.asarray(data[i], F32) for i, (n, _, _) in enumerate(layout)]
        pos, place = [SENT, SENT], []
        for (n, align, arena) in layout:
            start = (pos[arena] + 3) // 4 * 4 + align       # arenas start at a 16-byte boundary (torch's allocator): src % 16 == 4 align
            place.append((arena, start))
            pos[arena] = start + n + 5                      # at least five words of NaN between neighbours
        host = [np.full(p + SENT, np.nan, F32) for p in pos]
        for v, (arena, start) in zip(self.values, place):
            host[arena][start:start + len(v)] = v
        self.host = host
        self.arenas = [torch.from_numpy(h).to(DEV) for h in host]
        rows = [dict(src=self.arenas[arena].data_ptr() + 4 * start, count=len(v)) for v, (arena, start) in zip(self.values, place)]
        assert all(r['src'] % 16 == 4 * a for r, (_, a, _) in zip(rows, layout))
        self.arr, self.chunks = R.build(L.RdHistRange, CH, rows, 'count')
        self.n, self.nl = len(layout), len(self.limits)
        self.table_dev = R.upload(self.arr, self.n, DEV)
        self.limits_dev = torch.from_numpy(self.limits.copy()).to(DEV)
        sb, cb, wb = self.n * H.STATS_BYTES, self.n * self.nl * 4, max(int(L.lib().rd_hist_workspace(self.chunks)), 8)
        self.off = np.cumsum([4 * SENT, sb, 4 * SENT, (cb + 7) // 8 * 8, 4 * SENT, wb, 4 * SENT])
        self.sizes = (sb, cb, wb)
        self.fill = torch.from_numpy(np.random.RandomState(9).randint(1, 255, int(self.off[-1])).astype(np.uint8)).to(DEV)
        self.out = self.fill.clone()

    def ptrs(self):
        p = self.out.data_ptr()
        return p + int(self.off[0]), p + int(self.off[2]), p + int(self.off[4])        # stats, counts, workspace

    def call(self, **edit):
        sp, cp, wp = self.ptrs()
        a = dict(table=self.arr, dev=self.table_dev.data_ptr(), n=self.n, chunks=self.chunks, lim=self.limits.ctypes.data,
                 lim_dev=self.limits_dev.data_ptr(), nl=self.nl, counts=cp, stats=sp, ws=wp)
        a.update(edit)
        return L.lib().rd_hist(a['table'], a['dev'], a['n'], a['chunks'], a['lim'], a['lim_dev'], a['nl'], a['counts'], a['stats'], a['ws'],
                               torch.cuda.current_stream().cuda_stream)

    def read(self):
        """(stats, counts, the bytes of both) with the sentinels and the source arenas checked."""
        torch.cuda.synchronize()
        o, f = self.out.cpu().numpy(), self.fill.cpu().numpy()
        sb, cb, wb = self.sizes
        s0, c0, w0 = int(self.off[0]), int(self.off[2]), int(self.off[4])
        keep = np.ones(len(o), bool)
        for lo, size in ((s0, sb), (c0, cb), (w0, wb)):
            keep[lo:lo + size] = False
        assert np.array_equal(o[keep], f[keep]), 'a sentinel of the output allocation was written'
        for a, h in zip(self.arenas, self.host):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), h.view(np.uint32)), 'a source arena was written'
        stats = o[s0:s0 + sb].view(H.STATS_DTYPE).copy()
        counts = o[c0:c0 + cb].view(np.uint32).reshape(self.n, self.nl).copy()
        return stats, counts, o[s0:s0 + sb].tobytes() + o[c0:c0 + cb].tobytes()

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.out, self.fill)


def _check(rig, exact):
    assert rig.call() == 0
    stats, counts, raw = rig.read()
    for i, v in enumerate(rig.values):
        m, s = H.model(v, rig.limits), stats[i]
        assert np.array_equal(counts[i], m['counts']), i
        assert int(counts[i].sum()) == m['num'] == s['num'] and s['nonfinite'] == m['nonfinite'], i
        assert s['min'] == m['min'] and s['max'] == m['max'], i
        if exact:
            assert s['sum'].tobytes() == F64(m['sum']).tobytes() and s['sum_squares'].tobytes() == F64(m['sum_squares']).tobytes(), i
        else:
            d = v[np.isfinite(v)].astype(F64)
            assert abs(s['sum'] - m['sum']) <= _sum_bound(len(d), np.abs(d).sum()), (i, s['sum'], m['sum'])
            assert abs(s['sum_squares'] - m['sum_squares']) <= _sum_bound(len(d), (d * d).sum()), (i, s['sum_squares'], m['sum_squares'])
    return stats, counts, raw


# ------------------------------------------------------------------------------------------------------------- kernel vs model
@pytest.mark.parametrize('data', sorted(DATA))
@pytest.mark.parametrize('table', sorted(TABLES))
def test_kernel_equals_the_model(table, data):
    rig = Rig(TABLES[table], data, LIMITS['default'])
    stats, counts, _ = _check(rig, data in EXACT)
    if data == 'one_bucket':                                # the worst case for the atomics: one bin takes every element
        b = int(np.searchsorted(rig.limits, 0.5, side='right'))
        for i, v in enumerate(rig.values):
            assert counts[i][b] == len(v) and int(counts[i].sum()) == len(v)
    if data == 'planted':
        assert all(stats[i]['nonfinite'] >= min(len(v), 1) for i, v in enumerate(rig.values))
    empty = [i for i, v in enumerate(rig.values) if len(v) == 0]
    assert (table == 'one') == (not empty)
    for i in empty:
        assert not counts[i].any() and stats[i].tobytes() == bytes(H.STATS_BYTES)


@pytest.mark.parametrize('limits', ['two', 'pow2'])
@pytest.mark.parametrize('data', ['dyadic', 'planted'])
def test_other_limit_tables(limits, data):
    """A 2-limit table (one comparison, the upper clamp on everything above -1) and a small power-of-two table, where dyadic data
    hits limits exactly and both clamps are exercised."""
    rig = Rig(TABLES['seven'], data, LIMITS[limits])
    _, counts, _ = _check(rig, data in EXACT)
    assert counts[:, 0].any() and counts[:, -1].any()


def test_one_value_per_reachable_bucket_of_the_default_table():
    vals, buckets = _reachable()
    assert buckets == list(range(1, 1551))                  # every bucket but the one below -DBL_MAX
    tiled = np.tile(vals, (3 * CH + 7) // len(vals) + 1)[:3 * CH + 7]
    rig = Rig([(len(vals), 1, 0), (len(tiled), 3, 1)], [vals, tiled], LIMITS['default'])
    _, counts, _ = _check(rig, False)
    assert counts[0][0] == 0 and (counts[0][1:] == 1).all()
    assert counts[1][0] == 0 and counts[1][1:].min() >= len(tiled) // len(vals)


def test_a_repeated_call_gives_identical_bytes():
    rig = Rig(TABLES['many'], 'planted', LIMITS['default'])
    _, _, first = _check(rig, False)
    rig.out.copy_(rig.fill.flip(0))                         # other garbage in counts, statistics and workspace
    rig.fill = rig.out.clone()
    _, _, second = _check(rig, False)
    assert first == second


def test_every_validation_code_leaves_outputs_and_sentinels_untouched():
    rig = Rig(TABLES['seven'], 'normal', LIMITS['pow2'])
    sp, cp, wp = rig.ptrs()

    def table(**edit):
        arr = (L.RdHistRange * rig.n).from_buffer_copy(rig.arr)
        for k, (i, v) in edit.items():
            setattr(arr[i], k, v)
        return arr

    def lim(*v):
        a = np.array(v, F64)
        rig._keep = a
        return dict(lim=a.ctypes.data, nl=len(a))
    assert rig.call(table=None) == -1 and rig.call(dev=None) == -1 and rig.call(lim=None) == -1 and rig.call(lim_dev=None) == -1
    assert rig.call(counts=None) == -1 and rig.call(stats=None) == -1 and rig.call(ws=None) == -1
    assert rig.call(n=0) == -1 and rig.call(n=L.HIST_MAX_RANGES + 1) == -1
    assert rig.call(counts=cp + 2) == -1 and rig.call(stats=sp + 4) == -1 and rig.call(ws=wp + 4) == -1 and rig.call(lim_dev=rig.limits_dev.data_ptr() + 4) == -1
    assert rig.call(nl=1) == -2 and rig.call(nl=L.HIST_MAX_LIMITS + 1) == -2
    assert rig.call(**lim(0.0, 0.0)) == -2 and rig.call(**lim(1.0, 0.0)) == -2 and rig.call(**lim(0.0, np.inf)) == -2 and rig.call(**lim(np.nan, 1.0)) == -2
    assert rig.call(table=table(src=(0, None))) == -3 and rig.call(table=table(src=(3, None))) == -3
    assert rig.call(table=table(src=(1, rig.arr[1].src + 2))) == -3 and rig.call(table=table(count=(2, -1))) == -3
    assert rig.call(table=table(count=(6, 2 ** 31))) == -3
    assert rig.call(table=table(chunk0=(1, 0))) == -5 and rig.call(table=table(chunk0=(4, 2))) == -5 and rig.call(table=table(count=(0, CH + 1))) == -5
    assert rig.call(chunks=rig.chunks + 1) == -5 and rig.call(chunks=rig.chunks - 1) == -5 and rig.call(chunks=0) == -5 and rig.call(n=6) == -5
    assert rig.untouched()
    _check(rig, False)                                      # ... and the valid call behind them all is the model's


# ------------------------------------------------------------------------------------------------------------- the trainer
from test_gpu_step_log import _trainer, _batches       # noqa: E402

BS, S, STEPS = [2, 3, 3], 32, 11
ALL = H.KINDS


def _state(tr, step_buffers=True):
    b = tr.bank
    return [b.params, b.exp_avg, b.exp_avg_sq] + ([b.grads, tr.ts.losses, tr.ts.rec_mse] if step_buffers else []) + list(b.buffers.values())


def _same_state(a, b, what, step_buffers=True):
    for k, (x, y) in enumerate(zip(_state(a, step_buffers), _state(b, step_buffers))):
        x, y = x.contiguous().reshape(-1), y.contiguous().reshape(-1)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (what, k)


def _expect(tr, hist, stats, counts, exact_only=False):
    """The pending result against model() over the arenas read back from `tr` (synchronised behind the same step)."""
    lim, b = hist.limits, tr.bank
    arenas = {k: getattr(b, H.ARENA[k]).cpu().numpy() for k in hist.what}
    i = 0
    for kind in hist.what:
        a = arenas[kind]
        for (m, key), (off, shape) in b.index.items():
            v = a[off:off + int(np.prod(shape))]
            mo, s = H.model(v, lim), stats[i]
            assert hist.tags[i] == '%s/%s.%s' % (kind, H.MODULE[m], key)
            assert np.array_equal(counts[i], mo['counts']), hist.tags[i]
            assert (s['num'], s['nonfinite'], s['min'], s['max']) == (mo['num'], mo['nonfinite'], mo['min'], mo['max']), hist.tags[i]
            d = v[np.isfinite(v)].astype(F64)
            assert abs(s['sum'] - mo['sum']) <= _sum_bound(len(d), np.abs(d).sum()), hist.tags[i]
            assert abs(s['sum_squares'] - mo['sum_squares']) <= _sum_bound(len(d), (d * d).sum()), hist.tags[i]
            i += 1
    assert i == hist.n == len(stats)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_twin_trainers_histograms_equal_the_model_and_training_is_unchanged(dataset):
    """Twin A plain, twin B with the histograms of all four arenas armed at every 5th of 11 pipelined steps: bit-identical after every
    step; at a logging step the result equals model() over A's arenas behind the same step -- the updated parameters and moments, the
    step's own gradient.  Steps that are not armed make no call."""
    batches = _batches(dataset, sum(BS), S, STEPS)
    A, B = _trainer(dataset, BS, S), _trainer(dataset, BS, S)
    hist = B.enable_tb_hist(ALL)
    assert hist.n == 4 * len(B.bank.index) and hist.tags[0] == 'weights/encoder.convd1.conv1.weight'
    calls = []
    launch = hist.launch
    hist.launch = lambda stream=None: (calls.append(1), launch(stream))[1]
    with pytest.raises(RuntimeError, match='no armed step'):
        B.take_tb_hist()
    for i in range(STEPS):
        nxt = batches[i + 1] if i + 1 < STEPS else None
        A.step(*batches[i], next_batch=nxt)
        if i % 5 == 0:
            B.arm_tb_hist()
        B.step(*batches[i], next_batch=nxt)
        torch.cuda.synchronize()
        _same_state(A, B, ('step', i))
        assert len(calls) == i // 5 + 1
        if i % 5 == 0:
            pending = B.take_tb_hist()
            stats, counts = pending.raw()
            _expect(A, hist, stats, counts)
            assert int(stats['nonfinite'].sum()) == 0 and (stats['num'] == [e.count for e in hist.arr]).all()
            kinds = np.array(hist.kinds)
            assert (stats['min'][kinds == 'adam_v'] >= 0).all() and stats['sum_squares'][kinds == 'grads'].sum() > 0
    assert len(hist._free) == 1                             # one pinned buffer served all three logging steps


def test_histograms_beside_every_other_user_of_the_hook_and_a_planted_infinity():
    """Fundus, twins C and D under the guard (skip on non-finite), the health ring, the image grids and the weight average, C also
    with the histograms, all armed in the same steps; at step 5 the soft target carries one +inf pixel: the gradient arena holds
    non-finite values (hist_nonfinite/grads), the guard skips, the weights stay finite (no hist_nonfinite/weights)."""
    batches = _batches('fundus', sum(BS), S, STEPS)
    batches[5] = batches[5][:3] + (batches[5][3].clone(),)
    batches[5][3][1, 0, 3, 4] = float('inf')
    twins = []
    for with_hist in (True, False):
        tr = _trainer('fundus', BS, S)
        tr.enable_grad_guard(0.0)
        tr.enable_step_log(health=True, rows=16)
        tr.enable_avg_weights('ema', 0.5, 0)
        twins.append(tr)
    Ct, Dt = twins
    hist = Ct.enable_tb_hist(('weights', 'grads'))
    for i in range(STEPS):
        nxt = batches[i + 1] if i + 1 < STEPS else None
        for tr in twins:
            if i % 5 == 0:
                tr.arm_tb_images()
                if tr is Ct:
                    tr.arm_tb_hist()
            tr.step(*batches[i], next_batch=nxt)
        torch.cuda.synchronize()
        _same_state(Ct, Dt, ('step', i))
        if i % 5 == 0:
            ic, idt = Ct.take_tb_images().images(), Dt.take_tb_images().images()
            assert len(ic) == 7 and all(t == u and np.array_equal(g, h) for (t, g), (u, h) in zip(ic, idt))
            pending = Ct.take_tb_hist()
            stats, counts = pending.raw()
            _expect(Dt, hist, stats, counts)
            histos, scalars = pending.fetch()
            assert [h[0] for h in histos] == hist.tags and all(sum(h[7]) == h[3] and len(h[6]) == len(h[7]) for h in histos)
            if i == 5:
                assert [t for t, _ in scalars] == ['hist_nonfinite/grads'] and scalars[0][1] == int(stats['nonfinite'].sum()) > 0
                assert bool(torch.isfinite(Ct.bank.params).all()) and not bool(torch.isfinite(Ct.bank.grads).all())
            else:
                assert scalars == []
    assert repr(Ct.drain_step_log()) == repr(Dt.drain_step_log())      # (step 5's losses are not finite: compared as text)
    assert torch.equal(Ct._avg.bank.params, Dt._avg.bank.params)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_data_parallel_step_on_one_rank(dataset):
    """ddp.DataParallelStep over one rank runs the same after-step hook: a rank that does not write enqueues without a copy, the
    writing rank's result equals the model over its arenas behind the step, and parameters, moments and BatchNorm buffers equal the
    plain trainer's."""
    from ramdsir import ddp
    batches = _batches(dataset, sum(BS), S, 6)
    A, tr = _trainer(dataset, BS, S), _trainer(dataset, BS, S)
    runner = ddp.DataParallelStep(tr.ts)
    tr.runner, tr._step = runner, runner.step
    hist = tr.enable_tb_hist()
    for i in range(6):
        nxt = batches[i + 1] if i + 1 < 6 else None
        A.step(*batches[i], next_batch=nxt)
        if i in (0, 5):
            tr.arm_tb_hist(copy=i == 5)
        tr.step(*batches[i], next_batch=nxt)
        torch.cuda.synchronize()
        if i == 0:
            with pytest.raises(RuntimeError, match='no armed step'):
                tr.take_tb_hist()
    _same_state(A, tr, 'data parallel, one rank', step_buffers=False)
    _expect(tr, hist, *tr.take_tb_hist().raw())


def test_a_captured_graph_is_refused():
    tr = _trainer('fundus', [1, 1, 1], 32)
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='a captured hipGraph replays a fixed launch list, which has no place for the per-tensor histograms'):
        tr.enable_tb_hist()
    assert tr._hist is None


# ------------------------------------------------------------------------------------------------------------- the CLI
from test_gpu_ckpt import _tree, _train       # noqa: E402


def _records(out):
    """(scalar records, image records, histogram records) of every event file of a run, wall times left out."""
    sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))
    from utils import tfevents
    sc, im, hi = [], [], []
    for f in sorted(os.listdir(os.path.join(out, 'log'))):
        for e in tfevents.read_events(os.path.join(out, 'log', f))[1:]:
            assert len(e['scalars']) + len(e['images']) + len(e['histos']) == 1
            sc += [(e['step'],) + tuple(x) for x in e['scalars']]
            im += [(e['step'],) + tuple(x) for x in e['images']]
            hi += [(e['step'],) + tuple(x) for x in e['histos']]
    return sc, im, hi


def _files(out):
    """final_model.pth, the validation CSV (None where the run's validation wrote none) and the keep-best names."""
    read = lambda n: open(os.path.join(out, n), 'rb').read() if os.path.exists(os.path.join(out, n)) else None      # noqa: E731
    final = read('final_model.pth')
    assert final is not None
    return final, read('0_val_log.csv'), sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, 'model_*.pth')))


def _names(kinds, dataset):
    """The expected tags: the reference's state_dict names of the parameters.  Fundus trains on three domains, the geometry of
    tests/golden/state_manifest.json; the Prostate runs on five, so their restoration decoder has five BatchNorms per DSBN site and
    the names come from the module specs (which the manifest pins for three)."""
    import json
    from ramdsir import engine as E
    def spec_names(domains):
        mods = (('encoder', E.encoder_specs()), ('seg_decoder', E.decoder_specs()), ('rec_decoder', E.rec_decoder_specs(16, 3, domains)))
        return ['%s.%s' % (m, key) for m, specs in mods for key, _, kind, _ in specs if kind == 'param']
    man = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'state_manifest.json')))
    buffers = ('running_mean', 'running_var', 'num_batches_tracked')
    assert spec_names(3) == ['%s.%s' % (m, k) for m in ('encoder', 'seg_decoder', 'rec_decoder') for k, _, _ in man[m] if not k.endswith(buffers)]
    return ['%s/%s' % (kind, nm) for kind in kinds for nm in spec_names(3 if dataset == 'fundus' else 5)]


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_the_flag_adds_histogram_records_and_changes_nothing_else(tmp_path, dataset):
    """--tb_images 4 against --tb_images 4 --tb_hist 2, two epochs: final_model.pth, the CSV and the keep-best names byte-identical,
    scalar and image records equal, the histogram tags x steps exactly the expected set, every record's bucket counts sum to num."""
    data = _tree(tmp_path, dataset)
    plain, on = str(tmp_path / 'plain'), str(tmp_path / 'on')
    code, log0 = _train(data, dataset, plain, ['--tb_images', '4'], epochs=2)
    assert code == 0 and 'tb_hist:' not in log0, log0[-3000:]
    code, log1 = _train(data, dataset, on, ['--tb_images', '4', '--tb_hist', '2'], epochs=2)
    assert code == 0 and 'tb_hist: ' in log1 and 'histogram records at' in log1, log1[-3000:]
    assert _files(plain) == _files(on)
    (sc0, im0, hi0), (sc1, im1, hi1) = _records(plain), _records(on)
    assert hi0 == [] and sc0 == sc1 and im0 == im1 and len(im0) > 0
    iters = 10                                              # both trees: the longest domain list gives five batches per epoch
    assert [(h[0], h[1]) for h in hi1] == [(it, t) for it in range(0, iters, 2) for t in _names(('weights', 'grads'), dataset)]
    for h in hi1:
        step, tag, mn, mx, num, total, sq, limits, counts = h
        assert sum(counts) == num > 0 and len(limits) == len(counts) and mn <= mx and sq >= 0, (step, tag)
        assert list(limits) == sorted(limits) and counts[-1] > 0 and (counts[0] == 0 or limits[0] == H.default_limits()[0])
    assert any(h[2] < 0 < h[3] for h in hi1)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_all_four_kinds_and_a_resumed_run_writes_the_same_histograms(tmp_path, dataset):
    """Four epochs with --ckpt_every 1 --tb_hist 2 over all four arenas against the same run stopped after two epochs and resumed:
    twice the tags of the default, and equal histogram records at equal iterations."""
    data = _tree(tmp_path, dataset)
    flags = ['--ckpt_every', '1', '--tb_hist', '2', '--tb_hist_what', 'weights,grads,adam_m,adam_v']
    whole, cut = str(tmp_path / 'whole'), str(tmp_path / 'cut')
    code, log = _train(data, dataset, whole, flags)
    assert code == 0, log[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--resume', os.path.join(cut, 'last_state.pth')])
    assert code == 0 and 'continuing at epoch 2' in log, log[-3000:]
    (sc_w, _, hi_w), (sc_c, _, hi_c) = _records(whole), _records(cut)
    iters = 20
    tags = _names(H.KINDS, dataset)
    assert len(tags) == 2 * len(_names(('weights', 'grads'), dataset))
    assert [(h[0], h[1]) for h in hi_w] == [(it, t) for it in range(0, iters, 2) for t in tags]
    assert hi_w == hi_c
