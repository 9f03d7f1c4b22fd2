"""-m gpu: train.py --accum_steps -- rd_grad_accum (csrc/accum.hip) against its numpy model (ramdsir/accum.py window) on twin arenas
between sentinels, the fused trainer with enable_grad_accum against a twin driven by hand (pipelined and not, under the guard, the
grouped Adam and the weight average, across a snapshot in mid-window), and the CLI end to end.

Every comparison is an equality on bits, with one exception that is a property of IEEE 754 and not of this code: the payload of a NaN
that an ADDITION produces or passes on is the platform's (inf + -inf is 0x7FC00000 on the GPU and 0xFFC00000 in numpy on x86), so
where the model's sum is a NaN the kernel's must be a NaN, and every other word must have the model's bits.  The copy of a window's
first micro-batch is compared on bits throughout, NaN payloads included."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, accum as A, ckpt as CK, optim as O       # noqa: E402
from test_gpu_avg_weights import _batches, _bits, _models, _read, _same_checkpoint, _train, _trainer, _tree       # noqa: E402
from test_gpu_ckpt import _assert_same_run, _outputs        # noqa: E402
from test_gpu_grad_guard import _same_snap, _snap           # noqa: E402

F32 = np.float32
GAPW = 1024                                                 # 4 KiB of sentinel words in front of and behind every arena
SENT = 0xA5A5A5A5


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fbits(x):
    return int(np.asarray(x, F32).view(np.int32))


class Twin:
    """The gradient arena and the accumulator arena of n words, each in a buffer of its own, `ga` / `aa` words behind a 16-byte
    boundary, with 4 KiB of sentinel on either side."""

    def __init__(self, n, ga, aa):
        self.n, self.lo = n, (GAPW + ga, GAPW + aa)
        self.bufs = [torch.from_numpy(np.full(GAPW + 4 + n + GAPW, SENT, np.uint32).view(np.int32)).to(DEV) for _ in range(2)]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        self.ptr = [b.data_ptr() + 4 * lo for b, lo in zip(self.bufs, self.lo)]

    def put(self, which, words):
        lo = self.lo[which]
        self.bufs[which][lo:lo + self.n].copy_(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)))

    def get(self, which):
        """(the arena's words, whether every sentinel word is intact) -- synchronises."""
        host = self.bufs[which].cpu().numpy().view(np.uint32)
        lo = self.lo[which]
        return host[lo:lo + self.n].copy(), bool((host[:lo] == SENT).all() and (host[lo + self.n:] == SENT).all())

    def launch(self, k, steps, inv=None):
        return A.run(self.ptr[0], self.ptr[1], self.n, k, steps, A.inv_steps(steps) if inv is None else inv)


def _same_words(got, want, what, sums):
    """Bits; where `sums` (the words come out of an addition) a NaN of the model is matched by any NaN."""
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    ok = got == want
    if sums:
        ok |= np.isnan(got.view(F32)) & np.isnan(want.view(F32))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (what, 'first differing word', int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), 'of', bad.size)


def _grads(rng, n, plant):
    """Random float32 words of many magnitudes, denormals and both zeros among them; plant: NaN (two payloads) and both infinities."""
    x = (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(F32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1.1754942e-38], F32)
    idx = rng.randint(0, n, max(n // 9, 1))
    x[idx] = special[rng.randint(0, special.size, idx.size)]
    if plant:
        w = x.view(np.uint32)
        for pos, bits in zip(rng.randint(0, n, 4), (0x7FC00000, 0x7FA00001, 0x7F800000, 0xFF800000)):
            w[pos] = bits
    return x


def _walk_windows(tw, steps, rng, windows, what):
    """`windows` consecutive windows of `steps` launches: behind every launch both arenas against window(), the side that must not be
    written against its bits from before, and every sentinel."""
    n = tw.n
    acc_before = tw.get(1)[0]
    for w in range(windows):
        grads = [_grads(rng, n, plant=(w == 1 or n < 8)) for _ in range(steps)]
        states = A.window(grads)
        for k in range(steps):
            tw.put(0, grads[k])
            assert tw.launch(k, steps) == 0
            g, g_ok = tw.get(0)
            a, a_ok = tw.get(1)
            assert g_ok and a_ok, (what, w, k, 'a sentinel was written')
            if k < steps - 1:
                _same_words(g, grads[k], (what, w, k, 'grad must be untouched'), sums=False)
                _same_words(a, states[k], (what, w, k, 'acc'), sums=k > 0)
            else:
                _same_words(a, acc_before, (what, w, k, 'acc must be untouched'), sums=False)
                _same_words(g, states[k], (what, w, k, 'the mean in the gradient arena'), sums=True)
            acc_before = a


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('n', [1, 3, 4, 255, 1025, 70001])
def test_kernel_equals_the_model_over_every_position_of_two_windows(n):
    """n x the 4 x 4 alignments of grad and acc (the 16-byte path with its head and tail words where the two share a phase, the
    word path elsewhere) x N in {2, 3, 5}; the second window carries planted NaN (a quiet and a signalling payload) and both
    infinities (every window, for n < 8)."""
    for ga in range(4):
        for aa in range(4):
            for steps in (2, 3, 5):
                tw = Twin(n, ga, aa)
                tw.put(1, _grads(np.random.RandomState(7), n, False))      # what a previous window left: overwritten by the copy
                _walk_windows(tw, steps, np.random.RandomState(1000 * n + 100 * ga + 10 * aa + steps), 2, (n, ga, aa, steps))


@pytest.mark.parametrize('n,ga,aa', [(1024 * 4096 + 4103, 1, 1), (1024 * 1024 + 5, 0, 3)])
def test_kernel_past_the_grid_cap(n, ga, aa):
    """The grid is capped at 1024 workgroups: past 1024 x 4096 words on the 16-byte path and 1024 x 1024 on the word path a thread
    makes a second trip of its grid-stride loop (a size the issue's list does not reach)."""
    _walk_windows(Twin(n, ga, aa), 3, np.random.RandomState(n % 1000), 1, (n, ga, aa))


def test_one_step_windows_launch_nothing_and_refusals_touch_nothing():
    n = 1025
    tw = Twin(n, 1, 2)
    rng = np.random.RandomState(3)
    g, a = _grads(rng, n, True), _grads(rng, n, True)
    tw.put(0, g)
    tw.put(1, a)
    assert tw.launch(0, 1) == 0                                 # steps == 1: the gradient is its own mean
    assert tw.launch(0, 3, inv=0.3) == -6 and tw.launch(3, 3) == -5 and tw.launch(0, 0, inv=1.0) == -4
    assert A.run(tw.ptr[0], tw.ptr[0] + 8, n, 0, 2, 0.5) == -7 and A.run(tw.ptr[0] + 2, tw.ptr[1], n, 0, 2, 0.5) == -2
    assert A.run(None, tw.ptr[1], n, 0, 2, 0.5) == -1 and A.run(tw.ptr[0], tw.ptr[1], 0, 0, 2, 0.5) == -3
    for which, want in ((0, g), (1, a)):
        got, ok = tw.get(which)
        assert ok
        _same_words(got, want, ('untouched', which), sums=False)


# ------------------------------------------------------------------------------------------------------------- the trainer
BS, S, STEPS = [2, 3, 3], 32, 11
_HAND = {}


def _snap_h(tr):
    s = _snap(tr)
    s['hyper'] = tr.ts.hyper.clone()
    return s


def _same_h(a, b, what):
    _same_snap(a, b, what)
    assert torch.equal(_bits(a['hyper']), _bits(b['hyper'])), (what, 'hyper')


def _hand_run(dataset, steps):
    """(a), once per (dataset, N): a trainer with enable_grad_accum(N) over 11 NON-pipelined steps in lockstep with a twin driven by
    hand -- the twin runs ts.launch(head + backward), reads the gradient back, and at the window's last micro-batch puts model()'s
    mean into the arena and runs rd_adam_step + the repack.  Parameters, both moments, every BatchNorm buffer, the counter, the loss
    words and hyper are equal after every step.  Returns the per-step snapshots."""
    key = (dataset, steps)
    if key not in _HAND:
        batches = _batches(dataset, sum(BS), S, STEPS)
        tr, twin = _trainer(dataset, BS, S), _trainer(dataset, BS, S)
        acc = tr.enable_grad_accum(steps)
        assert tr._accum is acc and tr.ts._accum is acc and twin.ts._accum is None and acc.steps == steps
        ts, lib, window, snaps = twin.ts, L.lib(), [], []
        for i in range(STEPS):
            assert acc.next_is_boundary() == ((i + 1) % steps == 0) and acc.position() == i % steps
            tr.step(*batches[i])
            ts.load_raw(*batches[i][:3])
            ts.load_target(batches[i][3])
            ts.launch(ts.head_names() + ts.backward_names(), join=True)
            ts.advance()
            torch.cuda.synchronize()
            window.append(twin.bank.grads.cpu().numpy().copy())
            if len(window) == steps:
                mean = acc.model(window)
                assert np.isfinite(mean).all() and np.abs(mean).max() > 0
                twin.bank.grads.copy_(torch.from_numpy(mean))
                L.check(lib.rd_adam_step(C.byref(ts.ad), _st()), 'rd_adam_step')
                ts.wpack.refresh(_st())
                window = []
                torch.cuda.synchronize()
                assert torch.equal(_bits(tr.bank.grads), _bits(twin.bank.grads)), (i, 'the mean in the gradient arena')
            snaps.append(_snap_h(tr))
            _same_h(snaps[-1], _snap_h(twin), (dataset, steps, 'step', i))
            assert snaps[-1]['iter'] == (i + 1) // steps        # the counter counts updates
        assert torch.equal(tr.ts.wpack.packed, twin.ts.wpack.packed)
        nbt = [k for k in tr.bank.buffers if k[1].endswith('num_batches_tracked')]
        # BatchNorm moves at every iteration (the shared encoder / decoder BatchNorms see two passes per step, as in the reference)
        assert nbt and all(int(tr.bank.buffers[k]) in (STEPS, 2 * STEPS) for k in nbt)
        _HAND[key] = snaps
    return _HAND[key]


@pytest.mark.parametrize('steps', [2, 3])
@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_accumulating_trainer_equals_the_twin_driven_by_hand(dataset, steps):
    snaps = _hand_run(dataset, steps)
    assert len(snaps) == STEPS and snaps[-1]['iter'] == STEPS // steps
    # between two updates parameters and moments stand still; an update moves them
    for i in range(1, STEPS):
        moved = not torch.equal(snaps[i]['params'], snaps[i - 1]['params'])
        assert moved == ((i + 1) % steps == 0), i


@pytest.mark.parametrize('steps', [2, 3])
@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_pipelined_accumulation_equals_the_classical_one(dataset, steps):
    """(b) the same trainer with next_batch (the next batch's RAM beside the encoder backward, the input slots flipping) equals (a)
    after every step."""
    want = _hand_run(dataset, steps)
    batches = _batches(dataset, sum(BS), S, STEPS)
    tr = _trainer(dataset, BS, S)
    tr.enable_grad_accum(steps)
    for i in range(STEPS):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        torch.cuda.synchronize()
        _same_h(_snap_h(tr), want[i], (dataset, steps, 'pipelined step', i))


def test_a_repeated_batch_over_a_window_of_two_is_one_plain_step():
    """(c) (g + g) * 0.5 == g exactly: parameters and moments behind the window equal ONE plain step on that batch; the running
    statistics have moved twice."""
    batch = _batches('fundus', sum(BS), S, 1)[0]
    plain, tr = _trainer('fundus', BS, S), _trainer('fundus', BS, S)
    tr.enable_grad_accum(2)
    plain.step(*batch)
    tr.step(*batch)
    tr.step(*batch)
    torch.cuda.synchronize()
    a, b = _snap_h(tr), _snap_h(plain)
    for name in ('params', 'exp_avg', 'exp_avg_sq', 'hyper', 'losses', 'rec_mse'):
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    assert a['iter'] == b['iter'] == 1 and torch.equal(_bits(tr.bank.grads), _bits(plain.bank.grads))
    nbt = [k for k in tr.bank.buffers if k[1].endswith('num_batches_tracked')]
    assert nbt and all(int(tr.bank.buffers[k]) == 2 * int(plain.bank.buffers[k]) > 0 for k in nbt)
    rm = [k for k in tr.bank.buffers if k[1].endswith('running_mean')]
    assert any(not torch.equal(tr.bank.buffers[k], plain.bank.buffers[k]) for k in rm)


def test_a_nonfinite_micro_batch_makes_the_guard_skip_the_whole_window():
    """(d) N = 2 under enable_grad_guard: a +inf target pixel in the FIRST micro-batch of the third window (step 4) -- the verdict is
    the mean gradient's, so parameters, moments and every BatchNorm buffer behind step 5 are those from before step 4 (the roll-back
    covers both forward passes); the state word's steps count windows.  The unguarded twin ends the window non-finite."""
    batches = _batches('fundus', sum(BS), S, 8)
    batches[4] = batches[4][:3] + (batches[4][3].clone(),)
    batches[4][3][1, 0, 3, 4] = float('inf')
    for guarded in (True, False):
        tr = _trainer('fundus', BS, S)
        gd = tr.enable_grad_guard(0.0) if guarded else None
        tr.enable_grad_accum(2)
        for i in range(8):
            if i == 4:
                torch.cuda.synchronize()
                before = _snap(tr)
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < 8 else None)
            if i == 4 and guarded:
                torch.cuda.synchronize()
                assert gd.read()['steps'] == 2                  # no verdict in mid-window
                assert any(not torch.equal(tr.bank.buffers[k], v) for k, v in before['buffers'].items())      # the statistics moved
                assert all(torch.equal(_bits(gd.shadows[k]), _bits(v)) for k, v in before['buffers'].items())
            if i == 5:
                torch.cuda.synchronize()
                after = _snap(tr)
                assert not bool(torch.isfinite(tr.bank.grads).all())
                if not guarded:
                    assert not bool(torch.isfinite(after['params']).all())
                    break
                w = gd.read()
                assert (w['skip'], w['skipped'], w['steps'], w['clipped']) == (1, 1, 3, 0) and w['nonfinite'] > 0, w
                for name in ('params', 'exp_avg', 'exp_avg_sq'):
                    assert torch.equal(_bits(after[name]), _bits(before[name])), name
                for k in before['buffers']:
                    assert torch.equal(_bits(after['buffers'][k]), _bits(before['buffers'][k])), k
                assert after['iter'] == before['iter'] + 1 == 3
        torch.cuda.synchronize()
        if guarded:
            end, w = _snap(tr), gd.read()
            assert (w['steps'], w['skipped'], w['skip']) == (4, 1, 0) and end['iter'] == 4
            assert all(bool(torch.isfinite(end[n]).all()) for n in ('params', 'exp_avg', 'exp_avg_sq'))
            assert not torch.equal(end['params'], after['params'])


@pytest.mark.parametrize('accum_first', [True, False])
def test_accumulation_with_grouped_adam_guard_and_averaging_together(accum_first):
    """(e) one trainer with all four (the grouped Adam at its default values and an open guard leave the bits of the plain tail):
    the state equals (a)'s after every step, and the average moves at the window's last step only, where it is avg.model replayed
    over the read-back parameters at the counter's value -- the number of updates."""
    want = _hand_run('fundus', 2)
    batches = _batches('fundus', sum(BS), S, STEPS)
    tr = _trainer('fundus', BS, S)
    if accum_first:
        tr.enable_grad_accum(2)
    tr.enable_optim()
    gd = tr.enable_grad_guard(1e30)
    wa = tr.enable_avg_weights('ema', 0.5, 0)
    if not accum_first:
        tr.enable_grad_accum(2)
    avg_p = tr.bank.params.cpu().numpy().copy()
    for i in range(STEPS):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        torch.cuda.synchronize()
        _same_h(_snap_h(tr), want[i], ('all four', i))
        if (i + 1) % 2 == 0:
            avg_p = wa.model(avg_p, tr.bank.params.cpu().numpy(), int(tr.ts.iter))
        got = wa.bank.params.cpu().numpy()
        assert np.array_equal(got.view(np.int32), avg_p.view(np.int32)), ('avg', i)
    w = gd.read()
    assert (w['steps'], w['skipped'], w['clipped']) == (STEPS // 2, 0, 0)
    assert not torch.equal(wa.bank.params, tr.bank.params)


def test_a_snapshot_in_mid_window_continues_bit_for_bit(tmp_path):
    """(f) N = 2: a snapshot behind step 5 (one micro-batch of the third window accumulated), restored into a freshly initialised
    trainer with other weights, continued: equal to the uninterrupted run of (a) after every step."""
    want = _hand_run('fundus', 2)
    batches = _batches('fundus', sum(BS), S, STEPS)
    tr = _trainer('fundus', BS, S)
    acc = tr.enable_grad_accum(2)
    for i in range(5):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < 5 else None)
    assert acc.position() == 1
    sb = CK.TrainState(tr, extra=acc.named_ranges())
    assert sb.table[-1]['name'] == 'accum/arena'
    path = str(tmp_path / 'last_state.pth')
    sb.snapshot(path, dict(epoch=0, iter_num=5, grad_accum=dict(acc.settings(), micro=acc.position())))
    sb.close()
    state = CK.load_file(path)
    assert state['meta']['grad_accum'] == dict(steps=2, micro=1)
    fresh = _trainer('fundus', BS, S, seed=99)
    acc2 = fresh.enable_grad_accum(2)
    with pytest.raises(ValueError, match='grad_accum steps = 2, this run has 3'):
        CK.compare_grad_accum(state, dict(steps=3))
    sc = CK.TrainState(fresh, extra=acc2.named_ranges())
    sc.restore(state)
    acc2.set_position(CK.compare_grad_accum(state, acc2.settings()))
    sc.close()
    assert torch.equal(_bits(acc2.acc), _bits(acc.acc)) and bool(acc2.acc.any())
    for i in range(5, STEPS):
        fresh.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        torch.cuda.synchronize()
        _same_h(_snap_h(fresh), want[i], ('restored', i))


def test_captured_graphs_and_bad_step_counts_are_refused():
    """(g)"""
    tr = _trainer('fundus', [1, 1, 1], 32)
    for bad in (0, -1, 65537):
        with pytest.raises(ValueError, match='grad accum: steps'):
            tr.enable_grad_accum(bad)
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_grad_accum(2)
    tr._graphs = False
    tr.ts.graph = object()                                  # (what capture() leaves)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_grad_accum(2)
    tr.ts.graph = None
    tr.world = 2
    with pytest.raises(RuntimeError, match='one process'):
        tr.enable_grad_accum(2)
    tr.world = 1
    assert tr._accum is None and tr.ts._accum is None
    assert tr.enable_grad_accum(1) is None and tr.ts._accum is None       # N = 1: nothing is constructed
    acc = tr.enable_grad_accum(2)
    with pytest.raises(RuntimeError, match='gradient accumulation'):
        tr.ts.capture()
    assert tr.ts._accum is acc


# ------------------------------------------------------------------------------------------------------------- the CLI
EVERY = ['--log_every', '1', '--lr', '0.001']


def _lr_records(out):
    return [(s, v) for s, t, v in _outputs(out, None)['scalars'] if t == 'lr']


def _summary(log):
    m = re.search(r'accum: (\d+) micro-batches per update: (\d+) updates over (\d+) iterations, (\d+) trailing iterations? (?:is|are) not applied', log)
    assert m, log[-3000:]
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_one_spelled_out_and_the_schedule_of_two(tmp_path, dataset):
    """--accum_steps 1 spelled out against no flag: final_model.pth bytes, CSV, keep-best names, scalar records.  --accum_steps 2
    (with --lr_schedule cosine: under poly the first two updates share a rate): the lr records -- the last update's rate at every
    iteration, 0 before the first -- show iterations // 2 distinct schedule values, schedule_model's over the UPDATES; the summary
    line."""
    data = _tree(tmp_path, dataset)
    plain, one, two = (str(tmp_path / n) for n in ('plain', 'one', 'two'))
    iters = 10 if dataset == 'fundus' else 6
    code, log0 = _train(data, dataset, plain, EVERY, epochs=2)
    assert code == 0 and 'accum:' not in log0, log0[-3000:]
    code, log1 = _train(data, dataset, one, EVERY + ['--accum_steps', '1'], epochs=2)
    assert code == 0 and 'accum:' not in log1, log1[-3000:]
    assert _read(one, 'final_model.pth') == _read(plain, 'final_model.pth') is not None
    assert _read(one, '0_val_log.csv') == _read(plain, '0_val_log.csv') is not None
    assert _models(one, 'model_') == _models(plain, 'model_') and len(_models(plain, 'model_')) == 1
    _assert_same_run(_outputs(plain, dataset), _outputs(one, dataset), '--accum_steps 1 spelled out')
    code, log2 = _train(data, dataset, two, EVERY + ['--accum_steps', '2', '--lr_schedule', 'cosine'], epochs=2)
    assert code == 0, log2[-3000:]
    assert _summary(log2) == (2, iters // 2, iters, 0)
    lr = _lr_records(two)
    assert [s for s, _ in lr] == list(range(iters)) and lr[0][1] == 0.0
    for s, v in lr[1:]:                                     # iteration s follows update (s + 1) // 2 - 1
        assert abs(_fbits(v) - _fbits(O.schedule_model((s + 1) // 2 - 1, 1e-3, iters // 2, 'cosine'))) <= 1, (s, v)
    assert len({_fbits(v) for _, v in lr[1:]}) == iters // 2
    assert _read(two, 'final_model.pth') != _read(plain, 'final_model.pth')


def test_train_cli_three_on_fundus_names_its_trailing_iterations(tmp_path):
    data = _tree(tmp_path, 'fundus')
    code, log = _train(data, 'fundus', str(tmp_path / 'three'), EVERY + ['--accum_steps', '3'])
    assert code == 0, log[-3000:]
    assert _summary(log) == (3, 6, 20, 2) and '2 trailing iterations are not applied' in log
    assert len(_lr_records(str(tmp_path / 'three'))) == 20   # the loop counts iterations
    code, log = _train(data, 'fundus', str(tmp_path / 'none'), ['--accum_steps', '30'])
    assert code != 0 and '--accum_steps 30: the 20 iterations of this run complete no window' in log, log[-3000:]


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_a_resumed_accumulating_run_ends_in_the_same_model(tmp_path, dataset):
    """4 epochs with --accum_steps 2 --ckpt_every 1 against the same run stopped after 2 epochs and resumed.  The epochs are 5
    (Fundus) and 3 (Prostate) iterations long, so windows straddle epoch boundaries and snapshots are taken in mid-window: equal
    final_model.pth, CSV, keep-best names and scalar records.  Fundus: a resume under another N, or without the flag, is refused by
    name."""
    data = _tree(tmp_path, dataset)
    flags = ['--accum_steps', '2', '--ckpt_every', '1']
    whole, cut = str(tmp_path / 'whole'), str(tmp_path / 'cut')
    code, log_whole = _train(data, dataset, whole, flags)
    assert code == 0 and 'ckpt: 4 snapshots' in log_whole, log_whole[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    state = os.path.join(cut, 'last_state.pth')
    mid = CK.load_file(state)
    iters = 10 if dataset == 'fundus' else 6
    assert mid['meta']['grad_accum'] == dict(steps=2, micro=0) and mid['meta']['iter_num'] == iters
    assert [e['name'] for e in mid['table']][-1] == 'accum/arena' and int(CK.range_tensor(mid, 'iter')) == iters // 2
    if dataset == 'fundus':
        code, log = _train(data, dataset, cut, ['--accum_steps', '4', '--ckpt_every', '1', '--resume', state])
        assert code != 0 and 'grad_accum steps = 2, this run has 4' in log, log[-3000:]
        code, log = _train(data, dataset, cut, ['--ckpt_every', '1', '--resume', state])
        assert code != 0 and 'grad_accum steps = 2, this run has 1' in log, log[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--resume', state])
    assert code == 0 and 'continuing at epoch 2' in log, log[-3000:]
    assert _read(cut, '0_val_log.csv') == _read(whole, '0_val_log.csv') is not None
    assert _models(cut, 'model_') == _models(whole, 'model_')
    _same_checkpoint(torch.load(os.path.join(cut, 'final_model.pth'), map_location='cpu'),
                     torch.load(os.path.join(whole, 'final_model.pth'), map_location='cpu'), 'final_model.pth')
    _assert_same_run(_outputs(whole, dataset), _outputs(cut, dataset), 'stopped after two epochs and resumed')
    if dataset == 'fundus':
        # two epochs are 10 iterations, a whole number of windows; ONE epoch is 5: the snapshot holds a half-filled accumulator
        odd = str(tmp_path / 'odd')
        code, log = _train(data, dataset, odd, flags + ['--stop_after_epochs', '1'])
        assert code == 0 and 'Stopped after 1 epochs' in log, log[-3000:]
        state = os.path.join(odd, 'last_state.pth')
        mid = CK.load_file(state)
        assert mid['meta']['grad_accum'] == dict(steps=2, micro=1) and int(CK.range_tensor(mid, 'iter')) == 2
        assert bool(CK.range_tensor(mid, 'accum/arena').any())
        code, log = _train(data, dataset, odd, flags + ['--resume', state])
        assert code == 0 and 'continuing at epoch 1' in log, log[-3000:]
        _assert_same_run(_outputs(whole, dataset), _outputs(odd, dataset), 'stopped in mid-window and resumed')
