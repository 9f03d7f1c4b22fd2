"""-m gpu: train.py --clip_grad_norm / --skip_nonfinite -- rd_grad_guard (csrc/guard.hip) against its numpy model (ramdsir/guard.py
model), rd_adam_step_guarded against rd_adam_step on twin arenas, rd_guard_sync as a byte copy in the direction the device flag
selects, the fused trainer under the guard (identical when nothing is clipped, the model's scale when something is, no trace of a
non-finite step), the data-parallel step on one rank, and the CLI end to end.

Every comparison is an equality: the model restates the kernel's summation order (ramdsir/sumsq.py), so on random normal data, too,
the kernel's norm is the model's bit for bit (the ulp figure is printed: 0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, ckpt as CK, guard as G       # noqa: E402
from test_gpu_avg_weights import _batches, _bits, _models, _read, _same_checkpoint, _train, _trainer, _tree       # noqa: E402

F32 = np.float32
GAP, SENT = 4096, 0xA5
CHUNK = L.LOG_CHUNK


def _st():
    return torch.cuda.current_stream().cuda_stream


def _state_bytes(**kw):
    s = L.RdGuardState()
    for k, v in kw.items():
        setattr(s, k, v)
    return bytes(s)


def _state_tensor(**kw):
    return torch.from_numpy(np.frombuffer(_state_bytes(**kw), np.int64).copy()).to(DEV)


def _fbits(x):
    return int(np.asarray(x, F32).view(np.int32))


# ------------------------------------------------------------------------------------------------------------- rd_grad_guard
class GuardRig:
    """One device buffer: sentinel | workspace of exactly rd_grad_guard_workspace(n) bytes | sentinel | the 40-byte state word |
    sentinel; and a gradient of n floats that starts `align` words behind a 16-byte boundary."""

    def __init__(self, n, align):
        self.n, self.align = n, align
        self.ws_bytes = L.lib().rd_grad_guard_workspace(n)
        assert self.ws_bytes == G.workspace_bytes(n) == -(-n // CHUNK) * 16
        self.ws_off = GAP
        self.st_off = GAP + self.ws_bytes + GAP
        self.size = self.st_off + G.STATE_BYTES + GAP
        self.host = np.full(self.size, SENT, np.uint8)
        self.host[self.st_off:self.st_off + G.STATE_BYTES] = 0
        self.buf = torch.from_numpy(self.host).to(DEV)
        self.gbuf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0 and self.gbuf.data_ptr() % 16 == 0
        self.grad = self.gbuf[align:align + n]
        d = self.desc = L.RdGradGuard()
        d.grad, d.n, d.workspace, d.state = self.grad.data_ptr(), n, self.buf.data_ptr() + self.ws_off, self.buf.data_ptr() + self.st_off

    def run(self, g, max_norm, state=None):
        """Upload g, write the state word (default: zero), call; returns (code, the state word as a dict, the raw bytes of the buffer)."""
        self.grad.copy_(torch.from_numpy(np.ascontiguousarray(g, F32)))
        word = np.frombuffer(_state_bytes(**(state or {})), np.uint8)
        self.buf[self.st_off:self.st_off + G.STATE_BYTES] = torch.from_numpy(word.copy()).to(DEV)
        self.desc.max_norm = max_norm
        code = G.run_guard(self.desc)
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        for a, b in ((0, self.ws_off), (self.ws_off + self.ws_bytes, self.st_off), (self.st_off + G.STATE_BYTES, self.size)):
            assert (raw[a:b] == SENT).all(), ('sentinel written', a, b)
        assert np.array_equal(self.grad.cpu().numpy().view(np.int32), np.ascontiguousarray(g, F32).view(np.int32)), 'the gradient was written'
        return code, G.state_dict_of(raw[self.st_off:self.st_off + G.STATE_BYTES]), raw


def _same_word(got, want, what):
    assert {k: (_fbits(v) if k in ('norm', 'scale') else v) for k, v in got.items()} == \
        {k: (_fbits(v) if k in ('norm', 'scale') else v) for k, v in want.items()}, (what, got, want)


SIZES = [1, 3, 4095, 4096, 4097, 64 * 4096 + 5, 600 * 4096 + 1]


@pytest.mark.parametrize('n', SIZES)
def test_grad_guard_equals_the_model(n):
    """Seven sizes (one element, a head-only chunk, a chunk less one, one chunk, one chunk and one element, the second trip of lane 0's
    fold, 601 chunks) x the four 4-byte alignments of the gradient.  Integer-valued data: every sum is exact -- the state word equals
    the model's bit for bit, with and without clipping.  Random normal data: the norm equal to the model's, the scale the one
    the model forms from the device's norm.  Repeat calls leave the same bits in workspace and state."""
    rng = np.random.RandomState(n % 1000)
    worst = 0
    for align in range(4):
        rig = GuardRig(n, align)
        g = rng.randint(-8, 9, n).astype(F32)
        prev = dict(steps=7, clipped=2, skipped=1)
        for max_norm in (0.0, 1.0, 1e30):
            code, got, raw = rig.run(g, max_norm, prev)
            assert code == 0
            _same_word(got, G.model(g, max_norm, prev, align_words=align), (n, align, max_norm))
            assert got['skip'] == 0 and got['steps'] == 8 and got['skipped'] == 1
        code, again, raw2 = rig.run(g, 1e30, prev)
        assert code == 0 and np.array_equal(raw, raw2), 'a repeat call left other bits'
        x = (rng.randn(n) * 10.0 ** rng.uniform(-3, 2)).astype(F32)
        max_norm = float(np.sqrt(n)) * 0.1
        code, got, raw = rig.run(x, max_norm)
        want = G.model(x, max_norm, align_words=align)
        ulps = abs(_fbits(got['norm']) - _fbits(want['norm']))
        worst = max(worst, ulps)
        assert code == 0 and ulps == 0, (n, align, got, want)
        assert _fbits(got['scale']) == _fbits(G.scale_of(got['norm'], max_norm)) and got['skip'] == 0 and got['nonfinite'] == 0
        assert (got['steps'], got['clipped'], got['skipped']) == (1, int(got['scale'] < 1), 0)
        _, again, raw2 = rig.run(x, max_norm)
        assert np.array_equal(raw, raw2), 'a repeat call left other bits'
    print('n = %d: the kernel\'s norm on random normal data is within %d ulp of the model\'s' % (n, worst))


@pytest.mark.parametrize('n', [4097, 64 * 4096 + 5])
def test_grad_guard_counts_planted_nonfinite_values(n):
    """A NaN or an infinity at index 0, at n - 1 and on each side of a chunk boundary: skip, the exact count, scale 1, the norm of the
    finite elements, the counters."""
    rng = np.random.RandomState(n % 997)
    places = [[0], [n - 1], [CHUNK - 1], [CHUNK], [0, n - 1, CHUNK - 1, CHUNK]]
    for align in range(4):
        rig = GuardRig(n, align)
        for k, idx in enumerate(places):
            g = rng.randint(-8, 9, n).astype(F32)
            g[idx] = [(np.nan, np.inf, -np.inf)[(k + j) % 3] for j in range(len(idx))]
            prev = dict(steps=3, clipped=1, skipped=k)
            code, got, _ = rig.run(g, 0.5, prev)
            want = G.model(g, 0.5, prev, align_words=align)
            assert code == 0
            _same_word(got, want, (n, align, idx))
            assert (got['skip'], got['nonfinite'], got['scale'], got['steps'], got['clipped'], got['skipped']) == (1, len(set(idx)), 1.0, 4, 1, k + 1)       # (n = 4097: n - 1 is the chunk boundary itself)
    # finite elements whose norm is not finite as a float: skipped with a count of zero
    rig = GuardRig(5, 1)
    code, got, _ = rig.run(np.full(5, 3e38, F32), 1.0)
    assert code == 0 and got == dict(norm=float('inf'), scale=1.0, skip=1, nonfinite=0, steps=1, clipped=0, skipped=1)
    # squares that overflow a float but not a double: a finite norm, clipped
    code, got, _ = rig.run(np.array([1e30, -1e30, 1e30, 1e30, 0], F32), 1.0)
    assert code == 0
    _same_word(got, G.model(np.array([1e30, -1e30, 1e30, 1e30, 0], F32), 1.0, align_words=1), 'large squares')
    assert got['norm'] == float(F32(2) * F32(1e30)) and got['skip'] == 0 and got['clipped'] == 1


def test_grad_guard_validation_codes():
    """Every documented code comes back before anything is launched: the state word keeps its bytes."""
    rig = GuardRig(5000, 0)
    lib = L.lib()
    code, before, raw = rig.run(np.ones(5000, F32), 0.0)
    assert code == 0 and before['steps'] == 1

    def call(**edit):
        d = L.RdGradGuard.from_buffer_copy(rig.desc)
        d.max_norm = 1.0
        for k, v in edit.items():
            setattr(d, k, v)
        return lib.rd_grad_guard(C.byref(d), _st())
    assert lib.rd_grad_guard(None, _st()) == -1
    assert call(grad=None) == -1 and call(workspace=None) == -1 and call(state=None) == -1
    assert call(grad=rig.desc.grad + 2) == -1 and call(workspace=rig.desc.workspace + 4) == -1 and call(state=rig.desc.state + 4) == -1
    assert call(n=0) == -2 and call(n=-5) == -2 and call(n=(1 << 24) + 1) == -2
    assert call(max_norm=-1.0) == -3 and call(max_norm=float('nan')) == -3 and call(max_norm=float('inf')) == -3
    torch.cuda.synchronize()
    assert np.array_equal(rig.buf.cpu().numpy(), raw)
    assert call() == 0 and call(n=1) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- rd_adam_step_guarded
B1, B2, ADAM_EPS, BASE_LR, TOTAL = 0.9, 0.999, 1e-8, 2e-3, 50


class AdamTwin:
    """One Adam arena: parameters, moments, counter and hyper words of its own."""

    def __init__(self, p0, n_half):
        n = p0.numel()
        self.p, self.m, self.v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.g = torch.zeros(n, device=DEV)
        self.it = torch.zeros((), dtype=torch.int32, device=DEV)
        self.hyper = torch.zeros(4, device=DEV)
        a = self.a = L.RdAdam()
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.n_half_lr = self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, n_half
        a.iter, a.hyper_out, a.base_lr, a.total_iters = self.it.data_ptr(), self.hyper.data_ptr(), BASE_LR, TOTAL
        a.beta1, a.beta2, a.eps = B1, B2, ADAM_EPS

    def plain(self, g):
        self.g.copy_(g)
        L.check(L.lib().rd_adam_step(C.byref(self.a), _st()), 'rd_adam_step')

    def guarded(self, g, state):
        self.g.copy_(g)
        L.check(L.lib().rd_adam_step_guarded(C.byref(self.a), state.data_ptr(), _st()), 'rd_adam_step_guarded')

    def same(self, other, what):
        torch.cuda.synchronize()
        for name in ('p', 'm', 'v', 'hyper'):
            assert torch.equal(getattr(self, name).view(torch.int32), getattr(other, name).view(torch.int32)), (what, name)
        assert int(self.it) == int(other.it), what


@pytest.mark.parametrize('n,n_half', [(1000, 333), (1048869, 500001)])
def test_guarded_adam_against_the_plain_step_on_twin_arenas(n, n_half):
    """n = 1000 and 1,048,869 (past the 4096-block cap, a ragged tail), the half-lr boundary off every block boundary."""
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen).to(DEV) * (10.0 ** k) for k in (-2, 0, 1)]
    # scale 1: three steps, bit-identical
    a, b = AdamTwin(p0, n_half), AdamTwin(p0, n_half)
    one = _state_tensor(scale=1.0)
    for k, g in enumerate(grads):
        a.plain(g)
        b.guarded(g, one)
        a.same(b, ('scale 1, step', k))
    assert int(b.it) == 3 and not torch.equal(b.p.cpu(), p0)
    # scale 0.37: the plain step fed float32(g * 0.37)
    a, b = AdamTwin(p0, n_half), AdamTwin(p0, n_half)
    s37 = _state_tensor(scale=0.37)
    for k, g in enumerate(grads):
        a.plain(g * torch.tensor(0.37, dtype=torch.float32, device=DEV))
        b.guarded(g, s37)
        torch.cuda.synchronize()
        assert torch.equal(b.g, g)                           # the gradient itself is only read
        a.same(b, ('scale 0.37, step', k))
    # skip: nothing stored, the counter advances, lr and iteration words are the plain call's at the same counter
    skip = _state_tensor(scale=1.0, skip=1, skipped=1)
    keep = [t.clone() for t in (b.p, b.m, b.v)]
    a.plain(grads[0])                                       # the twin moves on: counter 3 -> 4
    b.guarded(torch.full((n,), float('nan')), skip)
    torch.cuda.synchronize()
    for t, k in zip((b.p, b.m, b.v), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    assert int(b.it) == int(a.it) == 4
    assert _fbits(b.hyper[0].cpu()) == _fbits(a.hyper[0].cpu()) and float(b.hyper[3]) == float(a.hyper[3]) == 3.0
    # skipped = 2: the bias corrections of a plain call whose counter was written two lower; max(1, .) at the start
    for it, skipped, plain_it in ((9, 2, 7), (2, 2, 0), (1, 2, 0), (0, 2, 0), (5, 0, 5)):
        a.it.fill_(plain_it)
        b.it.fill_(it)
        a.plain(grads[1])
        b.guarded(grads[1], _state_tensor(scale=1.0, skipped=skipped))
        torch.cuda.synchronize()
        assert torch.equal(b.hyper[1:3].view(torch.int32), a.hyper[1:3].view(torch.int32)), (it, skipped)
        assert float(b.hyper[3]) == it and int(b.it) == it + 1 and int(a.it) == plain_it + 1
    lib = L.lib()
    assert lib.rd_adam_step_guarded(None, one.data_ptr(), _st()) == -1 and lib.rd_adam_step_guarded(C.byref(b.a), None, _st()) == -1
    b.a.n = 0
    assert lib.rd_adam_step_guarded(C.byref(b.a), one.data_ptr(), _st()) == -1


# ------------------------------------------------------------------------------------------------------------- rd_guard_sync
class SyncArena:
    """Range pairs placed by hand in a live and a shadow buffer: range i starts lo / so bytes behind a 16-byte boundary, GAP bytes of
    sentinel in front of and behind every range on both sides.  specs: [(bytes, live offset, shadow offset)]."""

    def __init__(self, specs, seed):
        self.specs, rng = specs, np.random.RandomState(seed)
        self.pos, cur = [], GAP
        for nbytes, lo, so in specs:
            self.pos.append(cur)
            cur = (cur + 16 + nbytes + GAP + 15) // 16 * 16
        self.size = cur + GAP
        self.live_host, self.shadow_host = np.full(self.size, SENT, np.uint8), np.full(self.size, SENT, np.uint8)
        special = np.array([0x7fc00000, 0xffffffff, 0x7f800000, 0xff800001, 0, 0x80000000], np.uint32)       # NaNs, infinities, zeros
        for host, col in ((self.live_host, 1), (self.shadow_host, 2)):
            for p, sp in zip(self.pos, specs):
                w = rng.randint(0, 1 << 32, sp[0] // 4, dtype=np.uint64).astype(np.uint32)
                w[::3] = special[rng.randint(0, special.size, w[::3].size)]
                host[p + sp[col]:p + sp[col] + sp[0]] = w.view(np.uint8)
        self.live, self.shadow = torch.from_numpy(self.live_host).to(DEV), torch.from_numpy(self.shadow_host).to(DEV)
        assert self.live.data_ptr() % 16 == 0 and self.shadow.data_ptr() % 16 == 0
        self.n = len(specs)
        self.arr, self.chunks = G.build_table([(self.live.data_ptr() + p + lo, self.shadow.data_ptr() + p + so, nb)
                                               for p, (nb, lo, so) in zip(self.pos, specs)])
        self.table = G.upload_table(self.arr, self.n, DEV)

    def sync(self, skip):
        """One launch in the direction of the flag; the host model moves the same bytes; both whole buffers are compared."""
        state = _state_tensor(skip=int(skip), scale=1.0)
        src, dst, col_s, col_d = (self.shadow_host, self.live_host, 2, 1) if skip else (self.live_host, self.shadow_host, 1, 2)
        keep = (self.shadow if skip else self.live).clone()
        assert G.run_sync(self.arr, self.table, self.n, self.chunks, state.data_ptr()) == 0
        for p, sp in zip(self.pos, self.specs):
            dst[p + sp[col_d]:p + sp[col_d] + sp[0]] = src[p + sp[col_s]:p + sp[col_s] + sp[0]]
        torch.cuda.synchronize()
        assert torch.equal(self.shadow if skip else self.live, keep), 'the side that is read was written'
        assert np.array_equal(self.live.cpu().numpy(), self.live_host) and np.array_equal(self.shadow.cpu().numpy(), self.shadow_host)


SYNC_SIZES = [4, 8, 60, 16384 + 4]
ALL_PAIRS = [(nb, lo, so) for nb in SYNC_SIZES for lo in (0, 4, 8, 12) for so in (0, 4, 8, 12)]


@pytest.mark.parametrize('count', [1, 7, 64, 200])
def test_guard_sync_moves_the_bytes_in_the_direction_of_the_flag(count):
    """1, 7 and 200 ranges (and the 64 = four sizes x 4 x 4 alignments of live and shadow, each once): 4 B, 8 B (an int64), 60 B and
    16 KiB + 4 B; NaN and arbitrary bit patterns; shadow <- live with the flag clear, live <- shadow with it set, and back."""
    specs = [ALL_PAIRS[(5 * i + 3) % 64] for i in range(count)] if count != 64 else list(ALL_PAIRS)
    if count == 200:
        specs[9] = (0, 0, 0)                                # an empty range between full ones
    ar = SyncArena(specs, seed=count)
    assert not np.array_equal(ar.live_host, ar.shadow_host)
    ar.sync(skip=False)
    ar.live.copy_(torch.from_numpy(np.where(ar.live_host == SENT, ar.live_host, ar.live_host ^ 0x5A).astype(np.uint8)))
    ar.live_host[:] = ar.live.cpu().numpy()                 # the "forward pass" moves the live side
    ar.sync(skip=True)                                      # rolled back
    ar.sync(skip=False)


def test_guard_sync_at_the_chunk_edges():
    """The sizes around a chunk of the walk (csrc/range_walk.h) that the test above does not reach -- one word short of a chunk, a
    whole chunk, and three chunks and a ragged fourth -- each at the 16 pairings of live and shadow offsets mod 16, with an empty
    range between two full ones; both directions."""
    CH = L.GUARD_CHUNK
    specs = [(nb, lo, so) for nb in (CH - 4, CH, 3 * CH + 20) for lo in (0, 4, 8, 12) for so in (0, 4, 8, 12)]
    specs[7:7] = [(0, 0, 0)]
    ar = SyncArena(specs, seed=49)
    assert ar.n == 49 and ar.chunks == 16 * (1 + 1 + 4)
    ar.sync(skip=False)
    ar.live.copy_(torch.from_numpy(np.where(ar.live_host == SENT, ar.live_host, ar.live_host ^ 0x5A).astype(np.uint8)))
    ar.live_host[:] = ar.live.cpu().numpy()
    ar.sync(skip=True)
    ar.sync(skip=False)


def test_guard_sync_validation_codes_and_the_empty_call():
    specs = [(16384 + 4, 0, 0), (0, 0, 0), (64, 4, 8)]
    ar = SyncArena(specs, seed=5)
    lib, st = L.lib(), _state_tensor(scale=1.0)
    live0, shadow0 = ar.live.clone(), ar.shadow.clone()

    def code(table=True, dev=True, n=3, chunks=None, state=st.data_ptr(), **edit):
        arr = (L.RdGuardRange * 3).from_buffer_copy(ar.arr)
        for k, (i, v) in edit.items():
            setattr(arr[i], k, v)
        return lib.rd_guard_sync(arr if table else None, ar.table.data_ptr() if dev else None, n, ar.chunks if chunks is None else chunks,
                                 state, _st())
    assert code(table=False) == -1 and code(dev=False) == -1 and code(state=None) == -1 and code(n=-1) == -1 and code(n=0, state=None) == -1
    assert code(bytes=(0, -4)) == -2 and code(bytes=(0, 16384 + 6)) == -2 and code(bytes=(2, 63)) == -2
    assert code(live=(0, ar.live.data_ptr() + GAP + 2)) == -3 and code(shadow=(2, ar.shadow.data_ptr() + 1)) == -3
    assert code(live=(0, None)) == -3 and code(shadow=(2, None)) == -3 and code(state=st.data_ptr() + 4) == -3
    assert code(chunk0=(1, 1)) == -5 and code(chunk0=(0, 1)) == -5 and code(chunks=ar.chunks + 1) == -5 and code(chunks=0) == -5
    assert code(bytes=(0, 16384)) == -5
    assert code(n=0) == 0 and code(n=0, table=False, dev=False, chunks=0) == 0 and code(n=1, chunks=0, bytes=(0, 0)) == 0
    torch.cuda.synchronize()
    assert torch.equal(ar.live, live0) and torch.equal(ar.shadow, shadow0)
    ar.sync(skip=False)


# ------------------------------------------------------------------------------------------------------------- the trainer
BS, S, STEPS = [2, 3, 3], 32, 11
_OPEN, _CLIP = {}, {}


def _snap(tr):
    b = tr.bank
    return dict(params=b.params.clone(), exp_avg=b.exp_avg.clone(), exp_avg_sq=b.exp_avg_sq.clone(), iter=int(tr.ts.iter),
                losses=tr.ts.losses.clone(), rec_mse=tr.ts.rec_mse.clone(), buffers={k: v.clone() for k, v in b.buffers.items()})


def _same_snap(a, b, what):
    for name in ('params', 'exp_avg', 'exp_avg_sq', 'losses', 'rec_mse'):
        assert torch.equal(_bits(a[name]), _bits(b[name])), (what, name)
    assert a['iter'] == b['iter'] and list(a['buffers']) == list(b['buffers']), what
    for k in a['buffers']:
        assert torch.equal(_bits(a['buffers'][k]), _bits(b['buffers'][k])), (what, k)


def _open_run(dataset):
    """Once per dataset: twin A without a guard and twin B under max_norm = 1e30, 11 pipelined steps in lockstep, compared after every
    step.  Returns A's final state and B's per-step norms."""
    if dataset not in _OPEN:
        batches = _batches(dataset, sum(BS), S, STEPS)
        A, B = _trainer(dataset, BS, S), _trainer(dataset, BS, S)
        gd = B.enable_grad_guard(1e30)
        assert B._guard is gd and B.ts._guard is gd and A.ts._guard is None
        norms = []
        for i in range(STEPS):
            nxt = batches[i + 1] if i + 1 < STEPS else None
            A.step(*batches[i], next_batch=nxt)
            B.step(*batches[i], next_batch=nxt)
            torch.cuda.synchronize()
            _same_snap(_snap(A), _snap(B), ('step', i))
            w = gd.read()
            assert (w['steps'], w['clipped'], w['skipped'], w['skip'], w['nonfinite'], w['scale']) == (i + 1, 0, 0, 0, 0, 1.0), w
            assert np.isfinite(w['norm']) and w['norm'] > 0
            norms.append(w['norm'])
        assert int(A.ts.iter) == STEPS
        _OPEN[dataset] = dict(final=_snap(A), norms=norms)
    return _OPEN[dataset]


def _clip_run(dataset):
    """Once per dataset: the guarded trainer under max_norm = half the median of the open run's norms; every step's state word against
    the model evaluated on that step's read-back gradient."""
    if dataset not in _CLIP:
        max_norm = float(np.median(_open_run(dataset)['norms'])) / 2
        batches = _batches(dataset, sum(BS), S, STEPS)
        tr = _trainer(dataset, BS, S)
        gd = tr.enable_grad_guard(max_norm)
        word, words = None, []
        for i in range(STEPS):
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
            torch.cuda.synchronize()
            got = gd.read()
            word = gd.model(tr.bank.grads.cpu().numpy(), word)
            _same_word(got, word, ('step', i))
            words.append(got)
        _CLIP[dataset] = dict(final=_snap(tr), words=words, max_norm=max_norm)
    return _CLIP[dataset]


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_an_open_guard_changes_nothing(dataset):
    run = _open_run(dataset)
    assert len(run['norms']) == STEPS


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_clipping_applies_the_models_scale(dataset):
    run, plain = _clip_run(dataset), _open_run(dataset)
    words, max_norm = run['words'], run['max_norm']
    assert words[-1]['clipped'] == sum(w['norm'] > max_norm for w in words) >= STEPS // 2 and words[-1]['skipped'] == 0
    assert all((w['scale'] < 1) == (w['norm'] > max_norm) for w in words)
    assert all(_fbits(w['scale']) == _fbits(G.scale_of(w['norm'], max_norm)) for w in words)
    assert not torch.equal(run['final']['params'], plain['final']['params']) and bool(torch.isfinite(run['final']['params']).all())
    assert run['final']['iter'] == STEPS


def test_a_nonfinite_step_leaves_no_trace():
    """Fundus: at step 5 the soft target carries one +inf pixel -- the forward pass stays finite, the BCE gradient does not.  Guarded:
    parameters, both moments and every BatchNorm buffer behind step 5 equal their read-back from before it, iter advanced, skipped
    1; steps 6..10 run finite.  Control: the same plant on the unguarded twin leaves a non-finite value in the parameters."""
    batches = _batches('fundus', sum(BS), S, STEPS)
    batches[5] = batches[5][:3] + (batches[5][3].clone(),)
    batches[5][3][1, 0, 3, 4] = float('inf')
    for guarded in (True, False):
        tr = _trainer('fundus', BS, S)
        gd = tr.enable_grad_guard(0.0) if guarded else None
        for i in range(STEPS):
            if i == 5:
                torch.cuda.synchronize()
                before = _snap(tr)
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
            if i == 5:
                torch.cuda.synchronize()
                after = _snap(tr)
                assert not bool(torch.isfinite(tr.bank.grads).all())
                if guarded:
                    w = gd.read()
                    assert (w['skip'], w['skipped'], w['steps'], w['clipped'], w['scale']) == (1, 1, 6, 0, 1.0) and w['nonfinite'] > 0
                    for name in ('params', 'exp_avg', 'exp_avg_sq'):
                        assert torch.equal(_bits(after[name]), _bits(before[name])), name
                    for k in before['buffers']:
                        assert torch.equal(_bits(after['buffers'][k]), _bits(before['buffers'][k])), k
                    assert after['iter'] == before['iter'] + 1 == 6
                    for k, v in tr.bank.buffers.items():
                        assert torch.equal(_bits(gd.shadows[k]), _bits(v)), k
                else:
                    # the failure the guard is for, seen: the parameters hold non-finite values behind a forward pass that was finite
                    # (the running statistics it left are)
                    assert not bool(torch.isfinite(after['params']).all())
                    assert all(bool(torch.isfinite(v.float()).all()) for v in after['buffers'].values())
                    break
            elif guarded:
                torch.cuda.synchronize()
                w = gd.read()
                assert w['skip'] == 0 and w['skipped'] == int(i > 5) and np.isfinite(w['norm']), (i, w)
        torch.cuda.synchronize()
        if guarded:
            end = _snap(tr)
            assert end['iter'] == STEPS and all(bool(torch.isfinite(end[n]).all()) for n in ('params', 'exp_avg', 'exp_avg_sq', 'losses'))
            assert all(bool(torch.isfinite(v.float()).all()) for v in end['buffers'].values())
            assert not torch.equal(end['params'], after['params'])
            # the bias corrections of the last step count 10 applied updates: t = iter + 1 - skipped
            assert abs(float(tr.ts.hyper[1]) - (1 - B1 ** 10)) < 1e-6 and float(tr.ts.hyper[3]) == 10.0


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_guard_with_step_log_and_averaging_together(dataset):
    """Guard (1e30), the health ring and the weight average behind the same steps: records and the averaged bank equal those of the
    run without the guard."""
    batches = _batches(dataset, sum(BS), S, STEPS)
    out = []
    for guarded in (False, True):
        tr = _trainer(dataset, BS, S)
        if guarded:
            tr.enable_grad_guard(1e30)
        tr.enable_step_log(health=True, rows=16)
        wa = tr.enable_avg_weights('ema', 0.5, 0)
        for i in range(STEPS):
            tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        torch.cuda.synchronize()
        out.append((tr.drain_step_log(), wa.bank.params.clone(), {k: v.clone() for k, v in wa.bank.buffers.items()}, _snap(tr)))
    (rec0, p0, b0, s0), (rec1, p1, b1, s1) = out
    assert rec0 == rec1 and len(rec0) == STEPS and all(r['nonfinite'] == 0 and r['norms'][0] > 0 for r in rec0)
    assert torch.equal(_bits(p0), _bits(p1)) and all(torch.equal(_bits(b0[k]), _bits(b1[k])) for k in b0)
    _same_snap(s0, s1, 'with the ring and the average')
    _same_snap(s0, _open_run(dataset)['final'], 'against the bare twin')


def test_captured_graphs_are_refused():
    tr = _trainer('fundus', [1, 1, 1], 32)
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_grad_guard(1.0)
    assert tr._guard is None and tr.ts._guard is None
    tr._graphs = False
    tr.ts.graph = object()                                  # (what capture() leaves)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_grad_guard(1.0)
    assert tr.ts._guard is None
    tr.ts.graph = None
    gd = tr.enable_grad_guard(1.0)
    with pytest.raises(RuntimeError, match='guarded tail'):
        tr.ts.capture()
    with pytest.raises(ValueError, match='max_norm'):
        tr.enable_grad_guard(-1.0)
    assert tr.ts._guard is gd


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_data_parallel_step_on_one_rank_equals_the_plain_guarded_step(dataset):
    """ddp.DataParallelStep over one rank (no peers: every bucket exchange is the identity) runs segments A, B1, B2 and the guarded
    tail in place of segment C: the state behind 11 pipelined steps equals the plain guarded trainer's."""
    from ramdsir import ddp
    want = _clip_run(dataset)
    batches = _batches(dataset, sum(BS), S, STEPS)
    tr = _trainer(dataset, BS, S)
    runner = ddp.DataParallelStep(tr.ts)                    # built in front of the guard, as FusedTrainer.__init__ does
    tr.runner, tr._step = runner, runner.step
    gd = tr.enable_grad_guard(want['max_norm'])
    for i in range(STEPS):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
    torch.cuda.synchronize()
    _same_snap(_snap(tr), want['final'], 'data parallel, one rank')
    _same_word(gd.read(), want['words'][-1], 'data parallel, one rank')


# ------------------------------------------------------------------------------------------------------------- the CLI
_CLI_NORM = {}
EVERY = ['--log_every', '1']                                # every iteration is a logging iteration: the event file holds every norm


def _guard_scalars(out):
    from utils import tfevents
    logs = os.listdir(os.path.join(out, 'log'))
    assert len(logs) == 1
    got = {}
    for e in tfevents.read_events(os.path.join(out, 'log', logs[0]))[1:]:
        for tag, v in e['scalars']:
            if tag.startswith('guard/'):
                got.setdefault(tag, []).append((e['step'], v))
    return got


def _summary(log):
    m = re.search(r'grad_guard: (\d+) of (\d+) steps clipped, (\d+) skipped', log)
    assert m, log[-3000:]
    return tuple(int(v) for v in m.groups())


def _cli_clip(tmp_path, data, dataset):
    """The clipping norm of the CLI tests: half the median of the norms a --clip_grad_norm 1e30 run of 2 epochs logs."""
    if dataset not in _CLI_NORM:
        out = str(tmp_path / 'probe')
        code, log = _train(data, dataset, out, ['--clip_grad_norm', '1e30'] + EVERY, epochs=2)
        assert code == 0, log[-3000:]
        _CLI_NORM[dataset] = float(np.median([v for _, v in _guard_scalars(out)['guard/grad_norm']])) / 2
    return _CLI_NORM[dataset]


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_an_open_guard_leaves_every_output_alone_and_clipping_changes_the_model(tmp_path, dataset):
    data = _tree(tmp_path, dataset)
    plain, on, clip = (str(tmp_path / n) for n in ('plain', 'on', 'clip'))
    code, log0 = _train(data, dataset, plain, EVERY, epochs=2)
    assert code == 0 and 'grad_guard:' not in log0 and ' grad_norm ' not in log0, log0[-3000:]      # (the Namespace line names the flags)
    code, log1 = _train(data, dataset, on, ['--clip_grad_norm', '1e30'] + EVERY, epochs=2)
    assert code == 0, log1[-3000:]
    assert _read(on, 'final_model.pth') == _read(plain, 'final_model.pth') is not None
    assert _read(on, '0_val_log.csv') == _read(plain, '0_val_log.csv') is not None
    assert _models(on, 'model_') == _models(plain, 'model_') and len(_models(plain, 'model_')) == 1
    iters = 10 if dataset == 'fundus' else 6
    sc = _guard_scalars(on)
    assert sorted(sc) == ['guard/clipped', 'guard/grad_norm', 'guard/scale', 'guard/skipped']
    assert [s for s, _ in sc['guard/grad_norm']] == list(range(iters)) and _summary(log1) == (0, iters, 0)
    assert all(v == 1.0 for _, v in sc['guard/scale']) and all(v == 0.0 for _, v in sc['guard/clipped'] + sc['guard/skipped'])
    assert ' grad_norm ' in log1 and ' clipped 0 skipped 0' in log1
    _CLI_NORM.setdefault(dataset, float(np.median([v for _, v in sc['guard/grad_norm']])) / 2)
    max_norm = _cli_clip(tmp_path, data, dataset)
    code, log2 = _train(data, dataset, clip, ['--clip_grad_norm', repr(max_norm)] + EVERY, epochs=2)
    assert code == 0, log2[-3000:]
    assert _read(clip, 'final_model.pth') != _read(plain, 'final_model.pth')
    sc = _guard_scalars(clip)
    clipped, steps, skipped = _summary(log2)
    assert steps == iters and skipped == 0 == sc['guard/skipped'][-1][1] and clipped == sc['guard/clipped'][-1][1] >= 1
    assert clipped == sum(v < 1 for _, v in sc['guard/scale'])


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_a_resumed_guarded_run_ends_in_the_same_model(tmp_path, dataset):
    """4 epochs with --ckpt_every 1 under the guard against the same run stopped after 2 epochs and resumed: final_model.pth, the CSV
    and the summary counts are equal.  A resume with a changed --clip_grad_norm is refused by name."""
    data = _tree(tmp_path, dataset)
    max_norm = _cli_clip(tmp_path, data, dataset)
    flags = ['--clip_grad_norm', repr(max_norm), '--ckpt_every', '1'] + EVERY
    whole, cut = str(tmp_path / 'whole'), str(tmp_path / 'cut')
    code, log_whole = _train(data, dataset, whole, flags)
    assert code == 0 and 'ckpt: 4 snapshots' in log_whole, log_whole[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    state = os.path.join(cut, 'last_state.pth')
    mid = CK.load_file(state)
    assert [e['name'] for e in mid['table']][-1] == 'guard/state' and mid['meta']['grad_guard'] == dict(max_norm=max_norm)
    word = G.state_dict_of(CK.range_tensor(mid, 'guard/state').numpy())
    assert (word['clipped'], word['steps'], word['skipped']) == _summary(log)
    code, log = _train(data, dataset, cut, ['--clip_grad_norm', repr(max_norm * 2), '--ckpt_every', '1', '--resume', state] + EVERY)
    assert code != 0 and 'grad_guard max_norm' in log, log[-3000:]
    if dataset == 'fundus':
        code, log = _train(data, dataset, cut, ['--ckpt_every', '1', '--resume', state] + EVERY)
        assert code != 0 and 'holds a guard state' in log, log[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--resume', state])
    assert code == 0 and 'continuing at epoch 2' in log, log[-3000:]
    assert _read(cut, '0_val_log.csv') == _read(whole, '0_val_log.csv') is not None
    assert _models(cut, 'model_') == _models(whole, 'model_')
    _same_checkpoint(torch.load(os.path.join(cut, 'final_model.pth'), map_location='cpu'),
                     torch.load(os.path.join(whole, 'final_model.pth'), map_location='cpu'), 'final_model.pth')
    assert _summary(log) == _summary(log_whole) and _summary(log)[1] == (20 if dataset == 'fundus' else 12)
