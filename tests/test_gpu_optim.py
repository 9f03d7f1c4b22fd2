"""-m gpu: train.py --weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult -- rd_optim_step (csrc/optim.hip)
against rd_adam_step and rd_adam_step_guarded on twin arenas (the reference's optimizer is its two-range special case, bit for
bit), the two decay expressions against ramdsir/optim.py decay_model bit for bit, tables of up to 300 ranges against a float64
single-step reference within derived float32 bounds, torch.optim.AdamW / Adam(weight_decay) under a LambdaLR, the schedule words
against schedule_model, every validation code, the fused trainer with enable_optim, and the CLI end to end."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

from ramdsir import _lib as L, ckpt as CK, optim as O       # noqa: E402
from test_gpu_avg_weights import _batches, _models, _read, _same_checkpoint, _train, _trainer, _tree       # noqa: E402
from test_gpu_ckpt import _assert_same_run, _outputs        # noqa: E402
from test_gpu_grad_guard import _clip_run, _open_run, _same_snap, _same_word, _snap, _state_tensor       # noqa: E402

F32 = np.float32
EPS24 = 2.0 ** -24
GAPW = 1024                                                 # 4 KiB of sentinel words in front of and behind every array
SENT = -1515870811                                          # 0xA5A5A5A5 as an int32
B1, B2, ADAM_EPS, BASE_LR, TOTAL = 0.9, 0.999, 1e-8, 2e-3, 50
CHUNK = L.OPT_CHUNK


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fbits(x):
    return int(np.asarray(x, F32).view(np.int32))


def _ibits(t):
    return t.contiguous().view(torch.int32)


class Arena:
    """One Adam arena between sentinels: parameters, gradient and both moments of n floats, each starting `align` words behind a
    16-byte boundary with 4 KiB of sentinel on either side; counter and hyper words of its own (between sentinels as well); an
    rd_adam_t and an rd_optim_t over the same memory."""

    def __init__(self, p0, align, n_half=0, total=TOTAL, base_lr=BASE_LR):
        n = self.n = p0.numel()
        self.bufs, arrs = [], []
        self.aligns = tuple(align) if isinstance(align, tuple) else (align,) * 4         # of param, grad, exp_avg, exp_avg_sq
        for al in self.aligns:
            buf = torch.full((GAPW + 4 + n + GAPW,), SENT, dtype=torch.int32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            self.bufs.append(buf)
            arrs.append(buf[GAPW + al:GAPW + al + n].view(torch.float32))
        self.p, self.g, self.m, self.v = arrs
        self.p.copy_(p0)
        for t in (self.g, self.m, self.v):
            t.zero_()
        self.words = torch.full((GAPW + 8 + GAPW,), SENT, dtype=torch.int32, device=DEV)
        self.it, self.hyper = self.words[GAPW:GAPW + 1], self.words[GAPW + 4:GAPW + 8].view(torch.float32)
        self.it.zero_()
        self.hyper.zero_()
        a = self.a = L.RdAdam()
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.n_half_lr = self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, n_half
        a.iter, a.hyper_out, a.base_lr, a.total_iters = self.it.data_ptr(), self.hyper.data_ptr(), base_lr, total
        a.beta1, a.beta2, a.eps = B1, B2, ADAM_EPS
        d = self.d = L.RdOptim()
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.n, d.iter, d.hyper_out = a.param, a.grad, a.exp_avg, a.exp_avg_sq, n, a.iter, a.hyper_out
        d.base_lr, d.total_iters, d.beta1, d.beta2, d.eps = base_lr, total, B1, B2, ADAM_EPS
        self.set_table([(0, n, 1.0, 0.0)])

    def set_table(self, entries):
        self.entries = entries
        self.arr, self.chunks = O.make_table(entries)
        self.table = O.upload_table(self.arr, DEV)

    def plain(self, g):
        self.g.copy_(g)
        L.check(L.lib().rd_adam_step(C.byref(self.a), _st()), 'rd_adam_step')

    def guarded(self, g, state):
        self.g.copy_(g)
        L.check(L.lib().rd_adam_step_guarded(C.byref(self.a), state.data_ptr(), _st()), 'rd_adam_step_guarded')

    def optim(self, g, state=None):
        self.g.copy_(g)
        L.check(O.run_step(self.d, self.arr, self.table, len(self.entries), self.chunks, None if state is None else state.data_ptr()), 'rd_optim_step')

    def sentinels_intact(self):
        torch.cuda.synchronize()
        for buf, al in zip(self.bufs, self.aligns):
            lo, hi = GAPW + al, GAPW + al + self.n
            assert bool((buf[:lo] == SENT).all()) and bool((buf[hi:] == SENT).all()), 'a sentinel was written'
        w = self.words
        assert bool((w[:GAPW] == SENT).all()) and bool((w[GAPW + 1:GAPW + 4] == SENT).all()) and bool((w[GAPW + 8:] == SENT).all())

    def same(self, other, what):
        torch.cuda.synchronize()
        for name in ('p', 'm', 'v', 'hyper'):
            assert torch.equal(_ibits(getattr(self, name)), _ibits(getattr(other, name))), (what, name)
        assert int(self.it) == int(other.it), what


def _two_ranges(n, n_half):
    """The table of the acceptance property; a boundary at 0 or n leaves the one range that is not empty (count >= 1)."""
    return [(f, c, m, 0.0) for f, c, m in ((0, n_half, 0.5), (n_half, n - n_half, 1.0)) if c > 0]


# ------------------------------------------------------------------------------------------------------------- identity
IDENTITY_N = [1, 255, 257, 1000, 1048869]                   # the last: 257 chunks, and past rd_adam_step's 4096-block grid cap


def _halves(n):
    off = {1: 1, 255: 86, 257: 86, 1000: 333, 1048869: 500001}[n]      # off every chunk (and block) boundary
    assert off % CHUNK and off % 256
    return sorted({0, off, n})


@pytest.mark.parametrize('n', IDENTITY_N)
def test_the_two_range_table_is_rd_adam_step_bit_for_bit(n):
    """Twin arenas between sentinels, 3 steps each: param, both moments, hyper_out and iter equal bit for bit -- for the half-lr
    boundary at 0 (a single range), off every chunk boundary and at n, at the four 4-byte alignments of the arena start; against
    rd_adam_step, against rd_adam_step_guarded at scale 1 and 0.37 and under skip; and once with a NaN parameter, an infinite
    gradient and a NaN moment planted (nothing is compared but bits)."""
    gen = torch.Generator(device=DEV).manual_seed(n)
    p0 = torch.randn(n, generator=gen, device=DEV)
    grads = [torch.randn(n, generator=gen, device=DEV) * (10.0 ** k) for k in (-2, 0, 1)]
    one, s37, skip = _state_tensor(scale=1.0), _state_tensor(scale=0.37), _state_tensor(scale=1.0, skip=1, skipped=1)
    for n_half in _halves(n):
        table = _two_ranges(n, n_half)
        assert len(table) == (2 if 0 < n_half < n else 1)
        for align in range(4):
            for state in (None, one, s37):
                a, b = Arena(p0, align, n_half), Arena(p0, align)
                b.set_table(table)
                for k, g in enumerate(grads):
                    a.plain(g) if state is None else a.guarded(g, state)
                    b.optim(g, state)
                    a.same(b, (n, n_half, align, state is not None, k))
                    assert torch.equal(_ibits(b.g), _ibits(g))              # the gradient is only read
                assert int(b.it) == 3 and not torch.equal(b.p, p0)
                b.sentinels_intact()
            # skip (behind the three steps at scale 0.37): nothing is stored, the counter and the schedule words advance alike
            keep = [t.clone() for t in (b.p, b.m, b.v)]
            a.guarded(grads[0], skip)
            b.optim(torch.full((n,), float('nan'), device=DEV), skip)
            torch.cuda.synchronize()
            for t, k in zip((b.p, b.m, b.v), keep):
                assert torch.equal(_ibits(t), _ibits(k))
            assert int(a.it) == int(b.it) == 4 and torch.equal(_ibits(a.hyper), _ibits(b.hyper))
            b.sentinels_intact()
    # non-finite values, D = 0: the same bits, whatever they are
    n_half = _halves(n)[1]
    a, b = Arena(p0, 1, n_half), Arena(p0, 1)
    b.set_table(_two_ranges(n, n_half))
    g = grads[1].clone()
    for t in (a, b):
        t.p[0] = float('nan')
        t.m[n - 1] = float('nan')
        t.v[n // 2] = float('inf')
    g[n // 3] = float('inf')
    g[n - 1] = float('-inf')
    for k in range(2):
        a.plain(g)
        b.optim(g)
        a.same(b, ('non-finite', k))
    assert not bool(torch.isfinite(b.p).all())


def test_arenas_aligned_differently_from_one_another_go_word_by_word():
    """param, grad and the moments at different offsets from a 16-byte boundary have no common boundary: the same bits as the plain
    step (which is indifferent to alignment), sentinels intact."""
    n, n_half = 9001, 4099
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(11))
    for aligns in ((0, 1, 0, 0), (1, 1, 2, 1), (3, 0, 1, 2), (2, 2, 2, 0)):
        a, b = Arena(p0, 0, n_half), Arena(p0, aligns)
        b.set_table(_two_ranges(n, n_half))
        for k in range(2):
            g = torch.randn(n, device=DEV)
            a.plain(g)
            b.optim(g)
            a.same(b, (aligns, k))
        b.sentinels_intact()


def test_guarded_bias_corrections_count_the_updates_applied():
    """skipped = 2: the bias corrections of rd_adam_step_guarded at the same counter; max(1, .) at the start."""
    n = 1000
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    g = torch.randn(n, device=DEV)
    a, b = Arena(p0, 0, 333), Arena(p0, 0)
    b.set_table(_two_ranges(n, 333))
    for it, skipped in ((9, 2), (2, 2), (1, 2), (0, 2), (5, 0)):
        for t in (a, b):
            t.it.fill_(it)
            t.p.copy_(p0)
            t.m.zero_()
            t.v.zero_()
        st = _state_tensor(scale=1.0, skipped=skipped)
        a.guarded(g, st)
        b.optim(g, st)
        a.same(b, (it, skipped))
        assert float(b.hyper[3]) == it and int(b.it) == it + 1
        assert abs(float(b.hyper[1]) - (1 - B1 ** max(1, it + 1 - skipped))) < 1e-6


# ------------------------------------------------------------------------------------------------------------- decay in isolation
@pytest.mark.parametrize('mode', ['decoupled', 'l2'])
@pytest.mark.parametrize('D', [0.01, 0.5])
@pytest.mark.parametrize('mult', [0.5, 1.0])
def test_decay_in_isolation_bit_for_bit(mode, D, mult):
    """Zero gradients and zero moments.  Decoupled: Adam's update is exactly 0, so after one step param == decay_model(param) bit
    for bit and the moments stay 0.  L2: the gradient the update sees is decay_model's fma(D, param, 0); a twin arena stepped by
    rd_adam_step on THAT gradient ends in the same bits (parameters and both moments).  Exempt ranges (D = 0) are untouched; under a
    guard's skip nothing moves.  Dyadic parameters; ranges that start off every 16-byte boundary; the four alignments."""
    entries = [(0, 5, mult, D), (5, 4100, mult, 0.0), (4105, 300, mult, D), (4405, 3, mult, 0.0), (4408, 4097, mult, D)]
    n = 4408 + 4097
    rng = np.random.RandomState(int(D * 100) + (mode == 'l2'))
    p0 = torch.from_numpy((rng.randint(-512, 513, n) / 64.0).astype(F32))
    p0[7], p0[4106] = 0.0, -0.0
    decays = np.zeros(n, bool)
    for f, c, _, d in entries:
        decays[f:f + c] = d > 0
    zero = torch.zeros(n, device=DEV)
    for align in range(4):
        b = Arena(p0, align)
        b.set_table(entries)
        b.d.wd_mode = O.WD_MODES[mode]
        b.optim(zero)
        torch.cuda.synchronize()
        lr = F32(b.hyper[0].item())
        assert _fbits(lr) == _fbits(F32(BASE_LR))
        want_p, want_g = O.decay_model(p0.numpy(), np.zeros(n, F32), lr, mult, D, mode)
        got = b.p.cpu().numpy()
        assert np.array_equal(got[~decays].view(np.int32), p0.numpy()[~decays].view(np.int32)), 'an exempt range moved'
        assert not b.m[torch.from_numpy(~decays).to(DEV)].any() and not b.v[torch.from_numpy(~decays).to(DEV)].any()
        if mode == 'decoupled':
            assert np.array_equal(got[decays].view(np.int32), want_p[decays].view(np.int32))
            assert not b.m.any() and not b.v.any()
            moved = decays & (p0.numpy() != 0)
            assert moved.sum() > 4000 and (got[moved] != p0.numpy()[moved]).all()      # every decayed parameter but the zeros
        else:
            a = Arena(p0, align, n if mult == 0.5 else 0)
            a.plain(torch.from_numpy(np.where(decays, want_g, F32(0))).to(DEV))
            a.same(b, ('l2 against the plain step on the decayed gradient', align))
            assert bool((b.m[torch.from_numpy(decays & (p0.numpy() != 0)).to(DEV)] != 0).all())
        assert not b.g.any()                                    # the gradient arena is only read
        b.sentinels_intact()
        # under skip nothing moves
        keep = [t.clone() for t in (b.p, b.m, b.v)]
        b.optim(zero, _state_tensor(scale=1.0, skip=1, skipped=1))
        torch.cuda.synchronize()
        assert all(torch.equal(_ibits(t), _ibits(k)) for t, k in zip((b.p, b.m, b.v), keep)) and int(b.it) == 2
        b.sentinels_intact()


def test_decoupled_decay_with_a_gradient_equals_the_plain_step_on_the_decayed_parameter():
    """Random gradients and moments: decoupled decay is `param *= keep` in front of the update, so a twin whose parameters were
    multiplied on the host and stepped by rd_adam_step ends in the same bits; L2 likewise on the host-formed gradient; under a guard
    at scale 0.37 the L2 term is added behind the scale."""
    n, D = 9000, 0.05
    gen = torch.Generator().manual_seed(9)
    p0, g, m0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    v0 = torch.rand(n, generator=gen) * 0.01
    for mode in ('decoupled', 'l2'):
        for state_scale in (None, 0.37):
            state = None if state_scale is None else _state_tensor(scale=state_scale)
            b = Arena(p0, 3)
            b.set_table([(0, n, 0.5, D)])
            b.d.wd_mode = O.WD_MODES[mode]
            b.m.copy_(m0)
            b.v.copy_(v0)
            b.it.fill_(4)
            gs = g if state is None else (g.to(DEV) * torch.tensor(state_scale, dtype=torch.float32, device=DEV)).cpu()
            lr = O.schedule_model(4, BASE_LR, TOTAL)
            want_p, want_g = O.decay_model(p0.numpy(), gs.numpy(), lr, 0.5, D, mode)
            a = Arena(torch.from_numpy(want_p), 3, n)
            a.m.copy_(m0)
            a.v.copy_(v0)
            a.it.fill_(4)
            a.plain(torch.from_numpy(want_g))
            b.optim(g, state)
            a.same(b, (mode, state_scale))
            assert _fbits(b.hyper[0].item()) == _fbits(lr)


# ------------------------------------------------------------------------------------------------------------- ranges
def optim_reference(p0, m0, v0, g, hyper, mult, decay, mode):
    """One step in float64 from the device's own pre-step state and hyper_out, per element multiplier `mult` and decay `decay`, with
    the bound each output is held to: the derivation of adam_reference (tests/test_gpu_loss_edges.py; e = 2^-24, every operation
    correctly rounded, an fma only removes roundings), extended by the operations the grouped kernel adds.
      lr_g = M * lr                       one more rounding in the step size (M = 0.5 and 1 are exact; the bound does not use that):
                                          9 e |u| becomes 10 e |u|.
      decoupled: w = p0 * (1 - lr_g D)    lr_g D rounds once (relative e on a term far below 1), the subtraction once (e), the product
                                          once: |dw| <= 3 e |p0| (1 + e) held as 3 e |p0|; p = w - u rounds once more: e |p|.
      l2: g' = fma(D, p0, g)              one rounding: |dg'| <= e |g'|.  It enters m through (1 - b1) g': + (1 - b1) e |g'| = e |Bt|,
                                          and v through ((1 - b2) g') g': + 2 e B2 -- |dv| <= e (2 A2 + 5 B2) <= 5 e v, so sqrt(v) inherits
                                          2.5 e instead of 1.5 e and the denominator 6.5 e instead of 5.5 e: 11 e |u| in all.
    The one form 11 e |u| + 3 e |p0| (decayed elements only) + e |p| covers both modes."""
    p0, m0, v0, g, mult, decay = (np.asarray(t, np.float64) for t in (p0, m0, v0, g, mult, decay))
    lr, bc1, bc2 = (float(hyper[k]) for k in range(3))
    b1, b2, eps = float(F32(B1)), float(F32(B2)), float(F32(ADAM_EPS))
    lr_g = mult * lr
    on = decay > 0
    w = np.where(on & (mode == 0), p0 * (1.0 - lr_g * decay), p0)
    ge = np.where(on & (mode == 1), decay * p0 + g, g)
    dg = np.where(on & (mode == 1), EPS24 * np.abs(ge), 0.0)
    A, Bt = b1 * m0, (1.0 - b1) * ge
    m = A + Bt
    A2, B2t = b2 * v0, (1.0 - b2) * ge * ge
    v = A2 + B2t
    s = lr_g / bc1
    d = np.sqrt(v) / math.sqrt(bc2) + eps
    u = s * (m / d)
    p = w - u
    slack = 1.0 + 1e-6
    m_abs = EPS24 * (np.abs(A) + np.abs(Bt) + np.abs(m)) + (1.0 - b1) * dg
    m_tol = m_abs * slack + 3e-45
    v_tol = EPS24 * (2 * A2 + 5 * B2t) * slack + 5e-45
    p_tol = (EPS24 * np.abs(p) + 11 * EPS24 * np.abs(u) + (s / d) * m_abs + np.where(on, 3 * EPS24 * np.abs(p0), 0.0)) * slack + 1e-45
    return (p, m, v), (p_tol, m_tol, v_tol)


COUNTS = (1, 3, 16, 4095, 4096, 4097)
SETTINGS = ((0.5, 0.0), (1.0, 0.01), (0.25, 0.5), (1.0, 0.0), (2.0, 0.1))


@pytest.mark.parametrize('n_ranges', [1, 7, 64, 300])
@pytest.mark.parametrize('mode', [0, 1])
def test_tables_of_many_ranges_against_the_float64_reference(n_ranges, mode):
    """1 / 7 / 64 / 300 ranges with counts from {1, 3, 16, 4095, 4096, 4097} (below, at and above one chunk; starts at every 4-byte
    alignment) and alternating (lr_mult, D): two steps, each element held to optim_reference computed from the state read back
    before the step.  Sentinels intact."""
    rng = np.random.RandomState(n_ranges)
    counts = [COUNTS[(i * 5 + n_ranges) % 6] for i in range(n_ranges)] if n_ranges > 1 else [4097]
    entries, first = [], 0
    for i, c in enumerate(counts):
        entries.append((first, c) + SETTINGS[i % len(SETTINGS)] if n_ranges > 1 else (0, c, 0.5, 0.01))
        first += c
    n = first
    mult, decay = np.zeros(n), np.zeros(n)
    for f, c, m_, d_ in entries:
        mult[f:f + c], decay[f:f + c] = float(F32(m_)), float(F32(d_))
    p0 = torch.from_numpy(rng.randn(n).astype(F32))
    b = Arena(p0, n_ranges % 4)
    b.set_table(entries)
    b.d.wd_mode = mode
    assert b.chunks == sum(-(-c // CHUNK) for c in counts)
    worst = [0.0, 0.0, 0.0]
    for step in range(2):
        g = torch.from_numpy((rng.randn(n) * 10.0 ** rng.uniform(-2, 1)).astype(F32))
        pre = [t.cpu().numpy() for t in (b.p, b.m, b.v)]
        b.optim(g.to(DEV))
        b.sentinels_intact()
        hyper = b.hyper.cpu().numpy()
        assert float(hyper[3]) == step and int(b.it) == step + 1
        ref, tol = optim_reference(pre[0], pre[1], pre[2], g.numpy(), hyper, mult, decay, mode)
        for k, (name, t) in enumerate(zip(('param', 'exp_avg', 'exp_avg_sq'), (b.p, b.m, b.v))):
            got = t.cpu().double().numpy()
            assert np.isfinite(got).all()
            err = np.abs(got - ref[k])
            worst[k] = max(worst[k], float((err / tol[k]).max()))
            bad = np.flatnonzero(err > tol[k])
            assert bad.size == 0, '%s step %d: %d elements beyond the bound, first %d: err %.3e bound %.3e' % (
                name, step, bad.size, bad[0], err[bad[0]], tol[k][bad[0]])
        assert not np.array_equal(b.p.cpu().numpy(), pre[0])
    print('ranges %d mode %d: worst err / bound param %.3f exp_avg %.3f exp_avg_sq %.3f' % (n_ranges, mode, *worst))


# ------------------------------------------------------------------------------------------------------------- torch
@pytest.mark.parametrize('mode,schedule,warmup', [('decoupled', 'cosine', 3), ('l2', 'poly', 0), ('decoupled', 'constant', 0)])
def test_against_torch_optim_with_param_groups_and_lambda_lr(mode, schedule, warmup):
    """torch.optim.AdamW (decoupled) / torch.optim.Adam(weight_decay) (l2) over four param groups that mirror the table, 5 steps,
    the rate driven by a LambdaLR whose lambda is the documented formula; 1000 parameters; the tolerance of
    test_adam_matches_torch_optim_with_poly_lr (rtol 1e-5, atol 2e-7): the decay adds at most three roundings of relative size 6e-8
    per step to a parameter, far inside it."""
    gen = torch.Generator().manual_seed(51)
    n, base_lr, total = 1000, 2e-3, 40
    entries = [(0, 300, 0.5, 0.0), (300, 250, 0.5, 0.02), (550, 50, 1.0, 0.0), (600, 400, 1.0, 0.02)]
    p0 = torch.randn(n, generator=gen)
    params = [torch.nn.Parameter(p0[f:f + c].clone()) for f, c, _, _ in entries]
    groups = [dict(params=[p], lr=base_lr * m, weight_decay=d) for p, (_, _, m, d) in zip(params, entries)]
    opt = (torch.optim.AdamW if mode == 'decoupled' else torch.optim.Adam)(groups, lr=base_lr, betas=(0.9, 0.999), eps=1e-8)

    def lam(it):
        if schedule == 'poly':
            s = 1.0 if it == 0 else (1.0 - (it - 1) / total) ** 0.9
        elif schedule == 'cosine':
            s = 0.5 * (1.0 + math.cos(math.pi * min(it, total) / total))
        else:
            s = 1.0
        return s * (min(1.0, (it + 1) / warmup) if warmup > 0 else 1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    b = Arena(p0, 2, total=total, base_lr=base_lr)
    b.set_table(entries)
    b.d.schedule, b.d.warmup_iters, b.d.wd_mode = O.SCHEDULES[schedule], warmup, O.WD_MODES[mode]
    for step in range(5):
        g = torch.randn(n, generator=gen)
        for p, (f, c, _, _) in zip(params, entries):
            p.grad = g[f:f + c].clone()
        assert abs(opt.param_groups[3]['lr'] - float(O.schedule_model(step, base_lr, total, schedule, warmup))) < 1e-9
        opt.step()
        sched.step()
        b.optim(g.to(DEV))
        torch.cuda.synchronize()
        ref = torch.cat([p.data for p in params])
        np.testing.assert_allclose(b.p.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=2e-7)
    assert int(b.it) == 5


# ------------------------------------------------------------------------------------------------------------- schedule words
@pytest.mark.parametrize('schedule', ['poly', 'cosine', 'constant'])
@pytest.mark.parametrize('warmup', [0, 3])
def test_schedule_words_over_every_iteration(schedule, warmup):
    """hyper_out over all iterations of a 7-iteration schedule (and two beyond its end for cosine and constant): the lr within one
    float32 ulp of schedule_model, the bias corrections within one ulp of 1 - beta^(it + 1), the iteration number exact; a counter
    written from the host is honoured."""
    n, total = 1000, 7
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(7))
    b = Arena(p0, 0, total=total)
    b.set_table([(0, 400, 0.5, 0.01), (400, 600, 1.0, 0.0)])
    b.d.schedule, b.d.warmup_iters = O.SCHEDULES[schedule], warmup
    g = torch.randn(n, device=DEV)
    worst = 0

    def check(it):
        nonlocal worst
        h = b.hyper.cpu().numpy()
        want = O.schedule_model(it, BASE_LR, total, schedule, warmup)
        ulps = abs(_fbits(h[0]) - _fbits(want))
        worst = max(worst, ulps)
        assert ulps <= 1, (schedule, warmup, it, float(h[0]), float(want))
        for k, beta in ((1, B1), (2, B2)):
            w = F32(1.0 - float(F32(beta)) ** (it + 1))
            assert abs(float(h[k]) - float(w)) <= float(np.spacing(w)), (k, it)
        assert float(h[3]) == float(it) and int(b.it) == it + 1
    for it in range(total if schedule == 'poly' else total + 2):
        b.optim(g)
        torch.cuda.synchronize()
        check(it)
    if schedule == 'cosine':
        assert float(b.hyper[0]) == 0.0                         # at and beyond the end
    if schedule == 'constant':
        assert _fbits(b.hyper[0].item()) == _fbits(F32(BASE_LR))
    b.it.fill_(5)                                               # a resumed run sets the counter from the host
    b.optim(g)
    torch.cuda.synchronize()
    check(5)
    b.it.fill_(1)
    b.optim(g)
    torch.cuda.synchronize()
    check(1)
    assert bool(torch.isfinite(b.p).all())
    b.sentinels_intact()
    print('schedule %s warmup %d: lr within %d ulp of schedule_model' % (schedule, warmup, worst))


# ------------------------------------------------------------------------------------------------------------- validation
def test_every_validation_code_and_nothing_is_launched_on_refusal():
    n = 10000
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    b = Arena(p0, 1)
    b.set_table([(0, 5000, 0.5, 0.0), (5000, 1, 1.0, 0.01), (5001, n - 5001, 1.0, 0.0)])
    b.g.copy_(torch.randn(n))
    b.it.fill_(3)
    before = [x.clone() for x in b.bufs] + [b.words.clone()]
    lib, st = L.lib(), _state_tensor(scale=1.0)

    def code(table=True, dev=True, n_ranges=3, chunks=None, desc=True, rng=(), guard=None, **edit):
        d = L.RdOptim.from_buffer_copy(b.d)
        for k, v in edit.items():
            setattr(d, k, v)
        arr = (L.RdOptimRange * 3).from_buffer_copy(b.arr)
        for i, k, v in rng:
            setattr(arr[i], k, v)
        return lib.rd_optim_step(C.byref(d) if desc else None, arr if table else None, b.table.data_ptr() if dev else None, n_ranges,
                                 b.chunks if chunks is None else chunks, guard, _st())
    for guard in (None, st.data_ptr()):
        assert code(desc=False, guard=guard) == -1 and code(table=False, guard=guard) == -1 and code(dev=False, guard=guard) == -1
        for f in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'iter', 'hyper_out'):
            assert code(guard=guard, **{f: None}) == -1, f
        assert code(n=0, guard=guard) == -1 and code(n_ranges=0, guard=guard) == -1 and code(n_ranges=4097, guard=guard) == -1
        assert code(rng=[(1, 'count', 0)], guard=guard) == -2 and code(rng=[(1, 'first', 4999)], guard=guard) == -2
        assert code(n=n + 1, guard=guard) == -2 and code(n=n - 1, guard=guard) == -2 and code(n_ranges=2, chunks=3, guard=guard) == -2
        assert code(rng=[(0, 'lr_mult', 0.0)], guard=guard) == -3 and code(rng=[(0, 'lr_mult', float('nan'))], guard=guard) == -3
        assert code(rng=[(0, 'lr_mult', float('inf'))], guard=guard) == -3 and code(rng=[(2, 'lr_mult', -1.0)], guard=guard) == -3
        assert code(rng=[(1, 'weight_decay', -0.01)], guard=guard) == -3 and code(rng=[(1, 'weight_decay', float('nan'))], guard=guard) == -3
        assert code(rng=[(1, 'weight_decay', float('inf'))], guard=guard) == -3
        assert code(schedule=3, guard=guard) == -4 and code(schedule=-1, guard=guard) == -4 and code(wd_mode=2, guard=guard) == -4
        assert code(warmup_iters=-1, guard=guard) == -4 and code(warmup_iters=TOTAL, guard=guard) == -4
        assert code(rng=[(1, 'chunk0', 1)], guard=guard) == -5 and code(rng=[(2, 'chunk0', 4)], guard=guard) == -5
        assert code(chunks=b.chunks + 1, guard=guard) == -5 and code(chunks=0, guard=guard) == -5
    torch.cuda.synchronize()
    for x, y in zip(b.bufs + [b.words], before):
        assert torch.equal(x, y), 'a refused call wrote'
    assert int(b.it) == 3
    assert code() == 0 and code(warmup_iters=TOTAL - 1, schedule=2, wd_mode=1) == 0 and code(guard=st.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(b.it) == 6
    b.sentinels_intact()


# ------------------------------------------------------------------------------------------------------------- the trainer
BS, S, STEPS = [2, 3, 3], 32, 11
_DECAY = {}


def _run(tr, dataset, each=None):
    batches = _batches(dataset, sum(BS), S, STEPS)
    for i in range(STEPS):
        tr.step(*batches[i], next_batch=batches[i + 1] if i + 1 < STEPS else None)
        if each is not None:
            each(i)
    torch.cuda.synchronize()


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_enable_optim_with_default_values_changes_nothing(dataset):
    """(a) the grouped Adam under its default settings against the plain twin: parameters, moments, BatchNorm buffers, losses and
    counter equal bit for bit behind 11 pipelined steps; the table is the two ranges of the reference."""
    tr = _trainer(dataset, BS, S)
    op = tr.enable_optim()
    assert tr._optim is op and tr.ts._optim is op and op.settings() == O.DEFAULTS
    enc_end = tr.bank.module_range['enc'][1]
    assert op.entries == [(0, enc_end, 0.5, 0.0), (enc_end, tr.bank.n - enc_end, 1.0, 0.0)] and op.n == 2 and op.decayed_elements() == 0
    _run(tr, dataset)
    _same_snap(_snap(tr), _open_run(dataset)['final'], 'enable_optim() with the default values')
    assert _fbits(tr.lr()) == _fbits(O.schedule_model(STEPS - 1, 1e-3, 40))


def _decay_run():
    """Once: the fundus trainer under decoupled decay 0.05, cosine, warm-up 3, encoder multiplier 0.25; every step held to
    optim_reference over read-backs (pre-step state, the gradient the step left, its hyper words)."""
    if not _DECAY:
        tr = _trainer('fundus', BS, S)
        op = tr.enable_optim(weight_decay=0.05, lr_schedule='cosine', warmup_iters=3, enc_lr_mult=0.25)
        bank = tr.bank
        mult, decay = np.zeros(bank.n), np.zeros(bank.n)
        for f, c, m_, d_ in op.entries:
            mult[f:f + c], decay[f:f + c] = m_, d_
        pre = [None]

        def grab():
            torch.cuda.synchronize()
            pre[0] = [t.cpu().numpy() for t in (bank.params, bank.exp_avg, bank.exp_avg_sq)]
        grab()
        lrs = []

        def each(i):
            torch.cuda.synchronize()
            hyper = tr.ts.hyper.cpu().numpy()
            lrs.append(hyper[0])
            assert float(hyper[3]) == i
            ref, tol = optim_reference(*pre[0], bank.grads.cpu().numpy(), hyper, mult, decay, 0)
            for k, t in enumerate((bank.params, bank.exp_avg, bank.exp_avg_sq)):
                err = np.abs(t.cpu().double().numpy() - ref[k])
                assert (err <= tol[k]).all(), (i, k, int((err > tol[k]).sum()))
            grab()
        _run(tr, 'fundus', each)
        _DECAY.update(final=_snap(tr), entries=op.entries, lrs=lrs, n=op.n, decayed=op.decayed_elements())
    return _DECAY


def test_trainer_with_weight_decay_follows_the_reference_and_moves_the_conv_kernels():
    """(b) every element of every step within optim_reference's bounds (exempt tensors: the plain Adam arithmetic on this run's own
    gradients; conv kernels: with the decay); the lr words are schedule_model's; against the plain twin the conv kernels differ."""
    run, plain = _decay_run(), _open_run('fundus')['final']
    assert run['n'] > 20 and 0 < run['decayed'] < run['final']['params'].numel()
    for i, lr in enumerate(run['lrs']):
        assert abs(_fbits(lr) - _fbits(O.schedule_model(i, 1e-3, 40, 'cosine', 3))) <= 1, i
    p, q = run['final']['params'], plain['params']
    assert bool(torch.isfinite(p).all()) and run['final']['iter'] == STEPS
    for f, c, _, d in run['entries']:
        if d > 0 and c >= 64:
            assert not torch.equal(p[f:f + c], q[f:f + c]), (f, c)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_optim_with_guard_ring_and_averaging_together(dataset):
    """(c) the grouped Adam (default values) under an active guard (the clipping norm of the guard's own twin test), with the health
    ring and the weight average behind the same steps: the final state and the guard's state word equal those of the guarded run
    without enable_optim, whichever of the two is enabled first; the ring holds every step."""
    want = _clip_run(dataset)
    for optim_first in (True, False):
        tr = _trainer(dataset, BS, S)
        if optim_first:
            tr.enable_optim()
        gd = tr.enable_grad_guard(want['max_norm'])
        if not optim_first:
            tr.enable_optim()
        tr.enable_step_log(health=True, rows=16)
        wa = tr.enable_avg_weights('ema', 0.5, 0)
        _run(tr, dataset)
        _same_snap(_snap(tr), want['final'], ('guard + optim', optim_first))
        _same_word(gd.read(), want['words'][-1], ('guard + optim', optim_first))
        assert gd.read()['clipped'] >= STEPS // 2
        rec = tr.drain_step_log()
        assert len(rec) == STEPS and all(r['nonfinite'] == 0 for r in rec) and bool(torch.isfinite(wa.bank.params).all())
    # and with a decay under the same guard: runs, clips, stays finite, differs
    tr = _trainer(dataset, BS, S)
    tr.enable_optim(weight_decay=0.05, wd_mode='l2')
    gd = tr.enable_grad_guard(want['max_norm'])
    _run(tr, dataset)
    end = _snap(tr)
    assert bool(torch.isfinite(end['params']).all()) and gd.read()['clipped'] >= 1 and not torch.equal(end['params'], want['final']['params'])


def test_data_parallel_step_on_one_rank_equals_the_plain_optim_step():
    """(d) ddp.DataParallelStep over one rank runs segments A, B1, B2 and rd_optim_step + repack in place of segment C: the state
    behind 11 pipelined steps equals the plain trainer's under the same settings."""
    from ramdsir import ddp
    want = _decay_run()
    tr = _trainer('fundus', BS, S)
    runner = ddp.DataParallelStep(tr.ts)
    tr.runner, tr._step = runner, runner.step
    tr.enable_optim(weight_decay=0.05, lr_schedule='cosine', warmup_iters=3, enc_lr_mult=0.25)
    _run(tr, 'fundus')
    _same_snap(_snap(tr), want['final'], 'data parallel, one rank')


def test_captured_graphs_and_bad_settings_are_refused():
    tr = _trainer('fundus', [1, 1, 1], 32)
    tr._graphs = True                                       # (what use_graph=True leaves; nothing is captured here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_optim(weight_decay=0.01)
    tr._graphs = False
    tr.ts.graph = object()                                  # (what capture() leaves)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_optim(weight_decay=0.01)
    assert tr.ts._optim is None
    tr.ts.graph = None
    with pytest.raises(ValueError, match='warmup_iters 40 is not below the 40 iterations'):
        tr.enable_optim(warmup_iters=40)
    with pytest.raises(ValueError, match='optim: weight_decay'):
        tr.enable_optim(weight_decay=-1.0)
    assert tr.ts._optim is None
    op = tr.enable_optim(weight_decay=0.01)
    with pytest.raises(RuntimeError, match='grouped Adam'):
        tr.ts.capture()
    from ramdsir import ddp
    with pytest.raises(RuntimeError, match='grouped Adam'):
        ddp.DataParallelStep(tr.ts).capture()
    assert tr.ts._optim is op


# ------------------------------------------------------------------------------------------------------------- the CLI
EVERY = ['--log_every', '1', '--lr', '0.001']
SPELLED = ['--weight_decay', '0', '--wd_mode', 'decoupled', '--lr_schedule', 'poly', '--warmup_iters', '0', '--enc_lr_mult', '0.5']


def _lr_records(out):
    return [(s, v) for s, t, v in _outputs(out, None)['scalars'] if t == 'lr']


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_defaults_spelled_out_and_the_schedules(tmp_path, dataset):
    """The five flags at their defaults spelled out against a run without them: final_model.pth bytes, CSV, keep-best names, scalar
    records.  --lr_schedule constant: every lr record is --lr.  --lr_schedule cosine --warmup_iters 3: the lr records are
    schedule_model's to one ulp."""
    data = _tree(tmp_path, dataset)
    plain, spelled, const, cos = (str(tmp_path / n) for n in ('plain', 'spelled', 'const', 'cos'))
    iters = 10 if dataset == 'fundus' else 6
    code, log0 = _train(data, dataset, plain, EVERY, epochs=2)
    assert code == 0 and 'optim:' not in log0, log0[-3000:]
    code, log1 = _train(data, dataset, spelled, EVERY + SPELLED, epochs=2)
    assert code == 0 and 'optim:' not in log1, log1[-3000:]
    assert _read(spelled, 'final_model.pth') == _read(plain, 'final_model.pth') is not None
    _assert_same_run(_outputs(plain, dataset), _outputs(spelled, dataset), 'the defaults spelled out')
    lr0 = _lr_records(plain)
    assert [s for s, _ in lr0] == list(range(iters))
    assert all(abs(_fbits(v) - _fbits(O.schedule_model(s, 1e-3, iters))) <= 1 for s, v in lr0)
    code, log2 = _train(data, dataset, const, EVERY + ['--lr_schedule', 'constant'], epochs=2)
    assert code == 0 and 'optim: constant schedule, warmup 0, encoder lr x 0.5; weight decay 0 (decoupled) over 2 ranges, 0 of ' in log2, log2[-3000:]
    lr2 = _lr_records(const)
    assert [s for s, _ in lr2] == list(range(iters)) and all(_fbits(v) == _fbits(F32(1e-3)) for _, v in lr2)
    assert _read(const, 'final_model.pth') != _read(plain, 'final_model.pth')
    code, log3 = _train(data, dataset, cos, EVERY + ['--lr_schedule', 'cosine', '--warmup_iters', '3'], epochs=2)
    assert code == 0 and 'optim: cosine schedule, warmup 3' in log3, log3[-3000:]
    lr3 = _lr_records(cos)
    assert [s for s, _ in lr3] == list(range(iters))
    assert all(abs(_fbits(v) - _fbits(O.schedule_model(s, 1e-3, iters, 'cosine', 3))) <= 1 for s, v in lr3)
    assert lr3[0][1] < lr3[2][1] > lr3[-1][1]
    # the one refusal that needs the length of the run
    code, log4 = _train(data, dataset, str(tmp_path / 'warm'), EVERY + ['--warmup_iters', str(iters)], epochs=2)
    assert code != 0 and '--warmup_iters %d is not below the %d iterations' % (iters, iters) in log4, log4[-3000:]


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_a_resumed_run_with_decay_and_cosine_ends_in_the_same_model(tmp_path, dataset):
    """4 epochs with --weight_decay 0.01 --lr_schedule cosine against the same run stopped after 2 epochs and resumed: equal
    final_model.pth, CSV, keep-best names and scalar records.  A resume under a changed --weight_decay, or without the flags, is
    refused by name."""
    data = _tree(tmp_path, dataset)
    flags = ['--weight_decay', '0.01', '--lr_schedule', 'cosine', '--ckpt_every', '1']
    whole, cut = str(tmp_path / 'whole'), str(tmp_path / 'cut')
    code, log_whole = _train(data, dataset, whole, flags)
    assert code == 0 and 'ckpt: 4 snapshots' in log_whole and 'optim: cosine schedule' in log_whole, log_whole[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--stop_after_epochs', '2'])
    assert code == 0 and 'Stopped after 2 epochs' in log, log[-3000:]
    state = os.path.join(cut, 'last_state.pth')
    mid = CK.load_file(state)
    assert mid['meta']['optim'] == dict(weight_decay=0.01, wd_mode='decoupled', lr_schedule='cosine', warmup_iters=0, enc_lr_mult=0.5)
    assert not any('optim' in e['name'] for e in mid['table'])
    code, log = _train(data, dataset, cut, ['--weight_decay', '0.02', '--lr_schedule', 'cosine', '--ckpt_every', '1', '--resume', state])
    assert code != 0 and 'optim weight_decay = 0.01, this run has 0.02' in log, log[-3000:]
    if dataset == 'fundus':
        code, log = _train(data, dataset, cut, ['--ckpt_every', '1', '--resume', state])
        assert code != 0 and 'optim weight_decay = 0.01, this run has 0.0' in log, log[-3000:]
    code, log = _train(data, dataset, cut, flags + ['--resume', state])
    assert code == 0 and 'continuing at epoch 2' in log, log[-3000:]
    assert _read(cut, '0_val_log.csv') == _read(whole, '0_val_log.csv') is not None
    assert _models(cut, 'model_') == _models(whole, 'model_')
    _same_checkpoint(torch.load(os.path.join(cut, 'final_model.pth'), map_location='cpu'),
                     torch.load(os.path.join(whole, 'final_model.pth'), map_location='cpu'), 'final_model.pth')
    _assert_same_run(_outputs(whole, dataset), _outputs(cut, dataset), 'stopped after two epochs and resumed')
