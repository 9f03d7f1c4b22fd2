"""CPU-only tests of train.py --accum_steps (ramdsir/accum.py; rd_grad_accum in csrc/accum.hip): the exported symbol, every refusal
code of the entry point (they come back before anything is launched, so no GPU is needed), the numpy model against rows worked out in
exact rational arithmetic and within a derived bound of the float64 mean, the update count and the trailing remainder of the test
trees' runs, train.py's refusals, the resume refusals, and GradAccum over a CPU ParamBank.  No GPU call."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from ramdsir import _lib as L, accum as A, ckpt as CK       # noqa: E402
from fake_trainer import fake_state as _fake_state, fake_trainer as _fake_trainer       # noqa: E402
from test_cpu_grad_guard import _round_f32, _train_module       # noqa: E402

F32 = np.float32


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _fr(v):
    return Fraction(float(v))


# ------------------------------------------------------------------------------------------------------------- the entry point
def test_the_symbol_is_exported():
    assert 'rd_grad_accum' in L.exported_symbols()
    assert L.lib().rd_grad_accum is not None                    # resolves in the built library
    for name in ('rd_adam_step', 'rd_adam_step_guarded', 'rd_optim_step', 'rd_avg_step'):      # untouched beside it
        assert getattr(L.lib(), name) is not None
    assert L.ACCUM_MAX_STEPS == A.MAX_STEPS == 65536


class HostRig:
    """Two host arrays the entry point is pointed at: every refusal returns before a launch, so nothing dereferences them."""

    def __init__(self, n=1000):
        self.n = n
        self.buf = np.zeros(2 * n + 64, F32)
        self.g, self.a = self.buf.ctypes.data, self.buf.ctypes.data + 4 * (n + 32)

    def code(self, g=0, a=0, n=None, k=0, steps=4, inv=None, null=()):
        inv = float(A.inv_steps(steps)) if inv is None and 1 <= steps <= 65536 else (0.25 if inv is None else inv)
        gp = None if 'g' in null else self.g + g
        ap = None if 'a' in null else self.a + a
        return L.lib().rd_grad_accum(gp, ap, self.n if n is None else n, k, steps, inv, None)


def test_every_refusal_code_comes_back_before_a_launch():
    r = HostRig()
    assert r.code(null=('g',)) == -1 and r.code(null=('a',)) == -1 and r.code(null=('g', 'a')) == -1
    for off in (1, 2, 3):
        assert r.code(g=off) == -2 and r.code(a=off) == -2, off
    assert r.code(n=0) == -3 and r.code(n=-5) == -3 and r.code(n=(1 << 40) + 1) == -3
    assert r.code(steps=0) == -4 and r.code(steps=-2) == -4 and r.code(steps=65537) == -4
    assert r.code(k=-1) == -5 and r.code(k=4) == -5 and r.code(k=5) == -5 and r.code(steps=1, k=1) == -5
    # inv_steps: the bits of (float)(1.0 / steps) and nothing else -- the neighbours, the negative, 0, NaN, 1 / another N
    inv3 = A.inv_steps(3)
    for bad in (np.nextafter(inv3, F32(1)), np.nextafter(inv3, F32(0)), -inv3, F32(0), F32('nan'), A.inv_steps(2), F32(1)):
        assert r.code(steps=3, inv=float(bad)) == -6, bad
    assert r.code(steps=65536, inv=float(np.nextafter(A.inv_steps(65536), F32(1)))) == -6
    # overlap: the same arena, a shifted copy of it, the last word of one on the first of the other
    n = r.n
    assert L.lib().rd_grad_accum(r.g, r.g, n, 0, 4, 0.25, None) == -7
    assert L.lib().rd_grad_accum(r.g, r.g + 4, n - 1, 0, 4, 0.25, None) == -7
    assert L.lib().rd_grad_accum(r.g + 4, r.g, n - 1, 0, 4, 0.25, None) == -7
    assert L.lib().rd_grad_accum(r.g, r.g + 4 * (n - 1), n, 0, 4, 0.25, None) == -7
    assert L.lib().rd_grad_accum(r.g + 4 * (n - 1), r.g, n, 0, 4, 0.25, None) == -7
    # the order of the checks: the first that applies
    assert r.code(null=('g',), a=1, n=0, steps=0) == -1 and r.code(g=2, n=0, steps=0) == -2 and r.code(n=0, steps=0) == -3
    assert r.code(steps=0, k=-1) == -4 and r.code(k=9, inv=0.3) == -5
    # steps == 1: accepted, nothing launched (a launch on these host arrays without a device would not return 0)
    assert r.code(steps=1, k=0, inv=1.0) == 0
    # arrays that touch without overlapping are accepted by the checks in front of the launch: shown through steps == 1
    assert L.lib().rd_grad_accum(r.g, r.g + 4 * n, n, 0, 1, 1.0, None) == 0
    assert not r.buf.any()


def test_check_steps_and_inv_steps():
    for bad in (0, -1, 65537, 2.5, True, float('nan')):
        with pytest.raises((ValueError, OverflowError)):
            A.check_steps(bad)
    assert A.check_steps(1) == 1 and A.check_steps(65536) == 65536 and A.check_steps(4.0) == 4
    for n in (1, 2, 3, 4, 7, 10, 65536):
        assert _bits(A.inv_steps(n)) == _bits(_round_f32(Fraction(1, n))), n
    assert float(A.inv_steps(2)) == 0.5 and float(A.inv_steps(4)) == 0.25 and float(A.inv_steps(3)) != 1 / 3


# ------------------------------------------------------------------------------------------------------------- the model
def _by_hand(rows):
    """One element of a window in exact rational arithmetic, each operation rounded to float32 on its own: the copy, N - 2 sums,
    the last sum, the product with the float32 of 1 / N."""
    n = len(rows)
    acc = _fr(rows[0])
    for g in rows[1:-1]:
        acc = _fr(_round_f32(acc + _fr(g)))
    s = _fr(_round_f32(acc + _fr(rows[-1])))
    return _round_f32(s * _fr(_round_f32(Fraction(1, n))))


ROWS = {
    2: [(1.0, 3.0), (0.1, 0.2), (1.0, 2.0 ** -24), (1.0, 3 * 2.0 ** -24), (-5.5, 5.5), (1e-3, -7.25), (16777216.0, 1.0)],
    3: [(1.0, 1.0, 1.0), (0.1, 0.1, 0.1), (1.0, 2.0, 3.0), (1e8, 1.0, -1e8), (0.3, -0.7, 1.9), (2.0 ** -20, 1.0, 2.0 ** -24)],
    4: [(1.0, 2.0, 3.0, 4.0), (0.1, 0.2, 0.3, 0.4), (1e-5, 1e5, -1e5, 3.0), (7.0, -7.0, 7.0, -7.0)],
    7: [(1.0,) * 7, (0.1,) * 7, (1.0, -2.0, 3.0, -4.0, 5.0, -6.0, 7.0), (1e-3, 1e3, 2e-3, 2e3, 3e-3, 3e3, 0.5)],
}


@pytest.mark.parametrize('n', [2, 3, 4, 7])
def test_model_equals_rows_worked_out_in_exact_rational_arithmetic(n):
    rows = [tuple(float(F32(v)) for v in r) for r in ROWS[n]]
    grads = [np.array([r[k] for r in rows], F32) for k in range(n)]
    got = A.model(grads)
    want = np.array([_by_hand(r) for r in rows], F32)
    assert got.dtype == F32 and np.array_equal(_bits(got), _bits(want)), (got, want)
    # launch by launch: the copy is the first gradient's bits, the sums are the running sum rounded at every step
    states = A.window(grads)
    assert len(states) == n and np.array_equal(_bits(states[0]), _bits(grads[0])) and np.array_equal(_bits(states[-1]), _bits(got))
    for k in range(1, n - 1):
        by_hand = [_round_f32(_fr(a) + _fr(g)) for a, g in zip(states[k - 1], grads[k])]
        assert np.array_equal(_bits(states[k]), _bits(by_hand)), k
    assert not any(s is g for s in states for g in grads)       # copies: the inputs are not aliased
    g = A.GradAccum(_fake_trainer(), n)
    assert np.array_equal(_bits(g.model(grads)), _bits(got))
    with pytest.raises(ValueError, match='%d gradients for a window of %d' % (n + 1, n)):
        g.model(grads + [grads[0]])


def test_the_mean_is_not_the_correctly_rounded_mean():
    """(a + b) * inv is two roundings and the rounding of inv: three times float32(0.1) has the mean float32(0.1) exactly, and the
    window gives its upper neighbour.  N = 2: inv = 0.5 is exact, so the one rounding is the sum's -- 16777216 + 1 is a tie that goes
    to even and the half of it is 8388608, where the mean 8388608.5 is a float32."""
    tenth = F32(0.1)
    got = A.model([np.array([tenth])] * 3)[0]
    exact = (_fr(tenth) * 3) / 3
    assert _round_f32(exact) == tenth and got == np.nextafter(tenth, F32(1)) and got == _by_hand((tenth,) * 3)
    got = A.model([np.array([16777216.0], F32), np.array([1.0], F32)])[0]
    assert got == F32(8388608.0) and _round_f32(Fraction(16777217, 2)) == F32(8388608.5)


def test_model_nan_inf_rows_and_the_copy_keeps_a_nan_payload():
    nan, inf = F32('nan'), F32('inf')
    rows = [(nan, 1.0, 2.0), (1.0, nan, 2.0), (1.0, 2.0, nan), (inf, 1.0, 2.0), (1.0, -inf, 2.0), (inf, -inf, 1.0), (inf, 1.0, -inf),
            (inf, inf, inf), (3e38, 3e38, 1.0), (-3e38, -3e38, -3e38)]
    grads = [np.array([r[k] for r in rows], F32) for k in range(3)]
    got = A.model(grads)
    assert np.isnan(got[[0, 1, 2, 5, 6]]).all()
    assert got[3] == inf and got[4] == -inf and got[7] == inf
    assert got[8] == inf and got[9] == -inf                     # the sum overflows: what the arithmetic gives, not a clamped mean
    # the copy (k == 0) is a word copy: a signalling NaN with a payload, -0 and a denormal arrive with their bits
    words = np.array([0x7FA00001, 0xFFC12345, 0x80000000, 0x00000001, 0x7F800000], np.uint32)
    states = A.window([words.view(F32), np.ones(5, F32), np.ones(5, F32)])
    assert np.array_equal(states[0].view(np.uint32), words)
    assert np.isnan(states[1][:2]).all() and np.isnan(states[2][:2]).all() and states[2][4] == inf
    # N == 1: the gradient itself
    one = A.window([words.view(F32)])
    assert len(one) == 1 and np.array_equal(one[0].view(np.uint32), words) and one[0] is not words


@pytest.mark.parametrize('n', [2, 3, 4, 7, 16])
def test_model_is_within_gamma_of_the_float64_mean(n):
    """|model - mean| <= gamma(N + 1) * sum_k |g_k| / N with gamma(m) = m u / (1 - m u), u = 2^-24.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 / 4.2).  Every float32 operation on operands away
    from underflow and overflow returns the exact result times (1 + d), |d| <= u.  The window computes
        s = (...((g_0 + g_1)(1 + d_1) + g_2)(1 + d_2) ... + g_{N-1})(1 + d_{N-1}),
    so g_k carries at most N - 1 factors (1 + d_i); inv = (1 / N)(1 + d_inv) is the rounding of the reciprocal; the product adds
    (1 + d_p).  The result is sum_k (g_k / N) * prod_{i <= N + 1} (1 + d_i), and |prod - 1| <= gamma(N + 1) (Lemma 3.1), which gives
    the bound.  N - 1 additions, the rounding of inv and one product: N + 1 roundings.  The inputs are 2^-10 <= |g| <= 2^10 of both
    signs, so no intermediate comes near a subnormal or the overflow threshold; an exact cancellation to 0 is exact.  The float64
    mean carries an error of its own of at most (N + 1) 2^-53 relative to the same sum of magnitudes, which is added to the bound."""
    rng = np.random.RandomState(n)
    m = 20000
    grads = [(rng.choice([-1.0, 1.0], m) * 2.0 ** rng.uniform(-10, 10, m)).astype(F32) for _ in range(n)]
    got = A.model(grads).astype(np.float64)
    g64 = np.stack([g.astype(np.float64) for g in grads])
    mean, mag = g64.sum(0) / n, np.abs(g64).sum(0) / n
    u = 2.0 ** -24
    gamma = (n + 1) * u / (1 - (n + 1) * u)
    bound = gamma * mag + (n + 1) * 2.0 ** -53 * mag
    err = np.abs(got - mean)
    print('N = %d: max error / bound = %.3f' % (n, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())
    assert float((err / bound).max()) > 0.01                    # the bound is of the error's order, not a formality


# ------------------------------------------------------------------------------------------------------------- counting
@pytest.mark.parametrize('per_epoch,epochs,steps,updates,trailing', [
    (5, 4, 1, 20, 0), (5, 4, 2, 10, 0), (5, 4, 3, 6, 2), (5, 2, 2, 5, 0), (5, 2, 3, 3, 1), (5, 1, 2, 2, 1),       # the Fundus tree
    (3, 4, 1, 12, 0), (3, 4, 2, 6, 0), (3, 4, 3, 4, 0), (3, 2, 2, 3, 0), (3, 1, 2, 1, 1), (3, 4, 5, 2, 2)])       # the Prostate tree
def test_update_count_and_trailing_remainder_of_the_test_trees(per_epoch, epochs, steps, updates, trailing):
    T = _train_module()
    assert A.updates_of(per_epoch * epochs, steps) == (updates, trailing)
    a = T.parse_args(BASE_ARGS + ['--accum_steps', str(steps), '--epochs', str(epochs)])
    assert T.accum_totals(a, per_epoch) == (updates, per_epoch * epochs, trailing)
    line = T.accum_line(steps, updates, per_epoch * epochs, trailing)
    assert line.startswith('accum: %d micro-batches per update: %d updates over %d iterations, %d trailing iteration'
                           % (steps, updates, per_epoch * epochs, trailing))
    assert line.endswith('s are not applied' if trailing != 1 else ' is not applied')


def test_a_run_with_no_complete_window_is_refused():
    T = _train_module()
    a = T.parse_args(BASE_ARGS + ['--accum_steps', '7', '--epochs', '2'])
    with pytest.raises(ValueError, match=r'--accum_steps 7: the 6 iterations of this run complete no window'):
        T.accum_totals(a, 3)
    assert T.accum_totals(a, 4) == (1, 8, 1)
    # without the flag the count is the loop's, whatever it is
    assert T.accum_totals(T.parse_args(BASE_ARGS + ['--epochs', '0']), 5) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- flags
BASE_ARGS = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
REFUSALS = [
    (['--accum_steps', '0'], {}, '--accum_steps takes a number of micro-batches per update, got 0'),
    (['--accum_steps', '-3'], {}, '--accum_steps takes a number of micro-batches per update, got -3'),
    (['--accum_steps', '65537'], {}, '--accum_steps takes at most 65536'),
    (['--accum_steps', '2', '--norm', 'gn'], {}, '--norm gn trains through the modules'),
    (['--accum_steps', '2', '--norm', 'in'], {}, '--norm in trains through the modules'),
    (['--accum_steps', '2'], {'WORLD_SIZE': '2'}, r'--accum_steps runs in one process.*WORLD_SIZE=2'),
    (['--accum_steps', '2', '--tb_every_iter'], {}, '--accum_steps does not go with --tb_every_iter / --tb_health'),
    (['--accum_steps', '4', '--tb_health'], {}, '--accum_steps does not go with --tb_every_iter / --tb_health'),
]


def test_parse_default_uses_accum_and_help(capsys):
    T = _train_module()
    a = T.parse_args(BASE_ARGS)
    assert a.accum_steps == 1 and not T.uses_accum(a)
    spelled = T.parse_args(BASE_ARGS + ['--accum_steps', '1'])
    assert not T.uses_accum(spelled)
    for world in (1, 8):
        T.check_args(spelled, world)                            # N = 1 refuses nothing: data parallel, the ring, --norm gn
    T.check_args(T.parse_args(BASE_ARGS + ['--accum_steps', '1', '--norm', 'gn']), 1)
    T.check_args(T.parse_args(BASE_ARGS + ['--accum_steps', '1', '--tb_every_iter', '--tb_health']), 1)
    a = T.parse_args(BASE_ARGS + ['--accum_steps', '2', '--clip_grad_norm', '1', '--avg_weights', 'uniform', '--ckpt_every', '1',
                                  '--weight_decay', '0.01', '--lr_schedule', 'cosine', '--warmup_iters', '3', '--tb_images'])
    T.check_args(a, 1)
    assert T.uses_accum(a) and a.accum_steps == 2
    T.check_args(T.parse_args(BASE_ARGS + ['--accum_steps', '65536']), 1)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--accum_steps N' in text and 'mean of the N micro-batch gradients' in text
    assert "current micro-batch's losses and the last update's lr" in text and 'count updates' in text


@pytest.mark.parametrize('flags,env,match', REFUSALS)
def test_check_args_refusals_directly_and_through_main(flags, env, match, monkeypatch):
    T = _train_module()
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match=match):
        T.check_args(T.parse_args(BASE_ARGS + flags), int(env.get('WORLD_SIZE', '1')))
    # main() refuses before it touches the data root (which does not exist), a process group or the GPU
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: pytest.fail('a GPU call was made'))
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(BASE_ARGS + flags))


# ------------------------------------------------------------------------------------------------------------- the host object
def test_grad_accum_over_a_cpu_bank_ranges_settings_and_position():
    tr = _fake_trainer()
    g = A.GradAccum(tr, 3)
    assert g.settings() == dict(steps=3) and float(g.inv) == float(F32(1.0 / 3))
    (name, acc), = g.named_ranges()
    assert name == 'accum/arena' and acc is g.acc and name.startswith(CK.ACCUM_PREFIX)
    assert acc.shape == tr.bank.grads.shape and acc.dtype == torch.float32 and acc.data_ptr() != tr.bank.grads.data_ptr() and not acc.any()
    # the window position is host state
    assert g.position() == 0 and not g.next_is_boundary()
    g.set_position(2)
    assert g.position() == 2 and g.next_is_boundary()
    for bad in (-1, 3, 7):
        with pytest.raises(ValueError, match='position'):
            g.set_position(bad)
    assert A.GradAccum(tr, 2).next_is_boundary() is False
    for bad in (0, -2, 65537):
        with pytest.raises(ValueError, match='grad accum: steps'):
            A.GradAccum(tr, bad)


# ------------------------------------------------------------------------------------------------------------- the state file
def _accum_state(tr, g, micro):
    """(_fake_state takes an object with named_ranges(): the accumulator is one)"""
    return _fake_state(tr, g, dict(epoch=1, iter_num=5, previous_best=12.5, grad_accum=dict(g.settings(), micro=micro)))


def test_resume_refusals_name_grad_accum(tmp_path):
    tr = _fake_trainer()
    g2 = A.GradAccum(tr, 2)
    g2.acc.copy_(torch.arange(g2.acc.numel(), dtype=torch.float32))
    plain, with2 = _fake_state(tr), _accum_state(tr, g2, 1)
    names = [e['name'] for e in with2['table']]
    assert names[:-1] == [e['name'] for e in plain['table']] and names[-1] == 'accum/arena' and 'grad_accum' not in plain['meta']
    path = str(tmp_path / 'last_state.pth')
    CK.write_file(path, with2)
    back = CK.load_file(path)
    assert back['meta']['grad_accum'] == dict(steps=2, micro=1)
    assert torch.equal(CK.range_tensor(back, 'accum/arena'), g2.acc)
    assert CK.compare_grad_accum(back, g2.settings()) == 1      # the same N: the position to continue at
    assert CK.compare_grad_accum(plain, None) == 0              # neither side has a record: N = 1
    with pytest.raises(ValueError, match=r'grad_accum steps = 2, this run has 3'):
        CK.compare_grad_accum(back, dict(steps=3))
    with pytest.raises(ValueError, match=r'grad_accum steps = 2, this run has 1'):
        CK.compare_grad_accum(back, None)                       # the file has a record, the run has no flag
    with pytest.raises(ValueError, match=r'grad_accum steps = 1, this run has 2'):
        CK.compare_grad_accum(plain, g2.settings())             # a record-less file under --accum_steps 2
    # a record and a range table that contradict one another
    lying = _fake_state(tr, None, dict(epoch=1, iter_num=5, previous_best=0.0, grad_accum=dict(steps=2, micro=0)))
    with pytest.raises(ValueError, match='grad_accum steps = 2 but holds no accumulator arena'):
        CK.compare_grad_accum(lying, g2.settings())
    orphan = _fake_state(tr, g2)
    with pytest.raises(ValueError, match='grad_accum steps = 1 but holds an accumulator arena'):
        CK.compare_grad_accum(orphan, None)
    with pytest.raises(ValueError, match='grad_accum micro = 2 in a window of 2'):
        CK.compare_grad_accum(_accum_state(tr, g2, 2), g2.settings())
    # the other records do not see it
    CK.compare_avg_weights(back, None)
    CK.compare_grad_guard(back, None)
    CK.compare_optim(back, None)
