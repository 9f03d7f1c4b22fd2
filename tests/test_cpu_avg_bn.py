"""CPU tests of the BatchNorm re-estimation of the averaged model (train.py --avg_bn_recal, ramdsir/avg_bn.py, rd_bn_recal): the site
record has one layout in C and ctypes, the numpy model of the kernel equals rows worked out in exact rational arithmetic and agrees
with nn.BatchNorm2d(momentum=None), every validation code is returned before a launch, the flag refuses what it cannot do, and the
re-estimation plan is the forward list of a module in training mode with null running-statistics pointers.  Nothing is launched."""
import ctypes as C
import math
import os
import subprocess
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))

from ramdsir import _lib as L           # noqa: E402
from ramdsir import avg_bn as AB        # noqa: E402
from ramdsir import ckpt as CK          # noqa: E402
from ramdsir import engine as E         # noqa: E402

MODS = [('enc', E.encoder_specs(3, 16)), ('dec', E.decoder_specs(16, 2))]
SLOTS = L.STAT_SLOTS


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_site_record_has_one_layout_in_c_and_ctypes_and_the_symbol_is_exported(tmp_path):
    fields = ('stats', 'conv_bias', 'running_mean', 'running_var', 'num_batches_tracked', 'count', 'C', 'nslots', 'pad_')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%zu %d", sizeof(rd_bn_recal_site_t), '
           'RD_BN_RECAL_MAX_SITES);' + ''.join('printf(" %%zu", offsetof(rd_bn_recal_site_t, %s));' % f for f in fields) + 'return 0;}')
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    assert out[0] == C.sizeof(L.RdBnRecalSite) == 56 and out[1] == L.BN_RECAL_MAX_SITES == 4096
    assert out[2:] == [getattr(L.RdBnRecalSite, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert 'rd_bn_recal' in L.exported_symbols() and hasattr(C.CDLL(L.LIB_PATH), 'rd_bn_recal')
    fn = L.lib().rd_bn_recal
    assert fn.restype is C.c_int and len(fn.argtypes) == 7


# ------------------------------------------------------------------------------------------------------------- exact rows
def _rn(x, p):
    """The rational x rounded to the nearest number with a p-bit significand, ties to even (no underflow / overflow: the rows stay in
    the normal range)."""
    x = Fr(x)
    if x == 0:
        return x
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    assert Fr(2) ** e <= a < Fr(2) ** (e + 1)
    q = a / Fr(2) ** (e - p + 1)
    n, r = divmod(q.numerator, q.denominator)
    twice = 2 * r
    if twice > q.denominator or (twice == q.denominator and n % 2):
        n += 1
    return s * n * Fr(2) ** (e - p + 1)


r32 = lambda x: _rn(x, 24)      # noqa: E731
r64 = lambda x: _rn(x, 53)      # noqa: E731


def _exact_stat(s1, s2, count, cb):
    """csrc/bn_fin.h fwd_stat in rationals, every operation rounded where the kernel rounds it: (mean, unb)."""
    cnt = Fr(count)
    m0 = r64(Fr(s1) / cnt)
    vard = r64(r64(Fr(s2) / cnt) - r64(m0 * m0))
    if vard < 0:
        vard = Fr(0)
    mean = r32(r64(m0 + Fr(cb)))
    unb = r32(r64(r64(vard * cnt) / (cnt - 1))) if cnt > 1 else r32(vard)
    return mean, unb


def _exact_update(run, x, k):
    if k == 0:
        return Fr(x)
    w = r32(Fr(1) / r32(Fr(k + 1)))
    d = r32(Fr(x) - Fr(run))
    t = r32(w * d)
    return r32(Fr(run) + t)


def _fma_update(run, x, k):
    """What run + w * d as ONE fused operation would give: the form the kernel must not take."""
    w = r32(Fr(1) / r32(Fr(k + 1)))
    return r32(Fr(run) + w * r32(Fr(x) - Fr(run)))


def _slots_of(s1, s2, Cc=1, spread=1):
    """Statistic slots that hold (s1, s2) in `spread` equal parts (spread 1: the sums are exactly s1 and s2)."""
    sl = np.zeros((SLOTS, Cc, 2), np.float64)
    for j in range(spread):
        sl[j * 7 % SLOTS, :, 0] += np.float64(s1) / spread
        sl[j * 7 % SLOTS, :, 1] += np.float64(s2) / spread
    return sl


def _exact_sums(sl, nslots=SLOTS):
    """csrc/bn_fin.h slot_sums in rationals: the copies added one after the other in slot order, each sum rounded to float64."""
    s1, s2 = Fr(0), Fr(0)
    for k in range(nslots):
        s1, s2 = r64(s1 + Fr(float(sl[k, 0, 0]))), r64(s2 + Fr(float(sl[k, 0, 1])))
    return s1, s2


ROWS = [
    # (s1, s2, count, conv_bias or None, k, old mean, old var)
    (10.0, 37.5, 4.0, None, 0, float('nan'), float('nan')),             # k = 0 ignores the old value
    (10.0, 37.5, 4.0, 0.125, 0, float('nan'), 3.0),
    (7.0, 19.0, 3.0, None, 1, 0.1, 0.7),                                # k = 1, 2
    (7.0, 19.0, 3.0, -0.3, 2, 0.1, 0.7),
    (123.456, 9876.5, 16384.0, 0.01, 10 ** 6, -0.3333, 2.0001),         # k = 10^6: w = 1 / 1000001 rounded
    (5.0, 25.0, 1.0, None, 1, 0.25, 0.5),                               # count = 1: unb = var (= 0 here)
    (5.0, 26.5, 1.0, 1.5, 2, 0.25, 0.5),                                # count = 1, var = 1.5
    (3.0, 2.9999999, 3.0, None, 1, 0.5, 0.25),                          # s2 / n - m^2 < 0: clamped to 0
    (3.0, 2.9999999, 3.0, 2.0, 3, 0.5, 0.25),
]


@pytest.mark.parametrize('row', ROWS)
def test_model_equals_exact_rational_arithmetic(row):
    s1, s2, count, cb, k, om, ov = row
    f32 = np.float32
    s1, s2 = np.float64(s1), np.float64(s2)
    cbv = None if cb is None else np.array([f32(cb)], f32)
    for spread in (8, 1):
        sl = _slots_of(s1, s2, 1, spread)
        e1, e2 = _exact_sums(sl)
        assert spread > 1 or (e1, e2) == (Fr(float(s1)), Fr(float(s2)))
        rm, rv, nbt = AB.model(np.array([om], f32), np.array([ov], f32), sl, count, cbv, k)
        mean, unb = _exact_stat(e1, e2, Fr(count), Fr(float(f32(cb))) if cb is not None else Fr(0))
        want_m = _exact_update(Fr(float(f32(om))) if k else None, mean, k)
        want_v = _exact_update(Fr(float(f32(ov))) if k else None, unb, k)
        assert rm.dtype == rv.dtype == f32 and nbt == k + 1 and nbt.dtype == np.int64
        assert Fr(float(rm[0])) == want_m and Fr(float(rv[0])) == want_v, (row, float(rm[0]), float(want_m), float(rv[0]), float(want_v))
    if count == 1.0:
        assert unb == r32(max(Fr(float(s2)) - Fr(float(s1)) ** 2, 0))
    if s2 < s1 * s1 / count:
        assert unb == 0


def test_conv_bias_null_equals_a_zero_bias_and_shifts_only_the_mean():
    f32 = np.float32
    rng = np.random.RandomState(3)
    Cc = 17
    sl = rng.uniform(0.5, 2.0, (SLOTS, Cc, 2))
    sl[:, :, 1] += 40.0
    old = rng.normal(size=(2, Cc)).astype(f32)
    a = AB.model(old[0], old[1], sl, 48.0, None, 3)
    z = AB.model(old[0], old[1], sl, 48.0, np.zeros(Cc, f32), 3)
    b = AB.model(old[0], old[1], sl, 48.0, np.full(Cc, 0.75, f32), 3)
    assert a[0].tobytes() == z[0].tobytes() and a[1].tobytes() == z[1].tobytes()
    assert b[1].tobytes() == a[1].tobytes() and not np.array_equal(b[0], a[0])
    # nslots: the copies behind the first `nslots` are not read
    junk, zeros = sl.copy(), sl.copy()
    junk[8:], zeros[8:] = 1e30, 0.0
    for i in (0, 1):
        assert AB.model(old[0], old[1], junk, 48.0, None, 3, nslots=8)[i].tobytes() == AB.model(old[0], old[1], zeros, 48.0, None, 3)[i].tobytes()


def test_the_update_is_three_roundings_not_an_fma():
    """A row where run + w * d as one fused operation differs from the three separately rounded operations: the model (and, bit for
    bit with it, the kernel) gives the latter."""
    f32 = np.float32
    rng = np.random.RandomState(11)
    found = 0
    for _ in range(400):
        run, x = f32(rng.normal()), f32(rng.normal())
        k = int(rng.randint(1, 50))
        three, fused = _exact_update(Fr(float(run)), Fr(float(x)), k), _fma_update(Fr(float(run)), Fr(float(x)), k)
        got = AB.update_model(np.array([run], f32), np.array([x], f32), k)
        assert Fr(float(got[0])) == three
        found += three != fused
    assert found > 0


# ------------------------------------------------------------------------------------------------------------- against torch
@pytest.mark.parametrize('K', [1, 5, 32])
@pytest.mark.parametrize('with_bias', [False, True])
def test_model_iterated_agrees_with_batchnorm_momentum_none(K, with_bias):
    """model() over K batches against nn.BatchNorm2d(C, momentum=None) in training mode on the CPU (update_bn's semantics), fed the
    tensors whose sums produced the slots.  The inputs are multiples of 2^-10 of magnitude < 8, so z + bias is exact in float32 and the
    slot sums are exact in float64: both sides see the same data.

    Tolerance, from float32 rounding (u = 2^-24), per channel, to first order.  Exact values: x_k the batch mean resp. unbiased batch
    variance, R_K = (1 / K) sum_k x_k.  Let A = max_k |x_k| (every running value is a convex combination of the x_k, so |.| <= A) and
    n = N H W.
      model: the batch value is the correctly rounded float32 of a float64 expression: <= u A (the float64 part, including the
        cancellation in s2 / n - m^2, is <= 8 * 2^-53 (s2 / n + m^2) n / (n - 1) =: c64).  One update rounds d = x - r (|d| <= 2 A:
        2 u A, scaled by w), w itself (u w |d|), t = w d (u w |d|) and r + t (u A): <= u A (1 + 6 / (k + 1)).  An error already in r is
        scaled by 1 - w <= 1.  Over the K batches: <= u A (K + 6 (1 + ln K)) + u A + c64.
      torch: running = (1 - f) running + f x with f = 1 / k rounds f, 1 - f, two products and the sum: <= u A (3 + 2 / k) per batch,
        <= u A (3 K + 2 (1 + ln K)) in all; its batch mean is a float32 or wider sum of n terms of mean magnitude S1 = mean |x|:
        <= u (4 + log2 n) S1, its batch variance a sum of n non-negative terms: <= u (4 + log2 n) x_k.
    The two results lie within the sum of the two bounds."""
    f32 = np.float32
    rng = np.random.RandomState(100 + K)
    Cc, N, H, W = 5, 3, 4, 6
    n = N * H * W
    bias = (rng.randint(-2048, 2048, Cc) / 1024.0).astype(f32) if with_bias else None
    bn = torch.nn.BatchNorm2d(Cc, momentum=None).train()
    rm, rv = np.full(Cc, np.nan, f32), np.full(Cc, np.nan, f32)
    A_m, A_v, S1, c64 = np.zeros(Cc), np.zeros(Cc), np.zeros(Cc), np.zeros(Cc)
    exact_m, exact_v = np.zeros(Cc), np.zeros(Cc)
    for k in range(K):
        z = (rng.randint(-4096, 4096, (N, Cc, H, W)) / 1024.0).astype(f32) * (1 + np.arange(Cc, dtype=f32))[None, :, None, None] / 4
        x = z if bias is None else (z + bias[None, :, None, None]).astype(f32)
        assert bias is None or np.array_equal(x.astype(np.float64), z.astype(np.float64) + bias.astype(np.float64)[None, :, None, None])
        with torch.no_grad():
            bn(torch.from_numpy(x))
        # the slots: image i, row y go to slot (i * H + y): sums of z (the conv's sums exclude its bias)
        sl = np.zeros((SLOTS, Cc, 2), np.float64)
        z64 = z.astype(np.float64)
        for i in range(N):
            for y in range(H):
                sl[i * H + y, :, 0] = z64[i, :, y].sum(-1)
                sl[i * H + y, :, 1] = (z64[i, :, y] ** 2).sum(-1)
        rm, rv, nbt = AB.model(rm, rv, sl, float(n), bias, k)
        x64 = x.astype(np.float64)
        m = x64.mean((0, 2, 3))
        v = x64.var((0, 2, 3), ddof=1)
        exact_m += m / K
        exact_v += v / K
        A_m, A_v = np.maximum(A_m, np.abs(m)), np.maximum(A_v, v)
        S1 = np.maximum(S1, np.abs(x64).mean((0, 2, 3)))
        c64 = np.maximum(c64, 8 * 2.0 ** -53 * ((z64 ** 2).mean((0, 2, 3)) + z64.mean((0, 2, 3)) ** 2) * n / (n - 1))
    assert int(nbt) == K == int(bn.num_batches_tracked)
    u, lnK, lg = 2.0 ** -24, 1 + math.log(K), 4 + math.log2(n)
    for got, ref, exact, A, S in ((rm, bn.running_mean.numpy(), exact_m, A_m, S1), (rv, bn.running_var.numpy(), exact_v, A_v, A_v)):
        ours = u * A * (K + 6 * lnK) + u * A + c64
        theirs = u * A * (3 * K + 2 * lnK) + u * lg * S
        assert (np.abs(got - exact) <= ours).all(), (np.abs(got - exact) / ours).max()
        assert (np.abs(got - ref) <= ours + theirs).all(), (np.abs(got - ref) / (ours + theirs)).max()


# ------------------------------------------------------------------------------------------------------------- validation codes
def _site(**kw):
    """A table of one valid-looking site (the pointers are never dereferenced: every call below is refused before the launch)."""
    arr = (L.RdBnRecalSite * 1)()
    s = arr[0]
    s.stats, s.conv_bias, s.running_mean, s.running_var, s.num_batches_tracked = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    s.count, s.C, s.nslots = 16.0, 16, 64
    for k, v in kw.items():
        setattr(s, k, v)
    return arr


@pytest.mark.parametrize('code,call', [
    (-1, dict(host=False)), (-1, dict(dev=None)), (-1, dict(n=0)), (-1, dict(n=L.BN_RECAL_MAX_SITES + 1)), (-1, dict(max_c=0)),
    (-2, dict(k=-1)),
    (-3, dict(site=dict(stats=None))), (-3, dict(site=dict(running_mean=None))), (-3, dict(site=dict(running_var=None))),
    (-3, dict(site=dict(num_batches_tracked=None))), (-3, dict(site=dict(stats=0x10008))), (-3, dict(site=dict(running_var=0x40002))),
    (-3, dict(site=dict(num_batches_tracked=0x50004))),
    (-4, dict(site=dict(C=0))), (-4, dict(site=dict(C=17))),
    (-5, dict(site=dict(count=0.0))), (-5, dict(site=dict(count=0.5))), (-5, dict(site=dict(count=float('nan')))),
    (-6, dict(site=dict(nslots=0))), (-6, dict(site=dict(nslots=12))), (-6, dict(site=dict(nslots=72))), (-6, dict(site=dict(nslots=-8))),
    (-7, dict(eps=-1e-5)), (-7, dict(eps=float('nan'))),
])
def test_every_validation_code_is_returned_before_a_launch(code, call):
    arr = _site(**call.get('site', {}))
    host = arr if call.get('host', True) else None
    dev = call.get('dev', 0x60000)
    got = L.lib().rd_bn_recal(host, dev, call.get('n', 1), call.get('max_c', 16), call.get('k', 0), call.get('eps', 1e-5), None)
    assert got == code


# ------------------------------------------------------------------------------------------------------------- the flag
BASE = ['--save_path', 'unused', '--ram', '--rec']


def _train():
    import train
    return train


@pytest.mark.parametrize('extra,match', [
    (['--avg_bn_recal', '2'], 'needs --avg_weights'),
    (['--avg_bn_recal', '2', '--avg_weights', 'uniform', '--norm', 'gn'], '--norm gn'),
    (['--avg_bn_recal', '-1', '--avg_weights', 'ema'], 'number of batches'),
    (['--avg_bn_recal', '-3'], 'number of batches'),
])
def test_flag_refusals_directly_and_through_main(extra, match):
    T = _train()
    with pytest.raises(ValueError, match=match):
        T.check_args(T.parse_args(BASE + extra), 1)
    with pytest.raises(ValueError, match=match):
        T.main(T.parse_args(BASE + extra))                   # check_args is main()'s first statement: no GPU call, no file


def test_k_beyond_the_epoch_is_refused_directly_and_through_main(tmp_path, monkeypatch):
    T = _train()
    args = T.parse_args(['--save_path', str(tmp_path / 'out'), '--ram', '--rec', '--avg_weights', 'uniform', '--avg_bn_recal', '4'])
    T.check_args(args, 1)
    T.check_bn_recal(args, 4)
    with pytest.raises(ValueError, match='--avg_bn_recal 4 is more than the 3 iterations of an epoch'):
        T.check_bn_recal(args, 3)
    T.check_bn_recal(T.parse_args(BASE), 0)                  # off: any length
    # through main(): the length is known behind the loaders' construction; nothing of the GPU has been touched there

    def no_gpu(*a, **k):
        raise AssertionError('reached the trainer')
    monkeypatch.setattr(T, 'Validation', lambda *a, **k: None)
    monkeypatch.setattr(T, 'init_process', lambda world, local: None)
    monkeypatch.setattr(T, 'make_loaders', lambda *a, **k: ([], [], [], 3))
    monkeypatch.setattr(T, 'build_trainer', no_gpu)
    with pytest.raises(ValueError, match='more than the 3 iterations'):
        T.main(args)


def test_defaults_and_help():
    T = _train()
    a = T.parse_args(BASE)
    assert a.avg_bn_recal == 0 and not T.uses_bn_recal(a)
    assert T.uses_bn_recal(T.parse_args(BASE + ['--avg_bn_recal', '3']))
    T.check_args(T.parse_args(BASE + ['--avg_bn_recal', '0']), 1)           # spelled out: the flag left away


def test_a_captured_graph_and_a_missing_average_are_refused():
    from ramdsir.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr._graphs, tr._avg, tr._bn_recal, tr._bn_capture = True, None, None, False
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.enable_avg_bn_recal(2)
    with pytest.raises(RuntimeError, match='hipGraph'):
        tr.arm_bn_capture()
    tr._graphs = False
    with pytest.raises(RuntimeError, match='enable_avg_weights first'):
        tr.enable_avg_bn_recal(2)
    with pytest.raises(RuntimeError, match='enable_avg_bn_recal'):
        tr.arm_bn_capture()
    with pytest.raises(ValueError):
        tr.enable_avg_bn_recal(-1)
    assert tr.enable_avg_bn_recal(0) is None and tr._bn_recal is None


def _state(bn_recal):
    saved = dict(mode='uniform', decay=None, start=0)
    if bn_recal is not None:
        saved['bn_recal'] = bn_recal
    return dict(meta=dict(avg_weights=saved), table=[dict(name='params'), dict(name='avg/params')])


def test_resume_refuses_a_file_and_a_run_that_disagree_about_k():
    cur = dict(mode='uniform', decay=None, start=0)
    CK.compare_avg_weights(_state(None), cur)
    CK.compare_avg_weights(_state(2), dict(cur, bn_recal=2))
    for saved, now in ((2, 3), (2, None), (None, 2)):
        with pytest.raises(ValueError, match='bn_recal'):
            CK.compare_avg_weights(_state(saved), cur if now is None else dict(cur, bn_recal=now))


# ------------------------------------------------------------------------------------------------------------- the plan
def _recal(dtype, N, H, W):
    bank = E.ParamBank(MODS, 'cpu')
    wpack = E.WeightPack(bank, MODS, dtype)
    return AB.build_plan(bank, wpack, dtype, N, H, W), bank


def _module_train_plans(dtype, N, H, W):
    """The training plans Encoder.forward and Decoder.forward build for this geometry (networks/unet.py: the Plan defaults)."""
    def plan(mods, graph):
        bank = E.ParamBank(mods, 'cpu')
        pl = E.Plan(bank, dtype, N, [0, N], slope=0.0, training=True)
        graph(pl)
        pl.build(E.WeightPack(bank, mods, dtype))
        return pl

    def enc(pl):
        pl.feats = E.build_encoder(pl, E.Act(pl, N, H, W, 3, name='input'), n=16, mname='enc')

    def dec(pl):
        ins = []
        for l in range(5):
            a = E.Act(pl, N, H >> l, W >> l, 16 << l, name='feat')
            a.needs_grad = True
            ins.append(a)
        pl.out = E.build_decoder(pl, ins, n=16, num_classes=2, mname='dec')
    return plan(MODS[:1], enc), plan(MODS[1:], dec)


def _route(p, dt):
    r = L.RdRoute()
    rc = L.lib().rd_conv_route(C.byref(p), dt, C.byref(r))
    return rc, r.kernel.decode().split('<')[0] if rc == 0 else None, list(r.grid), r.block, r.lds, list(r.iarg)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('geom', [(4, 32, 32), (5, 64, 64)])
def test_recal_plan_is_a_forward_list_with_null_running_pointers_on_the_module_routes(dtype, geom):
    from ramdsir import infer as I
    pl, bank = _recal(dtype, *geom)
    names = [op[0].__name__ for op in pl.fwd]
    assert set(names) == {'rd_conv', 'rd_pool_fwd', 'rd_up_stats', 'rd_bn_finalize_fwd'} and pl.bwd == []
    frozen = I.build_plan(bank, E.WeightPack(bank, MODS, dtype), dtype, *geom)
    assert len(pl.recal_sites) == len(frozen.bn_sites) == names.count('rd_bn_finalize_fwd') == 26 and pl.bn_sites == []
    assert names.count('rd_conv') == 27 and names.count('rd_pool_fwd') == 4
    N, H, W = geom
    fins = [op for op in pl.fwd if op[0].__name__ == 'rd_bn_finalize_fwd']
    for op, site in zip(fins, pl.recal_sites):
        d = op[1][0]._obj
        assert d.training == 1 and d.G == 1
        assert all(not d.running_mean[g] and not d.running_var[g] and not d.num_batches_tracked[g] for g in range(L.MAXG))
        stats, cbias, rm, rv, nbt, count, Cc, nslots, act = site
        assert stats == d.stats and cbias == d.conv_bias and count == d.count[0] and Cc == d.C and nslots == SLOTS
        assert count == N * (4 if act.up else 1) * act.H * act.W and (cbias is None) == bool(act.up)
        # the destinations are the bank's own buffers of that site
        assert rm.data_ptr() == act.norm.buf(0, 'running_mean').data_ptr() and nbt.dtype == torch.int64 and rv.shape == (Cc,)
    assert {s[6] for s in pl.recal_sites} == {16, 32, 64, 128, 256}
    # the same sites, in the same order, as the frozen plan's
    assert [s[2].data_ptr() for s in pl.recal_sites] == [s[2].data_ptr() for s in frozen.bn_sites]
    table = AB.site_table(pl.recal_sites)
    assert L.lib().rd_bn_recal(table, 0x1000, len(pl.recal_sites), 255, 0, E.EPS, None) == -4          # a max_C below the table's
    assert L.lib().rd_bn_recal(table, 0x1000, len(pl.recal_sites), 256, -1, E.EPS, None) == -2         # (valid but for k)
    # every conv on the route of the modules' training plans
    enc, dec = _module_train_plans(dtype, *geom)
    ours = [op for op in pl.fwd if op[0].__name__ == 'rd_conv']
    theirs = [op for p in (enc, dec) for op in p.fwd if op[0].__name__ == 'rd_conv']
    assert len(ours) == len(theirs) == 27
    for a, b in zip(ours, theirs):
        assert a[2]['layer'] == b[2]['layer']
        ra, rb = _route(a[1][0]._obj, pl.dt), _route(b[1][0]._obj, pl.dt)
        assert ra[0] == 0 and ra == rb, (a[2]['layer'], ra, rb)
    assert [n for n in names if n != 'rd_conv'] == [op[0].__name__ for p in (enc, dec) for op in p.fwd if op[0].__name__ != 'rd_conv']


def test_recal_plan_refuses_other_modes():
    bank = E.ParamBank(MODS, 'cpu')
    for kw in (dict(training=False), dict(fused_step=True), dict(training=False, frozen_bn=True)):
        with pytest.raises(ValueError):
            E.Plan(bank, torch.float32, 2, [0, 2], recal_bn=True, **kw)
    with pytest.raises(ValueError):
        E.Plan(bank, torch.float32, 2, [0, 1, 2], recal_bn=True)
    with pytest.raises(ValueError):
        AB.build_plan(bank, E.WeightPack(bank, MODS, torch.float32), torch.float32, 1, 40, 32)
    gn = [('enc', E.encoder_specs(3, 16, 'gn'))]
    bank = E.ParamBank(gn, 'cpu')
    pl = E.Plan(bank, torch.float32, 1, [0, 1], recal_bn=True)
    E.build_encoder(pl, E.Act(pl, 1, 32, 32, 3), n=16, mname='enc', norm='gn')
    with pytest.raises(ValueError):
        pl.build(E.WeightPack(bank, gn, torch.float32))


def test_recal_bank_shares_the_parameters_and_owns_the_encoder_and_decoder_buffers():
    mods = MODS + [('rec', E.rec_decoder_specs(16, 3, 3))]
    live = E.ParamBank(mods, 'cpu')
    from ramdsir.avg import AveragedBank
    avg = AveragedBank(live)
    view = AB.RecalBank(avg)
    assert view.params is avg.params and list(view.buffers) == list(avg.buffers) and view.index is avg.index
    for (m, key), t in view.buffers.items():
        if m == 'rec':
            assert t is avg.buffers[(m, key)]
        else:
            assert t is not avg.buffers[(m, key)] and t.data_ptr() != avg.buffers[(m, key)].data_ptr() and torch.equal(t, avg.buffers[(m, key)])
    assert AB.ring_bytes(16, 16, 256, 256, 8, 2) == 16 * 16 * 256 * 256 * 8 * 2
