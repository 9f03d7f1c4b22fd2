"""The numpy model of the BatchNorm / GroupNorm finalize (tests/bn_fin_model.py) against references that are not the kernel:
exact rational arithmetic with every operation rounded by a helper of this file, and torch in float64 (nn.BatchNorm2d called once per
group in group order, autograd through F.batch_norm, nn.GroupNorm(1, C)) over every topology of bn_fin_model.TOPOLOGIES; and the
refusals of a folded finalize (rdfin::make_arg, csrc/bn_fin.h), which return before any launch.  No GPU.

Tolerances against torch are the derived float32 rounding bounds written out in bn_fin_model.py ("float32 rounding bounds": roundings
on the path x unit roundoff x 2, differences against the sum of the magnitudes of their terms).  Measured worst case as a fraction
of the bound, over all topologies (WORST below, printed by each test):
    BatchNorm forward   mean 0.43  invstd 0.20  scale 0.22  shift 0.20  y 0.17  running_mean 0.27  running_var 0.21
    BatchNorm backward  P 0.22  Q 0.13  R 0.16  dz 0.15  dgamma 0.13  dbeta 0.23
    GroupNorm           mean 0.48  invstd 0.13  scale 0.17  shift 0.11  P 0.17  Q 0.14  R 0.15  dz 0.17  dgamma 0.12  dbeta 0.16
                        dbias 0.08
The bounds come from the derivation, not from these figures."""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np
import torch
import torch.nn.functional as F

from ramdsir import _lib as L
import bn_fin_model as M

f32, f64 = np.float32, np.float64
EPS, MO = 1e-5, 0.1
EPS32 = float(f32(EPS))
WORST = {}


# ------------------------------------------------------------------------------------------------ rounding of rationals
def _rnd(x, p, qmin):
    """Round-to-nearest-even of a rational to a binary format with p significand bits and least exponent qmin."""
    x = Fr(x)
    if x == 0:
        return Fr(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    if Fr(2) ** (e + 1) <= a:
        e += 1
    assert Fr(2) ** e <= a < Fr(2) ** (e + 1)
    q = max(e - (p - 1), qmin)
    n = round(a / Fr(2) ** q)                              # Fraction.__round__: half to even
    return (n if x > 0 else -n) * Fr(2) ** q


def r32(x):
    return _rnd(x, 24, -149)


def r64(x):
    return _rnd(x, 53, -1074)


def sqrt32(x):
    """Correctly rounded float32 square root of a non-negative float32 given as a rational."""
    x = Fr(x)
    if x == 0:
        return Fr(0)
    k = 120
    num = x * Fr(4) ** k
    assert num.denominator == 1
    s = math.isqrt(num.numerator)
    lo, hi = Fr(s, 2 ** k), Fr(s + 1, 2 ** k)
    if s * s == num.numerator:
        return r32(lo)
    assert r32(lo) == r32(hi)                              # sqrt lies strictly between: both round alike, so does it
    return r32(lo)


def fr(x):
    return Fr(float(x))


def test_rounding_helpers_agree_with_numpy():
    rng = np.random.default_rng(1)
    for _ in range(300):
        a, b = f32(rng.standard_normal() * 10 ** rng.uniform(-20, 20)), f32(rng.standard_normal() * 10 ** rng.uniform(-3, 3))
        assert r32(fr(a) * fr(b)) == fr(f32(a * b)) and r32(fr(a) + fr(b)) == fr(f32(a + b)) and r32(fr(a) / fr(b)) == fr(f32(a / b))
        assert r64(fr(a) / fr(b)) == Fr(float(f64(a) / f64(b)))
        assert sqrt32(fr(abs(a))) == fr(np.sqrt(abs(a)))
    assert r32(Fr(1) + Fr(1, 2 ** 24)) == 1 and r32(Fr(1) + Fr(3, 2 ** 24)) == Fr(1) + Fr(1, 2 ** 22)      # ties to even
    assert r32(Fr(1, 2 ** 150)) == 0 and r32(Fr(3, 2 ** 150)) == Fr(1, 2 ** 148)                              # subnormal ties


# ------------------------------------------------------------------------------------------------ the kernels' formulas on rationals
def fr_momentum(old, x, mo):
    om = r32(1 - fr(mo))
    return r32(r32(om * old) + r32(fr(mo) * x))


def fr_fwd_stat(s1, s2, cnt, cb, eps):
    """fwd_stat of bn_fin.h, one channel: (mean, var, invstd, unb)."""
    m0 = r64(s1 / cnt)
    vard = r64(r64(s2 / cnt) - r64(m0 * m0))
    vard = max(vard, Fr(0))
    var = r32(vard)
    mean = r32(r64(m0 + cb))
    invstd = r32(1 / sqrt32(r32(var + fr(f32(eps)))))
    unb = r32(r64(r64(vard * cnt) / r64(cnt - 1))) if cnt > 1 else var
    return mean, var, invstd, unb


def fr_bwd(s1d, sgzd, mu, is_, gam, cnt):
    s1 = r32(s1d)
    s2 = r32(is_ * r32(r64(sgzd - r64(mu * s1d))))
    P = r32(gam * is_)
    Q = r32(r32(r32(r32(-gam * is_) * is_) * s2) / cnt)
    R = r32(r32(r32(-P * s1) / cnt) - r32(Q * mu))
    return s1, s2, P, Q, R


def _one_group_slots(s1, s2):
    """[1][RD_STAT_SLOTS][C][2] with the sums in copy 0."""
    st = np.zeros((1, L.STAT_SLOTS, len(s1), 2), f64)
    st[0, 0, :, 0], st[0, 0, :, 1] = s1, s2
    return st


def _search(rng, pred, draw, tries=20000):
    for _ in range(tries):
        v = draw(rng)
        if pred(*v):
            return v
    raise AssertionError('no row found')


def test_momentum_step_is_four_roundings_not_an_fma():
    mo = f32(MO)
    om = r32(1 - fr(mo))

    def differs(old, x):
        four = fr_momentum(fr(old), fr(x), mo)
        return four != r32(om * fr(old) + r32(fr(mo) * fr(x))) and four != r32(r32(om * fr(old)) + fr(mo) * fr(x))
    old, x = _search(np.random.default_rng(2), differs, lambda r: (f32(r.standard_normal()), f32(r.standard_normal())))
    got = M.momentum_step_model(np.array([old]), np.array([x]), MO)
    assert fr(got[0]) == fr_momentum(fr(old), fr(x), mo)
    # ... and through fwd_model: count = 4, one copy, no bias: mean = x exactly
    rm, rv, nbt = np.array([old], f32), np.array([1.0], f32), np.array(3, np.int64)
    st = _one_group_slots([4.0 * float(x)], [4.0 * float(f32(x * x)) + 8.0])
    M.fwd_model(st, 0, [4.0], None, [np.ones(1, f32)], [np.zeros(1, f32)], [rm], [rv], [nbt], EPS, MO, 1)
    assert fr(rm[0]) == fr_momentum(fr(old), fr(x), mo) and int(nbt) == 4


def test_shift_is_two_roundings_not_an_fma():
    def differs(beta, mean, sc):
        return r32(fr(beta) - r32(fr(mean) * fr(sc))) != r32(fr(beta) - fr(mean) * fr(sc))
    beta, mean, sc = _search(np.random.default_rng(3), differs, lambda r: tuple(f32(v) for v in r.standard_normal(3)))
    got_sc, got_sh = M.fwd_coef_model(np.array([sc]), np.array([beta]), np.array([mean]), np.array([1.0], f32))
    assert got_sc[0] == sc and fr(got_sh[0]) == r32(fr(beta) - r32(fr(mean) * fr(sc)))


def _clamp_value():
    """A float32 v whose float32 square rounds DOWN: a constant channel of it has s2 / n < (s1 / n)^2 in float64."""
    rng = np.random.default_rng(4)
    (v,) = _search(rng, lambda v: fr(f32(v * v)) < fr(v) * fr(v), lambda r: (f32(1.0 + r.random()),))
    return v


def test_forward_rows_in_exact_rational_arithmetic():
    """count = 1 (unb = var: the kernel's documented choice; torch refuses the case), count = 2, a general count, the clamp channel,
    with and without a conv bias."""
    rng = np.random.default_rng(5)
    vc = _clamp_value()
    for cnt, bias in ((1, True), (2, True), (2, False), (105, True), (4096, False), (2 ** 24, True)):
        Cc = 6
        # channel 0: the clamp channel (cnt values vc: sums exact for these counts up to 2^24 of a 24-bit value: < 2^53)
        s1 = np.round(rng.standard_normal(Cc) * 64 * cnt) / 16
        s2 = np.round((s1 / cnt) ** 2 * cnt * 16 + cnt * 16 * rng.uniform(0.5, 2.0, Cc)) / 16
        s1[0], s2[0] = float(vc) * cnt, float(f32(vc * vc)) * cnt
        if cnt == 1:                                       # one value x per channel: s2 = float32(x^2), x of 12 bits: exact, var = 0 ...
            x = np.round(rng.standard_normal(Cc) * 256) / 64
            s1[1:], s2[1:] = x[1:], (x * x)[1:]
            v5 = f32(1.3)                                  # ... and one whose float32 square rounds UP: a tiny positive var, unb = var
            while fr(f32(v5 * v5)) <= fr(v5) * fr(v5):
                v5 = np.nextafter(v5, f32(2))
            s1[5], s2[5] = float(v5), float(f32(v5 * v5))
        cb = (np.round(rng.standard_normal(Cc) * 8) / 8).astype(f32) if bias else None
        gam, bet = (1 + 0.2 * rng.standard_normal(Cc)).astype(f32), (0.3 * rng.standard_normal(Cc)).astype(f32)
        rm, rv, nbt = (0.1 * rng.standard_normal(Cc)).astype(f32), (1 + 0.1 * rng.random(Cc)).astype(f32), np.array(3, np.int64)
        rm0, rv0 = rm.copy(), rv.copy()
        sc, sh, mean, istd = M.fwd_model(_one_group_slots(s1, s2), 0, [float(cnt)], cb, [gam], [bet], [rm], [rv], [nbt], EPS, MO, 1)
        for c in range(Cc):
            e_mean, e_var, e_is, e_unb = fr_fwd_stat(fr(s1[c]), fr(s2[c]), Fr(cnt), fr(cb[c]) if bias else Fr(0), EPS)
            assert fr(mean[0, c]) == e_mean and fr(istd[0, c]) == e_is, (cnt, c)
            e_sc = r32(fr(gam[c]) * e_is)
            assert fr(sc[0, c]) == e_sc and fr(sh[0, c]) == r32(fr(bet[c]) - r32(e_mean * e_sc)), (cnt, c)
            assert fr(rm[c]) == fr_momentum(fr(rm0[c]), e_mean, f32(MO)) and fr(rv[c]) == fr_momentum(fr(rv0[c]), e_unb, f32(MO)), (cnt, c)
            if cnt == 1:
                assert e_unb == e_var
            if c == 0:                                     # the clamp: var exactly 0, invstd = 1 / sqrt(eps)
                assert fr(s2[0]) / cnt - (fr(s1[0]) / cnt) ** 2 < 0 and e_var == 0
                assert e_is == r32(1 / sqrt32(fr(f32(EPS)))) and istd[0, 0] == f32(1) / np.sqrt(f32(EPS))
        if cnt == 1:
            assert e_var > 0                               # channel 5: the tiny positive variance of one value
        assert int(nbt) == 4


def test_chain_of_three_in_exact_rational_arithmetic():
    """Three groups on one BatchNorm: the 3-step running recursion in group order; dgamma / dbeta over the chain onto a non-zero start."""
    rng = np.random.default_rng(6)
    Cc, counts = 5, [105.0, 2.0, 4096.0]
    st = np.zeros((3, L.STAT_SLOTS, Cc, 2), f64)
    for g, cnt in enumerate(counts):
        s1 = np.round(rng.standard_normal(Cc) * 64 * cnt) / 16
        st[g, 0, :, 0], st[g, 0, :, 1] = s1, np.round((s1 / cnt) ** 2 * cnt * 16 + cnt * 16 * rng.uniform(0.5, 2.0, Cc)) / 16
    gam, bet = (1 + 0.2 * rng.standard_normal(Cc)).astype(f32), (0.3 * rng.standard_normal(Cc)).astype(f32)
    rm, rv, nbt = (0.1 * rng.standard_normal(Cc)).astype(f32), (1 + 0.1 * rng.random(Cc)).astype(f32), np.array(3, np.int64)
    rm0, rv0 = rm.copy(), rv.copy()
    sc, sh, mean, istd = M.fwd_model(st, 0, counts, None, [gam] * 3, [bet] * 3, [rm] * 3, [rv] * 3, [nbt] * 3, EPS, MO, 1)
    for c in range(Cc):
        em, ev = fr(rm0[c]), fr(rv0[c])
        for g, cnt in enumerate(counts):
            e_mean, _, e_is, e_unb = fr_fwd_stat(fr(st[g, 0, c, 0]), fr(st[g, 0, c, 1]), Fr(int(cnt)), Fr(0), EPS)
            assert fr(mean[g, c]) == e_mean and fr(istd[g, c]) == e_is
            em, ev = fr_momentum(em, e_mean, f32(MO)), fr_momentum(ev, e_unb, f32(MO))
        assert fr(rm[c]) == em and fr(rv[c]) == ev
    assert int(nbt) == 6
    # backward over the same chain
    bst = np.zeros((3, L.STAT_SLOTS, Cc, 2), f64)
    bst[:, 0] = np.round(rng.standard_normal((3, Cc, 2)) * 1024) / 64
    dg, db = (0.05 * rng.standard_normal(Cc)).astype(f32), (0.05 * rng.standard_normal(Cc)).astype(f32)
    dg0, db0 = dg.copy(), db.copy()
    P, Q, R = M.bwd_model(bst, 0, mean, istd, counts, [gam] * 3, [dg] * 3, [db] * 3)
    for c in range(Cc):
        ea, eb = fr(dg0[c]), fr(db0[c])
        for g, cnt in enumerate(counts):
            s1, s2, eP, eQ, eR = fr_bwd(fr(bst[g, 0, c, 0]), fr(bst[g, 0, c, 1]), fr(mean[g, c]), fr(istd[g, c]), fr(gam[c]), Fr(int(cnt)))
            assert (fr(P[g, c]), fr(Q[g, c]), fr(R[g, c])) == (eP, eQ, eR)
            ea, eb = r32(ea + s2), r32(eb + s1)
        assert fr(dg[c]) == ea and fr(db[c]) == eb
        assert dg0[c] != 0 and db0[c] != 0


# ------------------------------------------------------------------------------------------------ torch in float64
GEOM = [(1, 2, 1), (3, 5, 7), (2, 3, 2), (1, 4, 4), (2, 1, 3)]       # (images, h, w) per group, cyclic: counts 2, 105, 12, 16, 6


def _note(key, err, bound):
    err, bound = np.asarray(err, f64), np.asarray(bound, f64)
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert np.all(err <= bound), (key, ratio)


def _group_data(name, Cc, rng, bias):
    """Dyadic float32 data per group: z (the bias-free conv result), x = z + b, the gradient gy; statistic slots as a producer with
    8 copies leaves them (pixel i into copy i % 8)."""
    G = len(M.TOPOLOGIES[name]['mod'])
    cb = (rng.integers(-8, 9, Cc) / 8.0).astype(f32) if bias else None
    off = rng.integers(-32, 33, Cc) / 4.0
    xs, gys, counts = [], [], []
    st, bst = np.zeros((G, L.STAT_SLOTS, Cc, 2), f64), np.zeros((G, L.STAT_SLOTS, Cc, 2), f64)
    for g in range(G):
        n, h, w = GEOM[g % len(GEOM)]
        z = rng.integers(-64, 65, (n, Cc, h, w)) / 16.0 + off[None, :, None, None]
        x = z + (cb.astype(f64)[None, :, None, None] if bias else 0.0)
        gy = rng.integers(-32, 33, (n, Cc, h, w)) / 8.0
        zp, xp, gp = (t.transpose(0, 2, 3, 1).reshape(-1, Cc) for t in (z, x, gy))
        for k in range(8):
            st[g, k, :, 0], st[g, k, :, 1] = zp[k::8].sum(0), (zp[k::8] ** 2).sum(0)
            bst[g, k, :, 0], bst[g, k, :, 1] = gp[k::8].sum(0), (gp[k::8] * xp[k::8]).sum(0)
        assert np.all(x.astype(f32) == x) and np.all((z * z).astype(f32) == z * z) and np.all((gy * x).astype(f32) == gy * x)
        xs.append(x); gys.append(gy); counts.append(float(n * h * w))
    assert M.sums_exact(st, 8) and M.sums_exact(bst, 8)
    return xs, gys, counts, cb, st, bst


def test_model_against_torch_double_over_the_topology_table():
    for ti, name in enumerate(M.TOPOLOGIES):
        rng = np.random.default_rng(100 + ti)
        Cc = 8
        st0, maps = M.make_state(name, Cc, rng)
        xs, gys, counts, cb, slots, bslots = _group_data(name, Cc, rng, bias=name != 'T2')
        G = len(counts)
        lists, arrs = M.state_lists(st0, maps)
        sc, sh, mean, istd = M.fwd_model(slots, 8, counts, cb, lists['gamma'], lists['beta'], lists['rm'], lists['rv'], lists['nbt'],
                                         EPS, MO, 1)
        # ---- forward: one module per running_mean object, called once per group in group order
        mods, run_bound = {}, {}
        for m in st0['rm']:
            bn = torch.nn.BatchNorm2d(Cc, eps=EPS32, momentum=float(f32(MO))).double().train()
            bn.running_mean.copy_(torch.from_numpy(st0['rm'][m].astype(f64)))
            bn.running_var.copy_(torch.from_numpy(st0['rv'][m].astype(f64)))
            bn.num_batches_tracked.fill_(3)
            mods[m] = bn
            run_bound[m] = [np.zeros(Cc), np.zeros(Cc)]
        exact = []
        for g in range(G):
            x = torch.from_numpy(xs[g])
            w, b = (torch.from_numpy(lists[k][g].astype(f64)) for k in ('gamma', 'beta'))
            m = maps['rm'][g]
            e_mean, e_var = xs[g].mean((0, 2, 3)), xs[g].var((0, 2, 3))
            if m is None:
                y = F.batch_norm(x, None, None, w, b, True, float(f32(MO)), EPS32)
            else:
                bn = mods[m]
                bn.weight.data, bn.bias.data = w, b
                old_m, old_v = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
                y = bn(x).detach()
                om, mo = 1.0 - float(f32(MO)), float(f32(MO))
                unb = e_var * counts[g] / (counts[g] - 1.0)
                run_bound[m][0] += M.SLACK * M.U32 * 3 * (np.abs(om * old_m) + np.abs(mo * e_mean))
                run_bound[m][1] += M.SLACK * M.U32 * 3 * (np.abs(om * old_v) + np.abs(mo * unb))
            e_is = 1.0 / np.sqrt(e_var + EPS32)
            exact.append((e_mean, e_is))
            bnd = M.bn_fwd_bounds(lists['gamma'][g], lists['beta'][g], e_mean, e_is)
            e_sc = lists['gamma'][g].astype(f64) * e_is
            e_sh = lists['beta'][g].astype(f64) - e_mean * e_sc
            # the exact coefficients ARE the module: y = x scale + shift in float64
            yy = xs[g] * e_sc[None, :, None, None] + e_sh[None, :, None, None]
            assert np.max(np.abs(yy - y.numpy())) <= 1e-12 * (1 + np.max(np.abs(yy)))
            _note('mean', np.abs(mean[g] - e_mean), bnd['mean'])
            _note('invstd', np.abs(istd[g] - e_is), bnd['invstd'])
            _note('scale', np.abs(sc[g] - e_sc), bnd['scale'])
            _note('shift', np.abs(sh[g] - e_sh), bnd['shift'])
            got = xs[g] * sc[g].astype(f64)[None, :, None, None] + sh[g].astype(f64)[None, :, None, None]
            _note('y', np.abs(got - y.numpy()), np.abs(xs[g]) * bnd['scale'][None, :, None, None] + bnd['shift'][None, :, None, None])
        for m, bn in mods.items():
            _note('running_mean', np.abs(arrs['rm'][m] - bn.running_mean.numpy()), run_bound[m][0])
            _note('running_var', np.abs(arrs['rv'][m] - bn.running_var.numpy()), run_bound[m][1])
            if maps['nbt'] == maps['rm']:
                assert int(arrs['nbt'][m]) == int(bn.num_batches_tracked)
        for m, a in arrs['nbt'].items():
            assert int(a) == 3 + maps['nbt'].count(m)
        # ---- backward: autograd through F.batch_norm, group by group; per-array sums in group order
        P, Q, R = M.bwd_model(bslots, 8, mean, istd, counts, lists['gamma'], lists['dgamma'], lists['dbeta'])
        terms = {'dgamma': {m: [] for m in st0['dgamma']}, 'dbeta': {m: [] for m in st0['dbeta']}}
        tb = {'dgamma': {m: np.zeros(Cc) for m in st0['dgamma']}, 'dbeta': {m: np.zeros(Cc) for m in st0['dbeta']}}
        for g in range(G):
            x = torch.from_numpy(xs[g]).requires_grad_(True)
            w = torch.from_numpy(lists['gamma'][g].astype(f64)).requires_grad_(True)
            b = torch.from_numpy(lists['beta'][g].astype(f64)).requires_grad_(True)
            (F.batch_norm(x, None, None, w, b, True, 0.1, EPS32) * torch.from_numpy(gys[g])).sum().backward()
            e_mean, e_is = exact[g]
            s1, sgz = gys[g].sum((0, 2, 3)), (gys[g] * xs[g]).sum((0, 2, 3))
            val, bnd = M.bn_bwd_exact(lists['gamma'][g], e_mean, e_is, s1, sgz, counts[g])
            bc = lambda v: np.asarray(v, f64)[None, :, None, None]
            dz = bc(val['P']) * gys[g] + bc(val['Q']) * xs[g] + bc(val['R'])
            scale_ = 1 + np.max(np.abs(bc(val['P']) * gys[g]) + np.abs(bc(val['Q']) * xs[g]) + np.abs(bc(val['R'])))
            assert np.max(np.abs(dz - x.grad.numpy())) <= 1e-11 * scale_                   # the exact coefficients ARE autograd
            assert np.max(np.abs(val['s2'] - w.grad.numpy())) <= 1e-11 * (1 + np.max(np.abs(sgz) + np.abs(e_mean * s1)) * np.max(e_is))
            assert np.max(np.abs(val['s1'] - b.grad.numpy())) <= 1e-12 * (1 + np.max(np.abs(s1)))
            for k, a in (('P', P), ('Q', Q), ('R', R)):
                _note(k, np.abs(a[g] - val[k]), bnd[k])
            got = bc(P[g]) * gys[g] + bc(Q[g]) * xs[g] + bc(R[g])
            _note('dz', np.abs(got - x.grad.numpy()), np.abs(gys[g]) * bc(bnd['P']) + np.abs(xs[g]) * bc(bnd['Q']) + bc(bnd['R']))
            for k, key in (('dgamma', 's2'), ('dbeta', 's1')):
                m = maps[k][g]
                if m is not None:
                    terms[k][m].append((w.grad if k == 'dgamma' else b.grad).numpy())
                    tb[k][m] += bnd[key]
        for k in ('dgamma', 'dbeta'):
            for m in st0[k]:
                total, ab = M.accumulate_bound(terms[k][m], st0[k][m])
                _note(k, np.abs(arrs[k][m] - total), tb[k][m] + ab)
    print('worst case / bound:', {k: round(v, 3) for k, v in WORST.items()})


def test_groupnorm_model_against_torch_double():
    for ci, (G, Cc, bias, with_db) in enumerate([(1, 1, True, True), (3, 24, True, True), (16, 24, False, True), (3, 300, True, False),
                                                 (1, 300, False, True), (3, 1, False, False)]):
        rng = np.random.default_rng(200 + ci)
        h, w = 3, 5
        cb = (rng.integers(-8, 9, Cc) / 8.0).astype(f32) if bias else None
        off = rng.integers(-32, 33, Cc) / 4.0
        z = rng.integers(-64, 65, (G, Cc, h, w)) / 16.0 + off[None, :, None, None]
        gy = rng.integers(-32, 33, (G, Cc, h, w)) / 8.0
        gam, bet = (1 + 0.2 * rng.standard_normal(Cc)).astype(f32), (0.3 * rng.standard_normal(Cc)).astype(f32)
        zt = torch.from_numpy(z).requires_grad_(True)
        bt = torch.from_numpy((cb if bias else np.zeros(Cc, f32)).astype(f64)).requires_grad_(True)
        gn = torch.nn.GroupNorm(1, Cc, eps=EPS32).double()
        gn.weight.data, gn.bias.data = torch.from_numpy(gam.astype(f64)), torch.from_numpy(bet.astype(f64))
        xt = zt + bt[None, :, None, None]
        y = gn(xt)
        (y * torch.from_numpy(gy)).sum().backward()
        x = xt.detach().numpy()
        st, bst = np.zeros((G, L.STAT_SLOTS, Cc, 2), f64), np.zeros((G, L.STAT_SLOTS, Cc, 2), f64)
        for g in range(G):
            zp, xp, gp = (t[g].transpose(1, 2, 0).reshape(-1, Cc) for t in (z, x, gy))
            for k in range(5):
                st[g, 11 * k, :, 0], st[g, 11 * k, :, 1] = zp[k::5].sum(0), (zp[k::5] ** 2).sum(0)
                bst[g, 11 * k, :, 0], bst[g, 11 * k, :, 1] = gp[k::5].sum(0), (gp[k::5] * xp[k::5]).sum(0)
        counts = [float(h * w)] * G
        sc, sh, mean, istd = M.gn_fwd_model(st, counts, cb, gam, bet, EPS)
        dg0, db0, dc0 = ((0.05 * rng.standard_normal(Cc)).astype(f32) for _ in range(3))
        dg, db, dc = dg0.copy(), db0.copy(), (dc0.copy() if with_db else None)
        P, Q, R = M.gn_bwd_model(bst, st, mean, istd, counts, cb, gam, dg, db, dc)
        terms, tbnd = {k: [] for k in ('dgamma', 'dbeta', 'dbias')}, {k: np.zeros(Cc) for k in ('dgamma', 'dbeta', 'dbias')}
        bc = lambda v: np.asarray(v, f64)[:, None, None]
        for g in range(G):
            s1, s2 = st[g, :, :, 0].sum(0), st[g, :, :, 1].sum(0)
            val, bnd = M.gn_exact(s1, s2, bst[g, :, :, 0].sum(0), bst[g, :, :, 1].sum(0), s1, counts[g], cb, gam, bet, EPS)
            yy = x[g] * bc(val['scale']) + bc(val['shift'])
            assert np.max(np.abs(yy - y[g].detach().numpy())) <= 1e-11 * (1 + np.max(np.abs(yy)))            # the exact values ARE the module
            dz = bc(val['P']) * gy[g] + bc(val['Q']) * x[g] + bc(val['R'])
            mag = np.abs(bc(val['P']) * gy[g]) + np.abs(bc(val['Q']) * x[g]) + np.abs(bc(val['R']))
            assert np.max(np.abs(dz - zt.grad[g].numpy())) <= 1e-11 * (1 + np.max(mag))
            for k, a in (('mean', mean), ('invstd', istd), ('scale', sc), ('shift', sh), ('P', P), ('Q', Q), ('R', R)):
                _note('gn_' + k, np.abs(a[g] - val[k]), bnd[k])
            got = bc(P[g]) * gy[g] + bc(Q[g]) * x[g] + bc(R[g])
            _note('gn_dz', np.abs(got - zt.grad[g].numpy()), np.abs(gy[g]) * bc(bnd['P']) + np.abs(x[g]) * bc(bnd['Q']) + bc(bnd['R']))
            for k in terms:
                terms[k].append(val[k])
                tbnd[k] += bnd[k]
        for k, arr, start, ref in (('dgamma', dg, dg0, gn.weight.grad), ('dbeta', db, db0, gn.bias.grad), ('dbias', dc, dc0, bt.grad)):
            if arr is None:
                continue
            total, ab = M.accumulate_bound(terms[k])
            assert np.max(np.abs(total - ref.numpy())) <= 1e-10 * (1 + np.max(np.abs(total)) + np.max(ab) / M.U32)
            final = total + start.astype(f64)              # the images are summed from 0, then added to the old content once
            _note('gn_' + k, np.abs(arr - final), tbnd[k] + ab + M.SLACK * M.U32 * np.abs(final))
    print('worst case / bound:', {k: round(v, 3) for k, v in WORST.items() if k.startswith('gn_')})


# ------------------------------------------------------------------------------------------------ refusals, before any launch
FAKE = 0x10000                                             # never dereferenced: every call below returns before it launches


def _fwd_fin(Cc=8, G=2, nslots=8, training=1):
    p = L.RdBnFwd()
    p.stats, p.scale, p.shift, p.mean, p.invstd = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000
    for g in range(max(G, 0)):
        p.gamma[g], p.beta[g], p.count[g] = FAKE + 0x5000, FAKE + 0x6000, 4.0
    p.C, p.G, p.eps, p.momentum, p.training, p.nslots = Cc, G, EPS, MO, training, nslots
    return p


def _bwd_fin(Cc=8, G=2, nslots=8):
    q = L.RdBnBwd()
    q.bstats, q.mean, q.invstd, q.P, q.Q, q.R = FAKE, FAKE + 0x3000, FAKE + 0x4000, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x7000
    for g in range(max(G, 0)):
        q.gamma[g], q.count[g] = FAKE + 0x5000, 4.0
    q.C, q.G, q.nslots = Cc, G, nslots
    return q


def _pool(p, Cc=8, scale=FAKE + 0x1000, shift=FAKE + 0x2000):
    gs = L.gstart_array([0, 1, 2])
    return L.lib().rd_pool_fwd(FAKE + 0x8000, scale, shift, 0.0, FAKE + 0x9000, 2, 1, 1, Cc, 2, gs, L.RD_F32, C.addressof(p), L.FIN_OWNER, None)


def _up(q, Cc=8, P=FAKE + 0x1000, Q=FAKE + 0x2000, R=FAKE + 0x7000):
    gs = L.gstart_array([0, 1, 2])
    return L.lib().rd_up_bwd(FAKE + 0x8000, FAKE + 0x9000, FAKE + 0xa000, P, Q, R, 2, 1, 1, Cc, 2, gs, L.RD_F32, C.addressof(q),
                             L.FIN_OWNER, None)


def test_folded_finalize_refusals():
    assert L.FIN_MAX_G == 8
    for kw in (dict(G=9), dict(G=0), dict(Cc=12), dict(nslots=12), dict(nslots=72), dict(nslots=-8)):
        assert _pool(_fwd_fin(**kw)) == -3, kw
        assert _up(_bwd_fin(**kw)) == -3, kw
    assert _pool(_fwd_fin(training=0)) == -3
    assert _pool(_fwd_fin(), scale=FAKE + 0x1004) == -3 and _pool(_fwd_fin(), shift=FAKE + 0x2004) == -3
    assert _pool(_fwd_fin(), scale=None) == -3
    assert _up(_bwd_fin(), P=FAKE + 0x1004) == -3 and _up(_bwd_fin(), Q=FAKE + 0x2004) == -3 and _up(_bwd_fin(), R=FAKE + 0x7004) == -3
