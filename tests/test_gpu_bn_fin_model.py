"""-m gpu: the BatchNorm finalize -- the explicit kernels rd_bn_finalize_fwd / rd_bn_finalize_bwd (csrc/bn.hip) and the finalize folded
into a consumer's prologue (csrc/bn_fin.h, carried here by rd_pool_fwd and rd_up_bwd in fp32) -- and the GroupNorm finalize kernels
rd_gn_finalize_fwd / rd_gn_finalize_bwd against the numpy model of tests/bn_fin_model.py, which tests/test_cpu_bn_fin_model.py holds to
exact rational arithmetic and to torch in float64.

Every comparison with the model is an equality on BITS (signs of zero included), over the topology table bn_fin_model.TOPOLOGIES
(chains of three and sixteen groups on one BatchNorm, interleaved chains, NULL groups inside a chain, the InstanceNorm contract,
pointer arrays shared differently), ragged counts from {1, 2, 105, 4096, 2^24}, a non-trivial starting state and planted channels
(_PLANTED).  The exceptions, all GroupNorm (those kernels are compiled with contraction on): on exact rows Q is within 1 ulp, and
shift and R (a - b * c: one fma or two roundings) equal one of the two forms on bits -- within 1 ulp of the model wherever the
difference does not cancel; random rows are within the derived rounding bounds of bn_fin_model against a float64 evaluation.

Every output vector, running array, counter, dgamma and dbeta lies between 4 KiB sentinels; statistic copies the folded code must not
read hold 1e30, buffers nothing may read hold NaN.  All are valid device buffers."""
import ctypes as C
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ramdsir import _lib as L                      # noqa: E402
import gpu_util as U                               # noqa: E402
import bn_fin_model as M                           # noqa: E402
from test_gpu_loss_edges import Guarded            # noqa: E402

f32, f64 = np.float32, np.float64
EPS, MO = 1e-5, 0.1
COUNTS = [1, 2, 105, 4096, 2 ** 24]
# channels planted in every case with C >= 8
_PLANTED = """0: mean = 1000 sigma; 1: mean = -30000 sigma (forward: m0^2 against s2 / n; backward: sgz - mu s1 cancels, float64 in the
kernel); 2: a constant channel (var = 0 exactly); 3: the clamp channel (a constant whose float32 square rounds down: s2 / n - m0^2 < 0);
4: gamma = 0; 5: gamma < 0; 6: conv_bias = 1000 beside sums of 2^-10; 7: both backward sums exactly 0 (signs of zero)."""


def _clamp_value():
    """The first float32 above 1 whose float32 square rounds DOWN by at least 2^-25: a constant channel of it has s2 / n - m0^2 <=
    -2^-25 in float64, 0.3 % of eps -- unclamped, invstd would differ in its leading digits (a rounding of 2^-46, as 1 + 2^-23 gives,
    would vanish in var + eps)."""
    v = f32(1.0)
    while True:
        v = np.nextafter(v, f32(2))
        if Fr(float(v)) ** 2 - Fr(float(f32(v * v))) >= Fr(1, 2 ** 25):
            return v


VC = _clamp_value()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.int64 else np.int32)


def _same(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(np.asarray(want)).reshape(-1)
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        gv, wv = g.view(f32) if g.dtype == np.int32 else g, w.view(f32) if w.dtype == np.int32 else w
        raise AssertionError('%s: %d of %d differ on bits; first at %d: got %r, model %r' % (what, bad.size, g.size, bad[0], gv[bad[0]], wv[bad[0]]))


# ------------------------------------------------------------------------------------------------ data
def _split_counts(cnt, ns):
    n = np.full(ns, cnt // ns, np.int64)
    n[0] += cnt - int(n.sum())
    return n


def _fwd_slots(G, Cc, counts, ns, rng, fill=0.0):
    """Statistic copies [G][RD_STAT_SLOTS][C][2] as a producer with `ns` copies leaves them: copy k holds the sums of n_k values of
    per-value moments (a, b) = (m, m^2 + v) plus a jitter that sums to zero over the copies -- all dyadic, so every order of addition
    is exact (asserted by the callers with bn_fin_model.sums_exact).  Copies from `ns` on hold `fill`.  Returns (slots, conv bias)."""
    st = np.full((G, L.STAT_SLOTS, Cc, 2), fill, f64)
    cb = (np.round(rng.standard_normal(Cc) * 8) / 8).astype(f32)
    for g in range(G):
        m = np.round(rng.standard_normal(Cc) * 32) / 16
        v = np.round(rng.uniform(0.5, 2.0, Cc) * 16) / 16
        a, b = m, m * m + v
        jit = np.round(rng.uniform(-16, 16, (ns, Cc, 2)) * 256) / 256
        if Cc >= 8:
            a[0], b[0] = 1000.0, 1000.0 ** 2 + 1.0
            a[1], b[1] = -30000.0, 30000.0 ** 2 + 1.0
            a[2], b[2] = 1.5, 2.25
            a[3], b[3] = float(VC), float(f32(VC * VC))
            a[6], b[6] = 2.0 ** -10, 2.0 ** -20 + 2.0 ** -12
            jit[:, [0, 1, 2, 3, 6]] = 0
        jit[0] = -jit[1:].sum(0)
        n = _split_counts(int(counts[g]), ns).astype(f64)
        st[g, :ns, :, 0] = n[:, None] * a[None] + jit[:, :, 0]
        st[g, :ns, :, 1] = n[:, None] * b[None] + jit[:, :, 1]
    if Cc >= 8:
        cb[6] = 1000.0
    return st, cb


def _bwd_slots(G, Cc, mean, ns, rng, fill=0.0):
    """Backward copies (sum g, sum g z): sum g z = mu * sum g + a moderate remainder (what the data of a channel with mean mu
    gives: the kernel's difference cancels), multiples of 2^-6 spread over `ns` copies; channel 7 exactly zero."""
    st = np.full((G, L.STAT_SLOTS, Cc, 2), fill, f64)
    for g in range(G):
        s1 = np.round(rng.standard_normal(Cc) * 100 * 64) / 64
        sgz = np.round((mean[g].astype(f64) * s1 + rng.standard_normal(Cc) * 50) * 64) / 64
        tot = np.stack([s1, sgz], -1)
        if Cc >= 8:
            tot[7] = 0.0
        sp = M.spread_slots(tot, ns, rng)
        if Cc >= 8:
            sp[:, 7] = 0.0
        st[g, :ns] = sp[:ns]
    return st


def _plant_params(st, Cc, name):
    if Cc >= 8 and not M.TOPOLOGIES[name].get('instnorm'):          # (the InstanceNorm contract: gamma stays ones)
        for a in st['gamma'].values():
            a[4], a[5] = 0.0, -abs(a[5]) - 0.5


def _counts(G, off):
    return [float(COUNTS[(g + off) % len(COUNTS)]) for g in range(G)]


# ------------------------------------------------------------------------------------------------ device state between sentinels
class DevState:
    """The arrays of a bn_fin_model state on the device, one guarded buffer per module and key."""
    def __init__(self, st, maps):
        self.maps, self.buf = maps, {k: {} for k in M.STATE_KEYS}
        for k in M.STATE_KEYS:
            for m, a in st[k].items():
                if k == 'nbt':
                    gb = Guarded(8, torch.int64, fill=0)
                    gb.t.fill_(int(a))
                else:
                    gb = Guarded(4 * a.shape[0], torch.float32)
                    gb.t.copy_(torch.from_numpy(a))
                self.buf[k][m] = gb

    def ptr(self, k, g):
        m = self.maps[k][g]
        return None if m is None else self.buf[k][m].ptr()

    def load(self, st):
        for k in M.STATE_KEYS:
            for m, a in st[k].items():
                if k == 'nbt':
                    self.buf[k][m].t.fill_(int(a))
                else:
                    self.buf[k][m].t.copy_(torch.from_numpy(a))

    def intact(self):
        return all(gb.intact() for d in self.buf.values() for gb in d.values())

    def check(self, arrs, keys, what):
        for k in keys:
            for m, a in arrs[k].items():
                _same(self.buf[k][m].t, a, '%s %s[%s]' % (what, k, m))


def _fwd_desc(ds, stats, cbias, out, Cc, counts, nslots, training=1):
    G = len(counts)
    p = L.RdBnFwd()
    p.stats = stats.data_ptr()
    p.conv_bias = cbias.data_ptr() if cbias is not None else None
    for k in ('scale', 'shift', 'mean', 'invstd'):
        setattr(p, k, out[k].ptr())
    for g in range(G):
        p.gamma[g], p.beta[g] = ds.ptr('gamma', g), ds.ptr('beta', g)
        p.running_mean[g], p.running_var[g], p.num_batches_tracked[g] = ds.ptr('rm', g), ds.ptr('rv', g), ds.ptr('nbt', g)
        p.count[g] = counts[g]
    p.C, p.G, p.eps, p.momentum, p.training, p.nslots = Cc, G, EPS, MO, training, nslots
    return p


def _bwd_desc(ds, bstats, mean, invstd, out, Cc, counts, nslots):
    G = len(counts)
    q = L.RdBnBwd()
    q.bstats, q.mean, q.invstd = bstats.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    q.P, q.Q, q.R = out['P'].ptr(), out['Q'].ptr(), out['R'].ptr()
    for g in range(G):
        q.gamma[g], q.dgamma[g], q.dbeta[g] = ds.ptr('gamma', g), ds.ptr('dgamma', g), ds.ptr('dbeta', g)
        q.count[g] = counts[g]
    q.C, q.G, q.nslots = Cc, G, nslots
    return q


def _outs(keys, G, Cc):
    return {k: Guarded(4 * G * Cc, torch.float32) for k in keys}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(U.dev())


def _model_fwd(st, maps, slots, nslots, counts, cb, training=1, invstd=None):
    lists, arrs = M.state_lists(st, maps)
    out = M.fwd_model(slots, nslots, counts, cb, lists['gamma'], lists['beta'], lists['rm'], lists['rv'], lists['nbt'], EPS, MO,
                      training, invstd=invstd)
    return dict(zip(('scale', 'shift', 'mean', 'invstd'), out)), arrs


def _model_bwd(st, maps, bslots, nslots, mean, invstd, counts):
    lists, arrs = M.state_lists(st, maps)
    out = M.bwd_model(bslots, nslots, mean, invstd, counts, lists['gamma'], lists['dgamma'], lists['dbeta'])
    return dict(zip('PQR', out)), arrs


# ------------------------------------------------------------------------------------------------ the explicit kernels
@pytest.mark.parametrize('Cc', [1, 24, 256])
def test_explicit_finalize_equals_the_model_on_bits(Cc):
    """rd_bn_finalize_fwd, then rd_bn_finalize_bwd on the saved mean / invstd it left, T1-T10: every output, running array, counter,
    dgamma and dbeta equals the model on bits."""
    lib = L.lib()
    for ti, name in enumerate(M.TOPOLOGIES):
        rng = np.random.default_rng(1000 * Cc + ti)
        st, maps = M.make_state(name, Cc, rng)
        _plant_params(st, Cc, name)
        G = len(maps['rm'])
        counts = _counts(G, ti)
        ns = L.STAT_SLOTS if ti % 2 else L.STAT_SLOTS_FOLD        # the explicit kernels read all copies: the unused ones hold zero
        slots, cb = _fwd_slots(G, Cc, counts, ns, rng)
        if name == 'T2':
            cb = None
        assert M.sums_exact(slots, L.STAT_SLOTS)
        ds = DevState(st, maps)
        out = _outs(('scale', 'shift', 'mean', 'invstd'), G, Cc)
        sd, cbd = _dev(slots), (_dev(cb) if cb is not None else None)
        p = _fwd_desc(ds, sd, cbd, out, Cc, counts, 0)
        L.check(lib.rd_bn_finalize_fwd(C.byref(p), None), name)
        torch.cuda.synchronize()
        want, arrs = _model_fwd(st, maps, slots, 0, counts, cb)
        _same(out['mean'].t, want['mean'], name + ' mean')
        _same(out['invstd'].t, want['invstd'], name + ' invstd')      # 1 / sqrt and the divisions are the correctly rounded sequences
        _same(out['scale'].t, want['scale'], name + ' scale')
        _same(out['shift'].t, want['shift'], name + ' shift')
        ds.check(arrs, M.STATE_KEYS, name)
        assert ds.intact() and all(o.intact() for o in out.values()), name
        if Cc >= 8:                                        # the planted channels are what they claim to be
            assert np.all(want['invstd'][:, 2:4] == f32(1) / np.sqrt(f32(EPS)))
            assert M.invstd_model(f32(float(f32(VC * VC)) - float(VC) ** 2), EPS) != f32(1) / np.sqrt(f32(EPS))      # unclamped: visible
            assert np.all(want['scale'][:, 4] == 0) or name == 'T8'
        # ---- backward on what the forward left
        bslots = _bwd_slots(G, Cc, want['mean'], ns, rng)
        assert M.sums_exact(bslots, L.STAT_SLOTS)
        bout = _outs('PQR', G, Cc)
        q = _bwd_desc(ds, _dev(bslots), out['mean'].t, out['invstd'].t, bout, Cc, counts, 0)
        L.check(lib.rd_bn_finalize_bwd(C.byref(q), None), name + ' bwd')
        torch.cuda.synchronize()
        st2 = {k: {m: a.copy() for m, a in arrs[k].items()} for k in M.STATE_KEYS}
        bw, arrs2 = _model_bwd(st2, maps, bslots, 0, want['mean'], want['invstd'], counts)
        for k in 'PQR':
            _same(bout[k].t, bw[k], '%s %s' % (name, k))
        ds.check(arrs2, M.STATE_KEYS, name + ' bwd')
        assert ds.intact() and all(o.intact() for o in bout.values()), name
        if Cc >= 8:
            assert (np.all(bw['P'][:, 4] == 0) or name == 'T8') and np.all(bw['Q'][:, 7] == 0) and np.all(bw['R'][:, 7] == 0)


@pytest.mark.parametrize('name', ['T3', 'T7'])
def test_explicit_finalize_eval_mode(name):
    """training = 0: coefficients from the running statistics (mean 0, variance 1 for a group without), the statistics buffer (NaN)
    unread, running arrays and counters unchanged on bits."""
    Cc = 24
    rng = np.random.default_rng(77)
    st, maps = M.make_state(name, Cc, rng)
    _plant_params(st, Cc, name)
    G = len(maps['rm'])
    counts = _counts(G, 1)
    ds = DevState(st, maps)
    out = _outs(('scale', 'shift', 'mean', 'invstd'), G, Cc)
    nan = torch.full((G, L.STAT_SLOTS, Cc, 2), float('nan'), dtype=torch.float64, device=U.dev())
    cbd = _dev(np.full(Cc, np.nan, f32))                   # eval mode has no batch mean to add the bias to
    p = _fwd_desc(ds, nan, cbd, out, Cc, counts, 0, training=0)
    L.check(L.lib().rd_bn_finalize_fwd(C.byref(p), None), name)
    torch.cuda.synchronize()
    want, arrs = _model_fwd(st, maps, None, 0, counts, None, training=0)
    for k in out:
        assert bool(torch.isfinite(out[k].t).all()), k
        _same(out[k].t, want[k], '%s eval %s' % (name, k))
    ds.check(st, M.STATE_KEYS, name + ' eval')             # the starting state, untouched
    assert ds.intact() and all(o.intact() for o in out.values())
    for g, m in enumerate(maps['rm']):
        if m is None:
            assert np.all(want['mean'][g] == 0) and np.all(want['invstd'][g] == f32(1) / np.sqrt(f32(1) + f32(EPS)))


# ------------------------------------------------------------------------------------------------ the folded finalize
def _gstart(G, ragged):
    gs = [0]
    for g in range(G):
        gs.append(gs[-1] + (1 + (g % 3 == 1) if ragged else 1))
    return gs


@pytest.mark.parametrize('Cc', [4, 24, 256])
def test_folded_forward_finalize_equals_the_model_on_bits(Cc):
    """rdfin::fwd in the global-path prologue of rd_pool_fwd (fp32, 2 x 2 x C images, one workgroup per image: every workgroup
    writes), T1-T7 x nslots 0 / 8 / 24 / 64, owner and non-owner.  Copies from nslots on hold 1e30 and must not be read."""
    lib = L.lib()
    for ti, name in enumerate(M.FOLDED):
        for ni, nslots in enumerate((0, 8, 24, 64)):
            rng = np.random.default_rng(2000 * Cc + 10 * ti + ni)
            st, maps = M.make_state(name, Cc, rng)
            _plant_params(st, Cc, name)
            G = len(maps['rm'])
            counts = _counts(G, ti + ni)
            ns = nslots or L.STAT_SLOTS
            slots, cb = _fwd_slots(G, Cc, counts, ns, rng, fill=1e30)
            if name == 'T2':
                cb = None
            assert M.sums_exact(slots, ns)
            want, arrs = _model_fwd(st, maps, slots, nslots, counts, cb)
            gs = _gstart(G, ragged=(ti + ni) % 2 == 1)
            N = gs[-1]
            z = torch.from_numpy(rng.standard_normal((N, 2, 2, Cc)).astype(f32)).to(U.dev())
            sd, cbd = _dev(slots), (_dev(cb) if cb is not None else None)
            ds = DevState(st, maps)
            for owner in (True, False):
                ds.load(st)
                out = _outs(('scale', 'shift', 'mean', 'invstd'), G, Cc)
                pooled = Guarded(4 * N * Cc, torch.float32)
                p = _fwd_desc(ds, sd, cbd, out, Cc, counts, nslots)
                what = '%s nslots %d %s' % (name, nslots, 'owner' if owner else 'non-owner')
                L.check(lib.rd_pool_fwd(L.ptr(z), out['scale'].ptr(), out['shift'].ptr(), 0.0, pooled.ptr(), N, 1, 1, Cc, G,
                                        L.gstart_array(gs), L.RD_F32, C.addressof(p), L.FIN_OWNER if owner else 0, None), what)
                torch.cuda.synchronize()
                _same(out['scale'].t, want['scale'], what + ' scale')
                _same(out['shift'].t, want['shift'], what + ' shift')
                if owner:
                    _same(out['mean'].t, want['mean'], what + ' mean')
                    _same(out['invstd'].t, want['invstd'], what + ' invstd')
                    ds.check(arrs, M.STATE_KEYS, what)
                else:                                      # what happens once per BatchNorm call is the owner's alone
                    assert bool(torch.isnan(out['mean'].t).all()) and bool(torch.isnan(out['invstd'].t).all()), what
                    ds.check(st, M.STATE_KEYS, what)
                assert ds.intact() and pooled.intact() and all(o.intact() for o in out.values()), what
                assert not bool(torch.isnan(pooled.t).any()), what


@pytest.mark.parametrize('Cc', [4, 24, 256])
def test_folded_backward_finalize_equals_the_model_on_bits(Cc):
    """rdfin::bwd in the prologue of rd_up_bwd (fp32, h = w = 1), T1-T7 x nslots 0 / 8 / 24 / 64, owner and non-owner."""
    lib = L.lib()
    for ti, name in enumerate(M.FOLDED):
        for ni, nslots in enumerate((0, 8, 24, 64)):
            rng = np.random.default_rng(3000 * Cc + 10 * ti + ni)
            st, maps = M.make_state(name, Cc, rng)
            _plant_params(st, Cc, name)
            G = len(maps['rm'])
            counts = _counts(G, ti + ni)
            ns = nslots or L.STAT_SLOTS
            fslots, cb = _fwd_slots(G, Cc, counts, ns, rng)
            fw, _ = _model_fwd(st, maps, fslots, nslots, counts, cb)          # saved mean / invstd with the planted channels
            bslots = _bwd_slots(G, Cc, fw['mean'], ns, rng, fill=1e30)
            assert M.sums_exact(bslots, ns)
            want, arrs = _model_bwd(st, maps, bslots, nslots, fw['mean'], fw['invstd'], counts)
            gs = _gstart(G, ragged=(ti + ni) % 2 == 0)
            N = gs[-1]
            g2 = torch.from_numpy(rng.standard_normal((N, 2, 2, Cc)).astype(f32)).to(U.dev())
            t = torch.from_numpy(rng.standard_normal((N, 1, 1, Cc)).astype(f32)).to(U.dev())
            bd, md, isd = _dev(bslots), _dev(fw['mean']), _dev(fw['invstd'])
            ds = DevState(st, maps)
            for owner in (True, False):
                ds.load(st)
                out = _outs('PQR', G, Cc)
                dt = Guarded(4 * N * Cc, torch.float32)
                q = _bwd_desc(ds, bd, md, isd, out, Cc, counts, nslots)
                what = '%s nslots %d %s' % (name, nslots, 'owner' if owner else 'non-owner')
                L.check(lib.rd_up_bwd(L.ptr(g2), L.ptr(t), dt.ptr(), out['P'].ptr(), out['Q'].ptr(), out['R'].ptr(), N, 1, 1, Cc, G,
                                      L.gstart_array(gs), L.RD_F32, C.addressof(q), L.FIN_OWNER if owner else 0, None), what)
                torch.cuda.synchronize()
                for k in 'PQR':
                    _same(out[k].t, want[k], '%s %s' % (what, k))
                ds.check(arrs if owner else st, M.STATE_KEYS, what)
                assert ds.intact() and dt.intact() and all(o.intact() for o in out.values()), what
                assert not bool(torch.isnan(dt.t).any()), what


# ------------------------------------------------------------------------------------------------ GroupNorm(1, C)
def _exact(x):
    return Fr(float(x))


def _gn_exact_rows(G, Cc, bias, rng):
    """Per image: dyadic per-channel sums whose pooled mean and variance are exactly representable (the last channel is solved for,
    in rational arithmetic), every double product of the kernel exact.  -> forward copies, conv bias, counts, (mean, var) per image."""
    cnt = 4
    n = cnt * Cc
    cb = (rng.integers(-8, 9, Cc) / 4.0).astype(f32) if bias else None
    st = np.zeros((G, L.STAT_SLOTS, Cc, 2), f64)
    stat = []
    for g in range(G):
        m, var = Fr(int(rng.integers(-16, 17)), 8), Fr(int(rng.integers(0, 33)) if g != 1 else 0, 16)
        s1 = [Fr(int(v), 8) for v in rng.integers(-128, 129, Cc)]
        s2 = [Fr(int(v), 64) for v in rng.integers(0, 4097, Cc)]
        b = [_exact(v) for v in cb] if bias else [Fr(0)] * Cc
        last = Cc - 1
        s1[last] = n * m - sum(s1[c] + cnt * b[c] for c in range(last)) - cnt * b[last]
        s2[last] = n * (var + m * m) - sum(s2[c] + 2 * b[c] * s1[c] + cnt * b[c] * b[c] for c in range(last)) \
            - 2 * b[last] * s1[last] - cnt * b[last] * b[last]
        S1 = sum(s1[c] + cnt * b[c] for c in range(Cc))
        S2 = sum(s2[c] + 2 * b[c] * s1[c] + cnt * b[c] * b[c] for c in range(Cc))
        assert S1 / n == m and S2 / n - m * m == var and var >= 0
        assert _exact(f32(float(m))) == m and _exact(f32(float(var))) == var               # representable, so nothing rounds
        for c in range(Cc):                                # the terms and double products of the kernel: exact
            assert _exact(float(s1[c])) == s1[c] and _exact(float(s2[c])) == s2[c] and (s1[c] * 64).denominator == 1
            assert _exact(2.0 * float(b[c]) * float(s1[c])) == 2 * b[c] * s1[c] and _exact(cnt * float(b[c]) * float(b[c])) == cnt * b[c] * b[c]
        tot = np.array([[float(s1[c]), float(s2[c])] for c in range(Cc)])
        st[g] = M.spread_slots(tot, L.STAT_SLOTS, rng, span=2.0 ** 8)
        stat.append((float(m), float(var)))
    assert M.sums_exact(st, L.STAT_SLOTS)
    return st, cb, [float(cnt)] * G, stat


def _gn_launch(st, bst, cb, counts, gam, bet, start, with_db, Cc, G):
    """rd_gn_finalize_fwd, then rd_gn_finalize_bwd on the mean / invstd it left.  -> outputs as numpy, all sentinels checked."""
    lib = L.lib()
    out = _outs(('scale', 'shift', 'mean', 'invstd', 'P', 'Q', 'R'), G, Cc)
    par = {k: Guarded(4 * Cc, torch.float32) for k in ('gamma', 'beta', 'dgamma', 'dbeta', 'dbias')}
    for k, a in (('gamma', gam), ('beta', bet), ('dgamma', start[0]), ('dbeta', start[1]), ('dbias', start[2])):
        par[k].t.copy_(torch.from_numpy(a))
    sd, bd, cbd = _dev(st), _dev(bst), (_dev(cb) if cb is not None else None)
    p = L.RdBnFwd()
    p.stats, p.conv_bias = sd.data_ptr(), (cbd.data_ptr() if cb is not None else None)
    for k in ('scale', 'shift', 'mean', 'invstd'):
        setattr(p, k, out[k].ptr())
    q = L.RdBnBwd()
    q.bstats, q.mean, q.invstd, q.fstats = bd.data_ptr(), out['mean'].ptr(), out['invstd'].ptr(), sd.data_ptr()
    q.P, q.Q, q.R = out['P'].ptr(), out['Q'].ptr(), out['R'].ptr()
    q.conv_bias, q.dbias = p.conv_bias, (par['dbias'].ptr() if with_db else None)
    for g in range(G):
        p.gamma[g], p.beta[g], p.count[g] = par['gamma'].ptr(), par['beta'].ptr(), counts[g]
        q.gamma[g], q.dgamma[g], q.dbeta[g], q.count[g] = par['gamma'].ptr(), par['dgamma'].ptr(), par['dbeta'].ptr(), counts[g]
    p.C, p.G, p.eps, p.momentum, p.training, p.nslots = Cc, G, EPS, MO, 1, 0
    q.C, q.G, q.nslots = Cc, G, 0
    L.check(lib.rd_gn_finalize_fwd(C.byref(p), None), 'gn fwd')
    L.check(lib.rd_gn_finalize_bwd(C.byref(q), None), 'gn bwd')
    torch.cuda.synchronize()
    assert all(o.intact() for o in out.values()) and all(o.intact() for o in par.values())
    res = {k: o.t.cpu().numpy().reshape(G, Cc) for k, o in out.items()}
    res.update({k: par[k].t.cpu().numpy() for k in ('gamma', 'beta', 'dgamma', 'dbeta', 'dbias')})
    return res


def _one_fma_or_two_roundings(got, two, one, product, what):
    """An expression a - b * c of a kernel compiled with contraction on is ONE fma or two roundings: the value equals one of the two
    forms on bits.  Where the result is no smaller than the product the two forms are within 1 ulp of each other, and so is the value
    of the model (`two`); where the difference cancels they are half an ulp OF THE PRODUCT apart, which is any number of ulps of the
    result (measured on the MI355X: shift 0.10586128 against the model's 0.10586125, 4 ulp, the fma form), so there the two forms on
    bits are the whole assertion."""
    g, t, o = _bits(got), _bits(two), _bits(one)
    ok = (g == t) | (g == o)
    assert ok.all(), '%s: %d of %d are neither the fma form nor the two-rounding form' % (what, int((~ok).sum()), ok.size)
    plain = np.abs(np.asarray(got, f64)) >= np.abs(product)
    assert not plain.any() or np.max(M.ulp_diff(got, two)[plain]) <= 1, what
    return int(plain.sum())


GN_CASES = [(G, bias, with_db) for G in (1, 3, 16) for bias in (False, True) for with_db in (False, True)]


@pytest.mark.parametrize('Cc', [1, 24, 256, 1024])
def test_groupnorm_finalize_exact_rows(Cc):
    """mean, invstd, scale, P, dgamma, dbeta and dbias (over the image sequence, onto a non-zero start) equal the model on bits; Q is
    within 1 ulp of it; shift and R are one fma or two roundings (_one_fma_or_two_roundings: within 1 ulp of the model wherever the
    difference does not cancel).  dbias is computed from the device's own Q and R."""
    for ci, (G, bias, with_db) in enumerate(GN_CASES):
        rng = np.random.default_rng(4000 * Cc + ci)
        st, cb, counts, stat = _gn_exact_rows(G, Cc, bias, rng)
        gam = (rng.integers(-16, 17, Cc) / 8.0).astype(f32)
        bet = (0.3 * rng.standard_normal(Cc)).astype(f32)
        b1 = rng.integers(-64, 65, (G, Cc)) / 8.0
        b2 = rng.integers(-2048, 2049, (G, Cc)) / 64.0
        bst = np.zeros((G, L.STAT_SLOTS, Cc, 2), f64)
        for g in range(G):
            bst[g] = M.spread_slots(np.stack([b1[g], b2[g]], -1), L.STAT_SLOTS, rng, span=2.0 ** 8)
        assert M.sums_exact(bst, L.STAT_SLOTS)
        start = [(0.05 * rng.standard_normal(Cc)).astype(f32) for _ in range(3)]
        got = _gn_launch(st, bst, cb, counts, gam, bet, start, with_db, Cc, G)
        what = 'G %d bias %d dbias %d' % (G, bias, with_db)
        sc, sh, mean, istd = M.gn_fwd_model(st, counts, cb, gam, bet, EPS)
        for g in range(G):                                 # the model's statistics are the planted ones, exactly
            assert np.all(mean[g] == f32(stat[g][0])) and np.all(istd[g] == M.invstd_model(f32(stat[g][1]), EPS))
        _same(got['mean'], mean, what + ' mean')
        _same(got['invstd'], istd, what + ' invstd')
        _same(got['scale'], sc, what + ' scale')
        _one_fma_or_two_roundings(got['shift'], sh, M.fma_sub_f32(bet[None, :], mean, sc), mean.astype(f64) * sc, what + ' shift')
        # every double product of the backward exact: invstd (24 bits) times dyadics of few bits
        step = max(1, Cc // 24)
        for g in range(G):
            mu, is_ = _exact(mean[g, 0]), _exact(istd[g, 0])
            for c in range(0, Cc, step):
                d = _exact(b2[g, c]) - mu * _exact(b1[g, c])
                assert _exact(float(d)) == d and _exact(float(istd[g, 0]) * float(d)) == is_ * d
                assert _exact(float(gam[c]) * (float(istd[g, 0]) * float(d))) == _exact(gam[c]) * is_ * d
        dg, db, dc = start[0].copy(), start[1].copy(), (start[2].copy() if with_db else None)
        P, Q, R, R0 = M.gn_bwd_model(bst, st, mean, istd, counts, cb, gam, dg, db, dc, Q=got['Q'], R=got['R'], parts=True)
        _same(got['P'], P, what + ' P')
        assert np.max(M.ulp_diff(got['Q'], Q)) <= 1, what                  # (float64 products and a quotient, one cast: no fma to form)
        _one_fma_or_two_roundings(got['R'], R, M.fma_sub_f32(R0, got['Q'], mean), got['Q'].astype(f64) * mean, what + ' R')
        _same(got['dgamma'], dg, what + ' dgamma')
        _same(got['dbeta'], db, what + ' dbeta')
        _same(got['dbias'], dc if with_db else start[2], what + ' dbias')


@pytest.mark.parametrize('Cc', [1, 24, 256, 1024])
def test_groupnorm_finalize_random_rows(Cc):
    """Every output within the derived float32 rounding bounds (bn_fin_model: "float32 rounding bounds") of the float64 evaluation."""
    for ci, (G, bias, with_db) in enumerate(GN_CASES):
        rng = np.random.default_rng(5000 * Cc + ci)
        cnt = 4.0
        counts = [cnt] * G
        cb = (0.5 * rng.standard_normal(Cc)).astype(f32) if bias else None
        gam, bet = (1 + 0.3 * rng.standard_normal(Cc)).astype(f32), (0.3 * rng.standard_normal(Cc)).astype(f32)
        st, bst = np.zeros((G, L.STAT_SLOTS, Cc, 2), f64), np.zeros((G, L.STAT_SLOTS, Cc, 2), f64)
        ns = L.STAT_SLOTS_FOLD if ci % 2 else L.STAT_SLOTS
        for g in range(G):
            x = rng.standard_normal((4, Cc)) * 2 + rng.standard_normal(Cc)[None]          # the four pixels of the image, bias-free
            gy = rng.standard_normal((4, Cc))
            xb = x + (cb.astype(f64)[None] if bias else 0.0)
            for k in range(4):
                st[g, (k * 17) % ns, :, 0], st[g, (k * 17) % ns, :, 1] = f32(x[k]), f32(x[k] * x[k])
                bst[g, (k * 17) % ns, :, 0], bst[g, (k * 17) % ns, :, 1] = f32(gy[k]), f32(gy[k] * xb[k])
        start = [(0.05 * rng.standard_normal(Cc)).astype(f32) for _ in range(3)]
        got = _gn_launch(st, bst, cb, counts, gam, bet, start, with_db, Cc, G)
        what = 'G %d bias %d dbias %d' % (G, bias, with_db)
        terms, tb = {k: [] for k in ('dgamma', 'dbeta', 'dbias')}, {k: np.zeros(Cc) for k in ('dgamma', 'dbeta', 'dbias')}
        for g in range(G):
            s1, s2 = st[g, :, :, 0].sum(0), st[g, :, :, 1].sum(0)
            val, bnd = M.gn_exact(s1, s2, bst[g, :, :, 0].sum(0), bst[g, :, :, 1].sum(0), s1, cnt, cb, gam, bet, EPS)
            for k in ('mean', 'invstd', 'scale', 'shift', 'P', 'Q', 'R'):
                err = np.abs(got[k][g].astype(f64) - val[k])
                assert np.all(err <= bnd[k]), '%s %s image %d: %.3g of the bound' % (what, k, g, np.max(err / np.maximum(bnd[k], 1e-300)))
            for k in terms:
                terms[k].append(val[k])
                tb[k] += bnd[k]
        for i, k in enumerate(('dgamma', 'dbeta', 'dbias')):
            if k == 'dbias' and not with_db:
                _same(got[k], start[i], what + ' dbias untouched')
                continue
            total, ab = M.accumulate_bound(terms[k])
            final = total + start[i].astype(f64)
            bound = tb[k] + ab + M.SLACK * M.U32 * np.abs(final)
            err = np.abs(got[k].astype(f64) - final)
            assert np.all(err <= bound), '%s %s: %.3g of the bound' % (what, k, np.max(err / np.maximum(bound, 1e-300)))


def test_groupnorm_backward_refuses_more_than_1024_channels():
    """C = 1025 (more than CPT channels per thread cover): -1, nothing launched, nothing touched."""
    G, Cc = 2, 1025
    out = _outs('PQR', G, Cc)
    dg = Guarded(4 * Cc, torch.float32)
    gam = torch.ones(Cc, device=U.dev())
    mi = torch.ones(G, Cc, device=U.dev())
    bst = torch.zeros(G, L.STAT_SLOTS, Cc, 2, dtype=torch.float64, device=U.dev())
    q = L.RdBnBwd()
    q.bstats, q.mean, q.invstd = bst.data_ptr(), mi.data_ptr(), mi.data_ptr()
    q.P, q.Q, q.R = out['P'].ptr(), out['Q'].ptr(), out['R'].ptr()
    for g in range(G):
        q.gamma[g], q.dgamma[g], q.dbeta[g], q.count[g] = gam.data_ptr(), dg.ptr(), dg.ptr(), 4.0
    q.C, q.G = Cc, G
    assert L.lib().rd_gn_finalize_bwd(C.byref(q), None) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o.t).all()) and o.intact() for o in out.values()) and bool(torch.isnan(dg.t).all()) and dg.intact()
