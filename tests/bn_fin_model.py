"""The numpy model of the BatchNorm and GroupNorm finalize (csrc/bn_fin.h fwd_stat / fwd_coef / momentum_step / bwd_stat / bwd_coef,
shared by the explicit kernels of csrc/bn.hip and the folded prologue; gn_finalize_fwd_kernel / gn_finalize_bwd_kernel): every
float32 operation rounded on its own, in the order of the source.  Test infrastructure, numpy only.

The slot sums and the forward statistics are ramdsir.avg_bn's slot_sums_model / fwd_stat_model (what rd_bn_recal is held to); this
module adds invstd, the coefficients, the running-statistics recursion, the backward and GroupNorm.

Pointer identity is OBJECT identity: the `*_of` arguments are lists with one numpy array (or None = a NULL pointer) per group, and
two groups that name the same array object share that buffer.  Arrays are updated in place, as the kernels update the buffers.

What is bit-exact:
  fwd_model / bwd_model   every output, on any data whose slot sums are exact in float64 (order-independent: the explicit kernels add
                          by wave butterfly, the folded code slot after slot).  The kernels are compiled with contraction off and their
                          divisions and 1 / sqrt are the correctly rounded sequences, as numpy's are.
  gn_fwd_model            mean, invstd, scale on "exact rows" (the pooled sums, mean and variance exactly representable; every double
                          product exact).  shift = beta - mean * scale is one expression of a kernel compiled with contraction ON:
                          one fma (fma_sub_f32) or two roundings (the model) -- the device value is one of the two on bits.  The two
                          are within 1 ulp of each other where the result is no smaller than the product; where the difference
                          cancels they are half an ulp of the PRODUCT apart, which is several ulps of the result.
  gn_bwd_model            P, dgamma, dbeta on exact rows; Q within 1 ulp; R = float32(..) - Q * mu as shift; dbias bit-exact when the
                          model is fed the device's own Q and R (Q=..., R=...), since dbias is computed from them.
  On other data the GroupNorm models are a float64 evaluation in one particular order and are compared within rounding bounds."""
import numpy as np

from ramdsir import _lib as L
from ramdsir.avg_bn import fwd_stat_model, slot_sums_model

f32, f64 = np.float32, np.float64
STAT_SLOTS = L.STAT_SLOTS


def _ns(nslots):
    return int(nslots) if int(nslots) > 0 else STAT_SLOTS


def invstd_model(var, eps):
    """1.0f / sqrtf(var + eps): three float32 operations, each correctly rounded."""
    with np.errstate(all='ignore'):
        t = (np.asarray(var, f32) + f32(eps)).astype(f32)
        return (f32(1) / np.sqrt(t).astype(f32)).astype(f32)


def fwd_coef_model(gamma, beta, mean, invstd):
    """fwd_coef: scale = gamma * invstd; shift = beta - (mean * scale) -- two roundings, no fma."""
    with np.errstate(all='ignore'):
        sc = (np.asarray(gamma, f32) * np.asarray(invstd, f32)).astype(f32)
        t = (np.asarray(mean, f32) * sc).astype(f32)
        return sc, (np.asarray(beta, f32) - t).astype(f32)


def momentum_step_model(old, x, mo):
    """momentum_step: (1 - mo) * old + mo * x as four float32 roundings."""
    mo = f32(mo)
    with np.errstate(all='ignore'):
        om = f32(f32(1) - mo)
        a = (om * np.asarray(old, f32)).astype(f32)
        b = (mo * np.asarray(x, f32)).astype(f32)
        return (a + b).astype(f32)


def _distinct(objs):
    """(object, [groups that name it]) in order of first appearance; None skipped."""
    out = []
    for g, o in enumerate(objs):
        if o is None:
            continue
        for p, gs in out:
            if p is o:
                gs.append(g)
                break
        else:
            out.append((o, [g]))
    return out


def fwd_model(slots, nslots, count, conv_bias, gamma_of, beta_of, rm_of, rv_of, nbt_of, eps, momentum, training, invstd=None):
    """rd_bn_finalize_fwd / rdfin::fwd.  slots [G][RD_STAT_SLOTS][C][2] float64 -> scale, shift, mean, invstd [G][C] float32; the
    running arrays and counters are updated in place (training) or left alone (training = 0: mean = running_mean or 0, invstd from
    running_var or 1, the slots are not read).  The running recursion runs in group order along each chain of groups that name the
    same running_mean object; running_var follows running_mean (the kernels identify a BatchNorm by its running_mean pointer alone,
    so the model refuses a running_var shared differently).  invstd: [G][C] to use INSTEAD of the model's own (the device's values,
    where a device's 1 / sqrt turned out not to be correctly rounded: everything downstream is then still held on bits)."""
    G = len(count)
    C = np.asarray(gamma_of[0]).shape[0]
    cb = None if conv_bias is None else np.asarray(conv_bias, f32)
    mean, istd, unb = np.zeros((G, C), f32), np.zeros((G, C), f32), np.zeros((G, C), f32)
    for g in range(G):
        assert (rm_of[g] is None) == (rv_of[g] is None)
        for j in range(g):
            assert (rm_of[g] is rm_of[j]) == (rv_of[g] is rv_of[j]) or rm_of[g] is None or rm_of[j] is None
        if training:
            s1, s2 = slot_sums_model(slots[g], _ns(nslots))
            mean[g], unb[g], var = fwd_stat_model(s1, s2, count[g], cb, with_var=True)
            istd[g] = invstd_model(var, eps)
        else:
            mean[g] = 0 if rm_of[g] is None else np.asarray(rm_of[g], f32)
            istd[g] = invstd_model(np.ones(C, f32) if rv_of[g] is None else rv_of[g], eps)
    if invstd is not None:
        istd = np.asarray(invstd, f32).reshape(G, C).copy()
    scale, shift = np.zeros((G, C), f32), np.zeros((G, C), f32)
    for g in range(G):
        scale[g], shift[g] = fwd_coef_model(gamma_of[g], beta_of[g], mean[g], istd[g])
    if training:
        for g in range(G):                                 # in place, in group order: a chain continues from its predecessor
            if rm_of[g] is None:
                continue
            rm_of[g][...] = momentum_step_model(rm_of[g], mean[g], momentum)
            rv_of[g][...] = momentum_step_model(rv_of[g], unb[g], momentum)
        for o, gs in _distinct(nbt_of):
            o[...] = o + len(gs)
    return scale, shift, mean, istd


def bwd_stat_model(s1d, sgzd, mu, istd):
    """bwd_stat: s1 = float32(s1d); s2 = invstd * float32(sgzd - double(mu) * s1d), the product and difference in float64."""
    with np.errstate(all='ignore'):
        s1d, sgzd = np.asarray(s1d, f64), np.asarray(sgzd, f64)
        t = np.asarray(mu, f32).astype(f64) * s1d
        d = (sgzd - t).astype(f32)
        return s1d.astype(f32), (np.asarray(istd, f32) * d).astype(f32)


def bwd_coef_model(gamma, istd, mu, s1, s2, count):
    """bwd_coef: P = gamma * is; Q = (((-gamma) * is) * is) * s2 / cnt; R = ((-P) * s1) / cnt - (Q * mu), float32 throughout."""
    gamma, istd, mu, cnt = np.asarray(gamma, f32), np.asarray(istd, f32), np.asarray(mu, f32), f32(count)
    with np.errstate(all='ignore'):
        P = (gamma * istd).astype(f32)
        q = ((-gamma) * istd).astype(f32)
        q = (q * istd).astype(f32)
        q = (q * s2).astype(f32)
        Q = (q / cnt).astype(f32)
        r = ((-P) * s1).astype(f32)
        r = (r / cnt).astype(f32)
        t = (Q * mu).astype(f32)
        return P, Q, (r - t).astype(f32)


def bwd_model(bslots, nslots, mean, invstd, count, gamma_of, dgamma_of, dbeta_of):
    """rd_bn_finalize_bwd / rdfin::bwd.  bslots [G][RD_STAT_SLOTS][C][2] float64 (sum g, sum g z), mean / invstd [G][C] -> P, Q, R
    [G][C] float32; dgamma += sum g zhat and dbeta += sum g as float32 additions in group order onto the old content, each pointer
    array on its own."""
    G = len(count)
    mean, invstd = np.asarray(mean, f32), np.asarray(invstd, f32)
    C = mean.shape[1]
    P, Q, R = (np.zeros((G, C), f32) for _ in range(3))
    for g in range(G):
        s1d, sgzd = slot_sums_model(bslots[g], _ns(nslots))
        s1, s2 = bwd_stat_model(s1d, sgzd, mean[g], invstd[g])
        P[g], Q[g], R[g] = bwd_coef_model(gamma_of[g], invstd[g], mean[g], s1, s2, count[g])
        with np.errstate(all='ignore'):
            if dgamma_of[g] is not None:
                dgamma_of[g][...] = (dgamma_of[g] + s2).astype(f32)
            if dbeta_of[g] is not None:
                dbeta_of[g][...] = (dbeta_of[g] + s1).astype(f32)
    return P, Q, R


# ------------------------------------------------------------------------------------------------ GroupNorm(1, C)
def _gn_block_sum(per_channel, nthreads=256):
    """Sum over the channels as the kernels do: thread t adds channels t, t + 256, ... in order, then the threads are added (the
    kernels: wave butterfly, then the four waves in order).  Exact rows do not depend on the order; other rows are compared within
    bounds."""
    v = np.asarray(per_channel, f64)
    acc = np.zeros(nthreads, f64)
    for c0 in range(0, v.shape[0], nthreads):
        part = v[c0:c0 + nthreads]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    o = 32
    w = acc.reshape(-1, 64).copy()
    while o:                                               # wave_sum_d: xor butterfly
        w = w + w[:, np.arange(64) ^ o]
        o >>= 1
    r = f64(0)
    for i in range(w.shape[0]):
        r = r + w[i, 0]
    return r


def gn_fwd_model(slots, count, conv_bias, gamma, beta, eps):
    """rd_gn_finalize_fwd: one statistics group per image, mean / variance pooled over (C, H, W).  slots [G][RD_STAT_SLOTS][C][2]
    (all RD_STAT_SLOTS copies are read: the kernel has no nslots), gamma / beta [C] -> scale, shift, mean, invstd [G][C] float32.
    float64 where the kernel is: S1 = sum_c (s1 + cnt b), S2 = sum_c (s2 + 2 b s1 + cnt b b), m = S1 / n, var = max(S2 / n - m m, 0)."""
    G = len(count)
    gamma, beta = np.asarray(gamma, f32), np.asarray(beta, f32)
    C = gamma.shape[0]
    scale, shift, mean, istd = (np.zeros((G, C), f32) for _ in range(4))
    for g in range(G):
        cnt = f64(f32(count[g]))
        s1, s2 = slot_sums_model(slots[g], STAT_SLOTS)
        b = np.zeros(C, f64) if conv_bias is None else np.asarray(conv_bias, f32).astype(f64)
        S1 = _gn_block_sum(s1 + cnt * b)
        S2 = _gn_block_sum((s2 + (2.0 * b) * s1) + (cnt * b) * b)
        n = cnt * f64(C)
        m = S1 / n
        vard = S2 / n - m * m
        vard = max(vard, 0.0)
        mean[g] = f32(m)
        istd[g] = invstd_model(np.full(C, f32(vard), f32), eps)
        scale[g], shift[g] = fwd_coef_model(gamma, beta, mean[g], istd[g])
    return scale, shift, mean, istd


def gn_bwd_model(bslots, fslots, mean, invstd, count, conv_bias, gamma, dgamma, dbeta, dbias, Q=None, R=None, parts=False):
    """rd_gn_finalize_bwd: the images in order.  mean / invstd [G][C] (the same for every channel of an image: element [g][0] is
    read), gamma [C]; dgamma / dbeta / dbias: [C] arrays updated in place, or None.  Per image the float32 sums dg += float32(sum g
    zhat), db += float32(sum g), dcb += float32(P b1 + Q sz + R cnt) start from 0 and are added to the old content once, at the end.
    Q: [G][C] to use for R and dbias, R: [G][C] to use for dbias, INSTEAD of the model's own (the device's: R may differ from the
    model's by the fma).  -> P, Q (the model's own), R = R0 - float32(Q mu) in two roundings; parts: R0 = float32(-is A / n) as well."""
    G = len(count)
    mean, invstd, gamma = np.asarray(mean, f32), np.asarray(invstd, f32), np.asarray(gamma, f32)
    C = gamma.shape[0]
    P, Qm, Rm, R0 = (np.zeros((G, C), f32) for _ in range(4))
    dg, db, dcb = (np.zeros(C, f32) for _ in range(3))
    gd = gamma.astype(f64)
    with np.errstate(all='ignore'):
        for g in range(G):
            mu, is_ = mean[g, 0], invstd[g, 0]
            mud, isd, cnt = f64(mu), f64(is_), f64(f32(count[g]))
            b1, b2 = slot_sums_model(bslots[g], STAT_SLOTS)
            b2 = isd * (b2 - mud * b1)
            A = _gn_block_sum(gd * b1)
            B = _gn_block_sum(gd * b2)
            n = cnt * f64(C)
            q = f32(((-isd) * isd) * B / n)
            r0 = f32((-isd) * A / n)
            Qm[g], R0[g] = q, r0
            qu = Qm[g] if Q is None else np.asarray(Q, f32).reshape(G, C)[g]
            Rm[g] = (R0[g] - (qu * mu).astype(f32)).astype(f32)
            P[g] = (gamma * is_).astype(f32)
            dg = (dg + b2.astype(f32)).astype(f32)
            db = (db + b1.astype(f32)).astype(f32)
            if dbias is not None:
                sz, _ = slot_sums_model(fslots[g], STAT_SLOTS)
                if conv_bias is not None:
                    sz = sz + cnt * np.asarray(conv_bias, f32).astype(f64)
                ru = Rm[g] if R is None else np.asarray(R, f32).reshape(G, C)[g]
                t = (P[g].astype(f64) * b1 + qu.astype(f64) * sz) + ru.astype(f64) * cnt
                dcb = (dcb + t.astype(f32)).astype(f32)
        if dgamma is not None:
            dgamma[...] = (dgamma + dg).astype(f32)
        if dbeta is not None:
            dbeta[...] = (dbeta + db).astype(f32)
        if dbias is not None:
            dbias[...] = (dbias + dcb).astype(f32)
    return (P, Qm, Rm, R0) if parts else (P, Qm, Rm)


def _fraction_to_f32(x):
    """A rational, correctly rounded to float32 (one rounding, half to even)."""
    from fractions import Fraction as Fr
    if x == 0:
        return f32(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    if Fr(2) ** (e + 1) <= a:
        e += 1
    q = max(e - 23, -149)
    v = float(round(a / Fr(2) ** q)) * 2.0 ** q
    return f32(-v if x < 0 else v)


def fma_sub_f32(a, b, c):
    """float32(a - b * c) with ONE rounding (what an fma gives), elementwise on float32 arrays: the product is exact in float64, the
    difference is taken with its exact error term (TwoSum), and where that is not zero the element is redone in rationals."""
    from fractions import Fraction as Fr
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    x, y = a.astype(f64), -(b.astype(f64) * c.astype(f64))
    s = x + y
    bb = s - x
    err = (x - (s - bb)) + (y - bb)
    out = s.astype(f32)
    for i in zip(*np.nonzero(err != 0)):
        out[i] = _fraction_to_f32(Fr(float(a[i])) - Fr(float(b[i])) * Fr(float(c[i])))
    return out


def ulp_diff(a, b):
    """|a - b| in units in the last place of float32, by the ordered-integer map (-0 = +0); inf where either is not finite."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib).astype(f64)
    return np.where(np.isfinite(a) & np.isfinite(b), d, np.inf)


# ------------------------------------------------------------------------------------------------ topologies and state
# One module index per group; None: every per-group pointer of that group is NULL except gamma / beta.  Keys other than `mod` share
# that pointer array differently from the rest (the kernels treat each pointer array on its own).
TOPOLOGIES = {
    'T1': dict(mod=[0]),
    'T2': dict(mod=[0, 0]),                                # the seg network
    'T3': dict(mod=[0, 1, 2, 3, 4]),                       # DSBN, five domains
    'T4': dict(mod=[0, 0, 0]),                             # chain of three
    'T5': dict(mod=[0, 1, 0, 1, 0]),                       # interleaved chains
    'T6': dict(mod=[0, 1, 1, 2, 0, 3, 0, 1]),              # G = FIN_MAX_G; two chains of three
    'T7': dict(mod=[None, 0, None, 0]),                    # NULL groups inside a chain
    'T8': dict(mod=[None] * 16, instnorm=True),            # the InstanceNorm contract: gamma -> ones, beta -> zeros, all else NULL
    'T9': dict(mod=[0] * 16),                              # chain of sixteen
    'T10': dict(mod=[0, 1, 2], dgamma=[0, 0, 1], dbeta=[0, 1, 1], rm=[0, 1, 1], nbt=[0, 0, 1]),
}
FOLDED = ('T1', 'T2', 'T3', 'T4', 'T5', 'T6', 'T7')        # G <= FIN_MAX_G
STATE_KEYS = ('gamma', 'beta', 'rm', 'rv', 'nbt', 'dgamma', 'dbeta')


def topo_maps(name):
    """{array name: [module index or None per group]}; rv follows rm; gamma / beta are never None (a NULL group gets its own)."""
    t = TOPOLOGIES[name]
    mod = t['mod']
    G = len(mod)
    maps = {k: list(t.get(k, mod)) for k in ('rm', 'nbt', 'dgamma', 'dbeta')}
    maps['rv'] = list(maps['rm'])
    own = [m if m is not None else 100 + g for g, m in enumerate(mod)]
    maps['gamma'] = [0] * G if t.get('instnorm') else own
    maps['beta'] = list(maps['gamma'])
    return maps


def make_state(name, C, rng):
    """Non-trivial starting state for a topology: ({key: {module index: array}}, maps): random gamma / beta / running statistics /
    dgamma / dbeta, num_batches_tracked = 3 (the InstanceNorm contract: gamma ones, beta zeros).  Callers plant channels on top."""
    maps = topo_maps(name)
    inst = TOPOLOGIES[name].get('instnorm', False)
    gen = dict(gamma=lambda: ((1.0 + 0.2 * rng.standard_normal(C)).astype(f32) if not inst else np.ones(C, f32)),
               beta=lambda: ((0.3 * rng.standard_normal(C)).astype(f32) if not inst else np.zeros(C, f32)),
               rm=lambda: (0.1 * rng.standard_normal(C)).astype(f32), rv=lambda: (1.0 + 0.1 * rng.random(C)).astype(f32),
               nbt=lambda: np.array(3, np.int64), dgamma=lambda: (0.05 * rng.standard_normal(C)).astype(f32),
               dbeta=lambda: (0.05 * rng.standard_normal(C)).astype(f32))
    st = {k: {} for k in STATE_KEYS}
    for k in STATE_KEYS:
        for m in maps[k]:
            if m is not None and m not in st[k]:
                st[k][m] = gen[k]()
    return st, maps


def state_lists(st, maps, copy=True):
    """The `*_of` lists of the model from a state: one array object per module (shared by identity), None where the map says NULL."""
    arrs = {k: {m: (a.copy() if copy else a) for m, a in st[k].items()} for k in STATE_KEYS}
    return {k: [None if m is None else arrs[k][m] for m in maps[k]] for k in STATE_KEYS}, arrs


def spread_slots(total, nslots, rng, step=2.0 ** -6, span=2.0 ** 12):
    """[C] float64 totals -> [RD_STAT_SLOTS][C] with the first `nslots` copies summing to `total` exactly in any order: every copy is
    a multiple of `step` below `span` in magnitude beside the remainder in copy 0 (the caller's totals are multiples of step)."""
    total = np.asarray(total, f64)
    out = np.zeros((STAT_SLOTS,) + total.shape, f64)
    if nslots > 1:
        out[1:nslots] = np.round(rng.uniform(-span, span, (nslots - 1,) + total.shape) / step) * step
    out[0] = total - out[1:nslots].sum(0)
    return out


def sums_exact(slots, nslots):
    """The exactness the bit equalities rest on, checked on the host: for every sum of slots [G][RD_STAT_SLOTS][C][2], math.fsum of
    the first `nslots` copies equals their float64 sum in slot order (the folded code), in reverse order, and by halving tree (the
    explicit kernels' butterfly over RD_STAT_SLOTS copies)."""
    import math
    v = np.asarray(slots, f64)
    v = v[:, :nslots].reshape(v.shape[0], nslots, -1)
    seq, rev = np.zeros((v.shape[0], v.shape[2]), f64), np.zeros((v.shape[0], v.shape[2]), f64)
    for k in range(nslots):
        seq = seq + v[:, k]
        rev = rev + v[:, nslots - 1 - k]
    t = np.zeros((v.shape[0], STAT_SLOTS, v.shape[2]), f64)
    t[:, :nslots] = v
    while t.shape[1] > 1:
        h = t.shape[1] // 2
        t = t[:, :h] + t[:, h:]
    if not (np.array_equal(seq, rev) and np.array_equal(seq, t[:, 0])):
        return False
    return all(math.fsum(v[g, :, i]) == seq[g, i] for g in range(v.shape[0]) for i in range(v.shape[2]))


# ------------------------------------------------------------------------------------------------ float32 rounding bounds
# u = 2^-24, the unit roundoff of float32.  Each bound below: the number of float32 roundings on the path of the output times u, against
# the magnitude the rounding acts on (for differences: the SUM of the magnitudes of the terms), times 2 for ulp granularity (a bound in
# u on a value just above a power of two is half as many ulps as just below).  float64 roundings (2^-53) are below 1e-8 u each on the
# data of these tests (|mean| <= 16 sigma) and are not counted.
U32 = 2.0 ** -24
SLACK = 2.0
#   mean   = float32(m0 + bias)                                            1 rounding             1 u |mean|
#   invstd = 1 / sqrt(float32(var) + eps): cast, add, sqrt (halves what precedes it), divide:      (1 + 1) / 2 + 1 + 1 = 3 <= 4 u |invstd|
#   scale  = gamma * invstd                                                4 + 1                  5 u |scale|
#   shift  = beta - mean * scale: the product carries mean (1) + scale (5) + 1 = 7 u, the difference 1 u of |beta| + |mean scale|
#                                                                                                  8 u (|beta| + |mean scale|)
#   running (one step) = (1 - mo) * old + mo * x: (1 - mo) rounded, product: 2 u |om old|; x carries 1 u, product: 2 u |mo x|; the sum
#            1 u more on both                                                                      3 u (|om old| + |mo x|), summed over a chain
#   P      = gamma * invstd                                                                        5 u |P|
#   s2     = invstd * float32(sgz - mu s1): mu carries 1 u into the product, the cast 1 u, invstd 4 u, the product 1 u
#                                                                                                  7 u invstd D,  D = |sgz| + |mu s1|
#   Q      = -gamma * is * is * s2 / cnt: is twice (8 u), four operations (4 u), s2 (7 u)          19 u Qmag,  Qmag = |gamma| is^3 D / cnt
#   R      = -P * s1 / cnt - Q * mu: first term P (5) + cast of s1 (1) + 2 operations = 8 u |T1|; second term Q (19 u Qmag |mu|) + mu
#            (1 u) + product (1 u) <= 21 u Qmag |mu|; the difference 1 u of both                   9 u |T1| + 22 u Qmag |mu|
FWD_ROUNDINGS = dict(mean=1, invstd=4, scale=5, shift=8, running=3)
BWD_ROUNDINGS = dict(P=5, s2=7, Q=19, R_t1=9, R_t2=22, s1=1)


def bn_fwd_bounds(gamma, beta, mean, invstd):
    """Bounds on |model - exact| for one group from the exact (float64) values."""
    gamma, beta, mean, invstd = (np.asarray(a, f64) for a in (gamma, beta, mean, invstd))
    sc = gamma * invstd
    k = SLACK * U32
    return dict(mean=k * 1 * np.abs(mean), invstd=k * 4 * np.abs(invstd), scale=k * 5 * np.abs(sc),
                shift=k * 8 * (np.abs(beta) + np.abs(mean * sc)))


def bn_bwd_exact(gamma, mean, invstd, s1, sgz, count):
    """The exact (float64) backward coefficients of one group and the bounds on |model - exact|.  mean / invstd: the exact ones."""
    gamma, mean, invstd, s1, sgz = (np.asarray(a, f64) for a in (gamma, mean, invstd, s1, sgz))
    cnt = float(count)
    s2 = invstd * (sgz - mean * s1)
    P = gamma * invstd
    Q = -gamma * invstd * invstd * s2 / cnt
    T1 = -P * s1 / cnt
    R = T1 - Q * mean
    D = np.abs(sgz) + np.abs(mean * s1)
    Qmag = np.abs(gamma) * invstd ** 3 * D / cnt
    k = SLACK * U32
    return dict(P=P, Q=Q, R=R, s1=s1, s2=s2), dict(P=k * 5 * np.abs(P), Q=k * 19 * Qmag, R=k * (9 * np.abs(T1) + 22 * Qmag * np.abs(mean)),
                                                   s2=k * 7 * invstd * D, s1=k * 1 * np.abs(s1))


# GroupNorm (the sums, mean and variance are float64 in the kernel; float32 enters with mean, invstd, gamma and the casts):
#   mean 1 u, invstd 4 u, scale 5 u, shift 8 u (|beta| + |mean scale|) as above
#   P      5 u |P|
#   Q      = float32(-is is B / n), B = sum_c gamma is (b2 - mu b1): is three times (12 u), mu (1 u on the mu b1 part), the cast (1 u)
#                                                                                                  14 u Qmag,  Qmag = is^3 sum_c |gamma| (|b2| + |mu b1|) / n
#   R      = float32(-is A / n) - Q mu: first term is (4) + cast (1) = 5 u |T1|; second Q (14 u Qmag |mu|) + mu (1) + product (1); the
#            difference (or fma) 1 u of both                                                       6 u |T1| + 17 u Qmag |mu|
#   dgamma, per image float32(is (b2 - mu b1)): is 4 u + mu 1 u + cast 1 u <= 6 u is D_c; each float32 addition 1 u of its partial sum
#   dbeta,  per image float32(b1): 1 u |b1|; additions likewise
#   dbias,  per image float32(P b1 + Q sz + R cnt): 5 u |P b1| + err(Q) |sz| + err(R) cnt + the cast 1 u of the three magnitudes;
#           additions likewise
def gn_exact(s1, s2, b1, b2, sz, count, conv_bias, gamma, beta, eps):
    """GroupNorm(1, C) of one image in float64 from the per-channel sums of the bias-free conv result (s1, s2, sz = s1 of the forward)
    and of the gradient (b1 = sum g, b2 = sum g z): exact values and bounds.  Returns (values, bounds): mean, invstd, scale, shift
    [C]; P [C], Q, R scalars; the per-image terms dgamma, dbeta, dbias [C]."""
    s1, s2, b1, b2, sz, gamma, beta = (np.asarray(a, f64) for a in (s1, s2, b1, b2, sz, gamma, beta))
    C = gamma.shape[0]
    cnt = float(count)
    b = np.zeros(C) if conv_bias is None else np.asarray(conv_bias, f64)
    n = cnt * C
    m = float(np.sum(s1 + cnt * b)) / n
    var = max(float(np.sum(s2 + 2.0 * b * s1 + cnt * b * b)) / n - m * m, 0.0)
    is_ = 1.0 / np.sqrt(var + float(f32(eps)))
    sc = gamma * is_
    val = dict(mean=np.full(C, m), invstd=np.full(C, is_), scale=sc, shift=beta - m * sc)
    k = SLACK * U32
    bnd = dict(mean=k * 1 * np.abs(val['mean']), invstd=k * 4 * val['invstd'], scale=k * 5 * np.abs(sc),
               shift=k * 8 * (np.abs(beta) + np.abs(m * sc)))
    gz = is_ * (b2 - m * b1)                               # sum g zhat per channel
    A, B = float(np.sum(gamma * b1)), float(np.sum(gamma * gz))
    P = gamma * is_
    Q = -is_ * is_ * B / n
    T1 = -is_ * A / n
    R = T1 - Q * m
    Dc = np.abs(b2) + np.abs(m * b1)
    Qmag = is_ ** 3 * float(np.sum(np.abs(gamma) * Dc)) / n
    eQ, eR = 14 * Qmag, 6 * abs(T1) + 17 * Qmag * abs(m)
    szb = sz + cnt * b
    val.update(P=P, Q=np.full(C, Q), R=np.full(C, R), dgamma=gz, dbeta=b1, dbias=P * b1 + Q * szb + R * cnt)
    bnd.update(P=k * 5 * np.abs(P), Q=np.full(C, k * eQ), R=np.full(C, k * eR), dgamma=k * 6 * is_ * Dc, dbeta=k * 1 * np.abs(b1),
               dbias=k * (5 * np.abs(P * b1) + eQ * np.abs(szb) + eR * cnt + (np.abs(P * b1) + np.abs(Q * szb) + abs(R) * cnt)))
    return val, bnd


def accumulate_bound(terms, start=None):
    """Bound on the float32 summation of `terms` [K][C] (exact values) in order onto `start`: 1 u of every partial sum (times SLACK)."""
    part = np.zeros(np.asarray(terms[0]).shape, f64) if start is None else np.asarray(start, f64).copy()
    bnd = np.zeros(part.shape, f64)
    for t in terms:
        part = part + np.asarray(t, f64)
        bnd = bnd + SLACK * U32 * np.abs(part)
    return part, bnd
