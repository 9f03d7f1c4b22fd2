"""-m gpu: bit-exact parity on integer data.  The tolerance tests (test_gpu_ops.py, test_gpu_fused_bwd.py) compare bf16 kernels with
max|diff| <= 4e-2 x RMS, which cannot see one dropped pixel of a weight gradient or one dropped term at a tile seam.  Here every
tensor holds small integers and every coefficient is dyadic (exact_util.py): every product is exact, every accumulation is exact
while its |terms| sum to less than 2^24 quanta (asserted on the reference, per accumulated quantity), and the result depends neither
on summation order nor on atomics, MFMA k-order or how tiles are dealt to workgroups.  The kernels, called through the C ABI on the
geometries of the tolerance tests, then have to match the fp64 torch reference BIT FOR BIT -- in bf16 as in fp32 -- after the one
round-to-nearest-even into the storage type (torch.equal: every value identical, a zero of either sign being a zero).  The data is full of exact zeros and ties: the activation derivative at 0
(x > 0 ? 1 : slope, as ATen) and the first maximum of a pool window are exercised over whole tensors."""
import ctypes as C
import functools
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ramdsir import _lib as L                                                   # noqa: E402
import gpu_util as U                                                            # noqa: E402
import exact_util as X                                                          # noqa: E402
from test_gpu_ops import FWD_CASES, GRAD_CASES, ROW_BLOCK_CASES, WG_CASES, _conv_desc   # noqa: E402
from test_gpu_fused_bwd import CASES as FUSED_CASES                             # noqa: E402

DTYPES = ['f32', 'bf16']
DENSITIES = [1.0, 0.25, 0.0625]
MAX_FALLBACK_CASES = 6
_BY_NAME = lambda cases: {c[0]: c for c in cases}


def _seed(name, k=0):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000 + 7 * k)


def _src_dims(mode, H, W):
    return (2 * H, 2 * W) if mode == L.SRC_POOL else ((H // 2, W // 2) if mode == L.SRC_UP else (H, W))


def _stats_dev(G, Cc):
    return torch.zeros(G, L.STAT_SLOTS, Cc, 2, dtype=torch.float64, device=U.dev())


def _storage(ref_nchw, dtype):
    """The NHWC storage-dtype tensor a kernel must have written for the exact NCHW fp64 result."""
    return X.to_storage(ref_nchw.permute(0, 2, 3, 1).contiguous(), U.DT[dtype][1])


def _rows(p, gstart, N):
    return U.group_rows(p, gstart, N)


# ------------------------------------------------------------------------------------ conv forward
@functools.lru_cache(maxsize=None)
def _fwd_data(name, density):
    """Host data and fp64 reference of one forward case (shared by both dtypes; never modified).  `stats_ratio` is the larger of the two
    statistics sums against the 2^24-quanta cap: the sums are compared only where it is below 1."""
    _, taps, src_spec, Cout, N, H, W, gstart, slope = _BY_NAME(FWD_CASES)[name]
    gen = _seed(name)
    G = len(gstart) - 1
    sl = X.slope(slope)
    xs, virt = [], []
    for mode, Cc in src_spec:
        hs, ws = _src_dims(mode, H, W)
        x = X.stored((N, Cc, hs, ws), gen)
        sc, sh = X.scale((G, Cc), gen), X.shift((G, Cc), gen)
        xs.append((x, sc, sh))
        virt.append(U.virtual_input(x, mode, sc, sh, sl, gstart))
    a = torch.cat(virt, 1)
    k = 3 if taps == 9 else 1
    w = X.weights((Cout, a.shape[1], k, k), gen, density)
    bias = X.bias(Cout, gen)
    o = F.conv2d(a, w, None, padding=k // 2)
    X.assert_exact_in_fp32(F.conv2d(a.abs(), w.abs(), None, padding=k // 2) + bias.abs().max(), [a, bias], name + ' out')
    ratio = max(X.exact_ratio(X.group_sums(o.abs(), gstart), o), X.exact_ratio(X.group_sums(o * o, gstart), o * o))
    return dict(xs=xs, w=w, bias=bias, slope=sl, out=o + bias[None, :, None, None], stats=X.pair_sums(o, o * o, gstart),
                stats_ratio=ratio)


def _stats_density(name):
    """The first density at which the statistics sums of the case are exact in fp32; a case must hold at 1/16."""
    for d in DENSITIES:
        if _fwd_data(name, d)['stats_ratio'] < 1.0:
            return d
    raise AssertionError('%s: the statistics sums are not exact in fp32 even at weight density 1/16 (%.3g x the cap)'
                         % (name, _fwd_data(name, DENSITIES[-1])['stats_ratio']))


def _run_forward(name, dtype, density, check_stats, cu_limit=0, stat_slots=0):
    _, taps, src_spec, Cout, N, H, W, gstart, _ = _BY_NAME(FWD_CASES)[name]
    d = _fwd_data(name, density)
    keep = U.Keep()
    G = len(gstart) - 1
    srcs = [U.make_src(keep, x, mode, dtype, sc, sh, d['slope']) for (mode, Cc), (x, sc, sh) in zip(src_spec, d['xs'])]
    p = _conv_desc(keep, srcs, d['w'], d['bias'], N, H, W, gstart, dtype, taps)
    out = torch.full((N, H, W, Cout), float('nan'), dtype=U.DT[dtype][1], device=U.dev())
    stats = _stats_dev(G, Cout)
    p.emode, p.out, p.stats, p.cu_limit, p.stat_slots = 0, out.data_ptr(), stats.data_ptr(), cu_limit, stat_slots
    what = '%s %s density %g cu_limit %d stat_slots %d' % (name, dtype, density, cu_limit, stat_slots)
    L.check(L.lib().rd_conv(C.byref(p), U.DT[dtype][0], None), what)
    torch.cuda.synchronize()
    X.assert_bits_equal(out, _storage(d['out'], dtype), what + ' out', nhwc=True)
    if check_stats:
        assert d['stats_ratio'] < 1.0
        if stat_slots:
            assert float(stats[:, stat_slots:].abs().max()) == 0.0, what + ': copies %d.. must stay zero' % stat_slots
        X.assert_bits_equal(stats.sum(1), d['stats'], what + ' stats')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_exact_conv_forward(case, dtype):
    """out == RNE(conv2d(virtual input, w) + bias) and stats.sum(1) == the fp64 sums of the result without the bias, bit for bit.  Dense
    +-1 weights; where the sum of squares of a wide layer would pass 2^24 quanta the dense run still compares `out`, and the first of
    the densities 1/4, 1/16 at which the sums are exact compares `out` and `stats`."""
    name = case[0]
    dens = _stats_density(name)
    _run_forward(name, dtype, 1.0, dens == 1.0)
    if dens != 1.0:
        _run_forward(name, dtype, dens, True)


def test_exact_conv_forward_sparse_fallback_is_the_exception():
    """The sparse-weight fallback of test_exact_conv_forward must not quietly become the rule."""
    sparse = [(c[0], _stats_density(c[0])) for c in FWD_CASES]
    sparse = [(n, d) for n, d in sparse if d != 1.0]
    assert len(sparse) <= MAX_FALLBACK_CASES, sparse


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stat_slots', [0, L.STAT_SLOTS_FOLD], ids=['all_slots', 'fold_slots'])
@pytest.mark.parametrize('cu_limit', [0, 4])
@pytest.mark.parametrize('name', ['affact32_32_70x100', 'cat16_aff8_32_41x64'])
def test_exact_conv_forward_persistent_variants(name, cu_limit, stat_slots, dtype):
    """The persistent small-channel forward kernel as the training step launches it on a side lane: a compute-unit budget (another
    dealing of the tiles to the workgroups) and the sums folded into the first RD_STAT_SLOTS_FOLD copies."""
    dens = _stats_density(name)
    _run_forward(name, dtype, dens, True, cu_limit, stat_slots)


# ------------------------------------------------------------------------------------ conv gradient
@functools.lru_cache(maxsize=None)
def _grad_data(name, table):
    """Host data and the fp64 autograd reference of one gradient case (shared by dtypes, accumulate and launch forms)."""
    _, taps, dst_spec, Cout, N, H, W, gstart, slope, _ = _BY_NAME(GRAD_CASES if table == 'grad' else ROW_BLOCK_CASES)[name]
    gen = _seed(name, 1)
    G = len(gstart) - 1
    k = 3 if taps == 9 else 1
    sl = X.slope(slope)
    ys, virt, prod = [], [], []
    for kind, Cd, act in dst_spec:
        hs, ws = (2 * H, 2 * W) if kind == L.DST_POOL else ((H // 2, W // 2) if kind == L.DST_UPY else (H, W))
        z = X.stored((N, Cd, hs, ws), gen)
        sc, sh = X.scale((G, Cd), gen), X.shift((G, Cd), gen)
        zz = F.interpolate(z, scale_factor=2, mode='bilinear', align_corners=False) if kind == L.DST_UPY else z
        y = (zz * _rows(sc, gstart, N) + _rows(sh, gstart, N)).requires_grad_(True)
        a = U.act(y, sl) if act else y
        if kind == L.DST_POOL:
            a = F.max_pool2d(a, 2)
        ys.append(y)
        virt.append(a)
        prod.append((z, zz, sc, sh))
    a = torch.cat(virt, 1)
    w = X.weights((Cout, a.shape[1], k, k), gen)
    dz = X.grad((N, Cout, H, W), gen)
    (F.conv2d(a, w, None, padding=k // 2) * dz).sum().backward()
    terms = F.conv_transpose2d(dz.abs(), w.abs(), None, padding=k // 2)            # sum |dz w| per element of the input gradient
    dsts = []
    c0 = 0
    for i, (kind, Cd, act) in enumerate(dst_spec):
        z, zz, sc, sh = prod[i]
        gref = ys[i].grad
        old = X.grad(gref.shape, gen)
        t = terms[:, c0:c0 + Cd]
        c0 += Cd
        X.assert_exact_in_fp32(t.max() + 2, [gref, dz], '%s.dst%d' % (name, i))
        X.assert_exact_in_fp32(X.group_sums(gref.abs(), gstart), gref, '%s.dst%d sum g' % (name, i))
        X.assert_exact_in_fp32(X.group_sums((gref * zz).abs(), gstart), gref * zz, '%s.dst%d sum g z' % (name, i))
        dsts.append(dict(z=z, sc=sc, sh=sh, grad=gref, old=old, bstats=X.pair_sums(gref, gref * zz, gstart)))
    return dict(w=w, dz=dz, slope=sl, dsts=dsts, Cin=a.shape[1])


def _run_gradient(name, table, dtype, accumulate, halves):
    _, taps, dst_spec, Cout, N, H, W, gstart, _, _ = _BY_NAME(GRAD_CASES if table == 'grad' else ROW_BLOCK_CASES)[name]
    d = _grad_data(name, table)
    keep = U.Keep()
    G = len(gstart) - 1
    src = U.make_src(keep, d['dz'], L.SRC_RAW, dtype)
    p = _conv_desc(keep, [src], d['w'], None, N, H, W, gstart, dtype, taps, transpose=True)
    p.emode = 1
    p.c_split = dst_spec[0][1] if len(dst_spec) == 2 else d['Cin']
    outs = []
    for i, (kind, Cd, act) in enumerate(dst_spec):
        t = d['dsts'][i]
        dd = L.RdDst()
        gbuf = keep(U.nhwc(t['old'] if accumulate else torch.full(t['old'].shape, float('nan')), dtype))
        bst = keep(_stats_dev(G, Cd))
        dd.g, dd.z = gbuf.data_ptr(), keep(U.nhwc(t['z'], dtype)).data_ptr()
        dd.scale, dd.shift = keep(U.fdev(t['sc'])).data_ptr(), keep(U.fdev(t['sh'])).data_ptr()
        dd.bstats, dd.kind, dd.act, dd.accumulate, dd.Cd, dd.slope, dd.n_off, dd.g_fixed = bst.data_ptr(), kind, act, accumulate, Cd, d['slope'], 0, -1
        p.dst[i] = dd
        outs.append((gbuf, bst))
    if len(dst_spec) == 1:
        p.dst[1].kind = L.DST_NONE
    what = '%s %s acc %d%s' % (name, dtype, accumulate, ' row blocks' if halves else '')
    if halves:                                                # two launches over the 32-row blocks of the packed weights (test_gpu_ops.py)
        assert len(dst_spec) == 1 and p.CinPad == 32 and p.CoutPad == 64
        d0 = p.dst[0]
        for kb in range(2):
            q = L.RdConv()
            C.memmove(C.byref(q), C.byref(p), C.sizeof(L.RdConv))
            q.Cout = q.c_split = min(32, p.Cout - 32 * kb)
            q.CoutPad, q.w_tap_rows = 32, p.CoutPad
            q.w = p.w + 32 * kb * p.CinPad * 2
            q.dst[0].g, q.dst[0].z = d0.g + 64 * kb, d0.z + 64 * kb
            q.dst[0].scale, q.dst[0].shift, q.dst[0].bstats = d0.scale + 128 * kb, d0.shift + 128 * kb, d0.bstats + 512 * kb
            L.check(L.lib().rd_conv(C.byref(q), U.DT[dtype][0], None), what + ' rows%d' % kb)
    else:
        L.check(L.lib().rd_conv(C.byref(p), U.DT[dtype][0], None), what)
    torch.cuda.synchronize()
    for i in range(len(dst_spec)):
        t = d['dsts'][i]
        gbuf, bst = outs[i]
        X.assert_bits_equal(gbuf, _storage(t['grad'] + (t['old'] if accumulate else 0), dtype), '%s dst%d' % (what, i), nhwc=True)
        X.assert_bits_equal(bst.sum(1), t['bstats'], '%s dst%d bstats' % (what, i))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_exact_conv_gradient(case, accumulate, dtype):
    """Every destination buffer == RNE(autograd gradient + old) and bstats.sum(1) == (sum g, sum g z) of the unrounded gradient, bit for
    bit, for all three destination kinds, stored over a NaN prefill and accumulated onto an integer `old`."""
    _run_gradient(case[0], 'grad', dtype, accumulate, False)


@pytest.mark.parametrize('halves', [False, True], ids=['one_launch', 'row_blocks'])
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', ROW_BLOCK_CASES, ids=[c[0] for c in ROW_BLOCK_CASES])
def test_exact_conv_gradient_over_row_blocks(case, accumulate, halves):
    _run_gradient(case[0], 'rows', 'bf16', accumulate, halves)


def _bnbwd_pair(shape, G, gstart, gen):
    """A BatchNorm-backward source: stored g, z and coefficients; dz = P g + Q z + R is a multiple of 1/4 below 8, hence exactly
    representable in bf16 when it is staged."""
    N, Cz = shape[0], shape[1]
    g, z = X.grad(shape, gen), X.stored(shape, gen)
    P, Q, R = X.scale((G, Cz), gen), X.qcoef((G, Cz), gen), X.shift((G, Cz), gen)
    dz = g * _rows(P, gstart, N) + z * _rows(Q, gstart, N) + _rows(R, gstart, N)
    assert float(dz.abs().max()) < 8 and X.quantum(dz) >= 0.25
    return g, z, P, Q, R, dz


@functools.lru_cache(maxsize=None)
def _bnbwd_offsets_data():
    gen = _seed('bnbwd_offsets')
    N, H, W, Cz, Ca = 2, 9, 20, 32, 64
    gstart = [0, 1, 2]
    g, z, P, Q, R, dz = _bnbwd_pair((N, Cz, H, W), 2, gstart, gen)
    w = X.weights((Cz, Ca, 3, 3), gen)
    zprod = X.stored((4, Ca, H, W), gen)
    sc, sh = X.scale((2, Ca), gen), X.shift((2, Ca), gen)
    y = (zprod[2:4] * sc[1][None, :, None, None] + sh[1][None, :, None, None]).requires_grad_(True)
    (F.conv2d(F.relu(y), w, None, padding=1) * dz).sum().backward()
    old = X.grad((4, Ca, H, W), gen)
    gref = y.grad
    X.assert_exact_in_fp32(F.conv_transpose2d(dz.abs(), w.abs(), None, padding=1).max() + 2, [gref, dz], 'bnbwd')
    X.assert_exact_in_fp32(gref.abs().sum((0, 2, 3)), gref, 'bnbwd sum g')
    X.assert_exact_in_fp32((gref * zprod[2:4]).abs().sum((0, 2, 3)), gref * zprod[2:4], 'bnbwd sum g z')
    bstats = torch.stack([gref.sum((0, 2, 3)), (gref * zprod[2:4]).sum((0, 2, 3))], -1)
    return dict(g=g, z=z, P=P, Q=Q, R=R, w=w, zprod=zprod, sc=sc, sh=sh, old=old, grad=gref, bstats=bstats,
                dims=(N, H, W, Cz, Ca), gstart=gstart)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_exact_conv_bnbwd_offsets(accumulate, dtype):
    """dz = P g + Q z + R folded into the read; n_off / g_fixed as the rec decoder uses them: images 2..3 of a 4-image producer tensor,
    producer group 1.  Images 0..1 and group 0 are not touched."""
    d = _bnbwd_offsets_data()
    N, H, W, Cz, Ca = d['dims']
    keep = U.Keep()
    src = U.make_src(keep, d['g'], L.SRC_BNBWD, dtype, scale=d['P'], shift=d['R'], ptr2=d['z'], q=d['Q'])
    p = _conv_desc(keep, [src], d['w'], None, N, H, W, d['gstart'], dtype, 9, transpose=True)
    p.emode, p.c_split = 1, Ca
    prefill = d['old'] if accumulate else torch.full(d['old'].shape, float('nan'))
    gbuf = U.nhwc(prefill, dtype)
    bst = _stats_dev(2, Ca)
    dd = L.RdDst()
    dd.g, dd.z = gbuf.data_ptr(), keep(U.nhwc(d['zprod'], dtype)).data_ptr()
    dd.scale, dd.shift = keep(U.fdev(d['sc'])).data_ptr(), keep(U.fdev(d['sh'])).data_ptr()
    dd.bstats, dd.kind, dd.act, dd.accumulate, dd.Cd, dd.slope, dd.n_off, dd.g_fixed = bst.data_ptr(), L.DST_PLAIN, 1, accumulate, Ca, 0.0, 2, 1
    p.dst[0] = dd
    p.dst[1].kind = L.DST_NONE
    L.check(L.lib().rd_conv(C.byref(p), U.DT[dtype][0], None), 'bnbwd')
    torch.cuda.synchronize()
    X.assert_bits_equal(gbuf[2:4], _storage(d['grad'] + (d['old'][2:4] if accumulate else 0), dtype), 'bnbwd %s acc %d' % (dtype, accumulate), nhwc=True)
    if accumulate:
        X.assert_bits_equal(gbuf[0:2], _storage(d['old'][0:2], dtype), 'bnbwd: images 0..1 untouched', nhwc=True)
    else:
        assert bool(torch.isnan(gbuf[0:2].float()).all()), 'bnbwd: images 0..1 untouched'
    assert float(bst[0].abs().max()) == 0.0                  # only producer group 1 was touched
    X.assert_bits_equal(bst.sum(1)[1], d['bstats'], 'bnbwd bstats')


# ------------------------------------------------------------------------------------ rd_src_t.out
def _skip_if_forced_elsewhere(p):
    if os.environ.get('RAMDSIR_DEBUG_LIB') == '1' and not L.lib().rd_conv_honours_src_out(C.byref(p), L.RD_BF16):
        pytest.skip('forced dispatch routes this launch away from the kernel that stores its sources')
    assert L.lib().rd_conv_honours_src_out(C.byref(p), L.RD_BF16) == 1


@pytest.mark.parametrize('case', ['forward_cat_aff64_affact64', 'gradient_dz'])
def test_exact_conv_stores_sources(case):
    """rd_src_t.out on the geometries of the two tolerance tests: the stored act(scale x + shift) of both sources of a forward launch
    and the stored dz = P g + Q z + R of a gradient launch, every pixel once, bit for bit -- beside the launch's own exact result."""
    gen = _seed(case, 2)
    keep = U.Keep()
    dtype = 'bf16'
    if case == 'forward_cat_aff64_affact64':
        N, H, W, Cout, gstart = 8, 103, 95, 64, [0, 3, 8]
        srcs, virt, outs = [], [], []
        for mode, Cc, slope in [(L.SRC_AFF, 64, 0.0), (L.SRC_AFFACT, 64, X.slope(0.01))]:
            x = X.stored((N, Cc, H, W), gen)
            sc, sh = X.scale((2, Cc), gen), X.shift((2, Cc), gen)
            s = U.make_src(keep, x, mode, dtype, sc, sh, slope)
            outs.append(torch.full((N, H, W, Cc), float('nan'), dtype=torch.bfloat16, device=U.dev()))
            s.out = outs[-1].data_ptr()
            srcs.append(s)
            virt.append(U.virtual_input(x, mode, sc, sh, slope, gstart))
        a = torch.cat(virt, 1)
        w = X.weights((Cout, a.shape[1], 3, 3), gen)
        bias = X.bias(Cout, gen)
        p = _conv_desc(keep, srcs, w, bias, N, H, W, gstart, dtype, 9)
        out = torch.full((N, H, W, Cout), float('nan'), dtype=torch.bfloat16, device=U.dev())
        p.emode, p.out, p.stats = 0, out.data_ptr(), None
        _skip_if_forced_elsewhere(p)
        X.assert_exact_in_fp32(float(a.abs().max()) * a.shape[1] * 9 + 3, [a], case)
        L.check(L.lib().rd_conv(C.byref(p), L.RD_BF16, None), case)
        torch.cuda.synchronize()
        for i, (o, v) in enumerate(zip(outs, virt)):
            X.assert_bits_equal(o, _storage(v, dtype), '%s: stored source %d' % (case, i), nhwc=True)
        X.assert_bits_equal(out, _storage(F.conv2d(a, w, bias, padding=1), dtype), case + ' out', nhwc=True)
    else:
        N, H, W, Cz, Ca = 7, 100, 104, 64, 64
        gstart = [0, 2, 7]
        g, z, P, Q, R, dz = _bnbwd_pair((N, Cz, H, W), 2, gstart, gen)
        w = X.weights((Cz, Ca, 3, 3), gen)
        zprod = X.stored((N, Ca, H, W), gen)
        sc, sh = X.scale((2, Ca), gen), X.shift((2, Ca), gen)
        y = (zprod * _rows(sc, gstart, N) + _rows(sh, gstart, N)).requires_grad_(True)
        (F.conv2d(F.relu(y), w, None, padding=1) * dz).sum().backward()
        src = U.make_src(keep, g, L.SRC_BNBWD, dtype, scale=P, shift=R, ptr2=z, q=Q)
        dz_out = torch.full((N, H, W, Cz), float('nan'), dtype=torch.bfloat16, device=U.dev())
        src.out = dz_out.data_ptr()
        p = _conv_desc(keep, [src], w, None, N, H, W, gstart, dtype, 9, transpose=True)
        p.emode, p.c_split = 1, Ca
        gbuf = torch.full((N, H, W, Ca), float('nan'), dtype=torch.bfloat16, device=U.dev())
        dd = L.RdDst()
        dd.g, dd.z = gbuf.data_ptr(), keep(U.nhwc(zprod, dtype)).data_ptr()
        dd.scale, dd.shift = keep(U.fdev(sc)).data_ptr(), keep(U.fdev(sh)).data_ptr()
        dd.bstats, dd.kind, dd.act, dd.accumulate, dd.Cd, dd.slope, dd.n_off, dd.g_fixed = None, L.DST_PLAIN, 1, 0, Ca, 0.0, 0, -1
        p.dst[0] = dd
        p.dst[1].kind = L.DST_NONE
        _skip_if_forced_elsewhere(p)
        X.assert_exact_in_fp32(8.0 * Cz * 9, [dz, y.grad], case)
        L.check(L.lib().rd_conv(C.byref(p), L.RD_BF16, None), case)
        torch.cuda.synchronize()
        X.assert_bits_equal(dz_out, _storage(dz, dtype), case + ': stored dz', nhwc=True)
        X.assert_bits_equal(gbuf, _storage(y.grad, dtype), case + ' dgrad', nhwc=True)


# ------------------------------------------------------------------------------------ wgrad
@functools.lru_cache(maxsize=None)
def _wgrad_data(name):
    case = _BY_NAME(WG_CASES)[name]
    _, taps, src_spec, Cout, N, H, W, bnbwd = case[:8]
    gen = _seed(name, 3)
    gstart = case[8] if len(case) > 8 else [0, 1, N]
    G = len(gstart) - 1
    k = 3 if taps == 9 else 1
    xs, virt = [], []
    for mode, Cc in src_spec:
        hs, ws = _src_dims(mode, H, W)
        x = X.stored((N, Cc, hs, ws), gen)
        sc, sh = X.scale((G, Cc), gen), X.shift((G, Cc), gen)
        xs.append((x, sc, sh))
        virt.append(U.virtual_input(x, mode, sc, sh, 0.0, gstart))
    a = torch.cat(virt, 1)
    if bnbwd:
        dzsrc = _bnbwd_pair((N, Cout, H, W), G, gstart, gen)
        dz = dzsrc[5]
    else:
        dz = X.grad((N, Cout, H, W), gen)
        dzsrc = (dz,)
    w = torch.zeros(Cout, a.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    (F.conv2d(a, w, None, padding=k // 2) * dz).sum().backward()
    w0 = torch.zeros(Cout, a.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    (F.conv2d(a.abs(), w0, None, padding=k // 2) * dz.abs()).sum().backward()        # sum |a dz| per weight element
    old = X.ints(-3, 3, w.shape, gen)
    X.assert_exact_in_fp32(w0.grad + 3, [a, dz, X.quantum(a) * X.quantum(dz)], name + ' dW')
    return dict(xs=xs, dzsrc=dzsrc, bnbwd=bnbwd, gstart=gstart, Cin=a.shape[1], old=old, dW=(old + w.grad.detach()).float())


def _run_wgrad(name, dtype, cu_limit=0):
    """-> (dW on the device, workspace bytes of the launch)"""
    case = _BY_NAME(WG_CASES)[name]
    _, taps, src_spec, Cout, N, H, W, _ = case[:8]
    d = _wgrad_data(name)
    keep = U.Keep()
    gstart = d['gstart']
    p = L.RdWgrad()
    for i, ((mode, Cc), (x, sc, sh)) in enumerate(zip(src_spec, d['xs'])):
        p.a[i] = U.make_src(keep, x, mode, dtype, sc, sh, 0.0)
    if d['bnbwd']:
        g, z, P, Q, R, _ = d['dzsrc']
        p.dz = U.make_src(keep, g, L.SRC_BNBWD, dtype, scale=P, shift=R, ptr2=z, q=Q)
    else:
        p.dz = U.make_src(keep, d['dzsrc'][0], L.SRC_RAW, dtype)
    p.na, p.taps, p.N, p.H, p.W, p.Cin, p.Cout, p.G = len(src_spec), taps, N, H, W, d['Cin'], Cout, len(gstart) - 1
    p.gstart = L.gstart_array(gstart)
    p.cu_limit = cu_limit
    ws_bytes = L.lib().rd_wgrad_workspace(C.byref(p), U.DT[dtype][0])
    part = torch.full((ws_bytes // 4,), float('nan'), device=U.dev())
    dW = d['old'].float().to(U.dev())
    p.partial, p.dW, p.beta = part.data_ptr(), dW.data_ptr(), 1.0
    L.check(L.lib().rd_wgrad(C.byref(p), U.DT[dtype][0], None), name)
    torch.cuda.synchronize()
    X.assert_bits_equal(dW, d['dW'], '%s %s cu_limit %d dW' % (name, dtype, cu_limit))
    return ws_bytes


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', WG_CASES, ids=[c[0] for c in WG_CASES])
def test_exact_wgrad(case, dtype):
    """dW (fp32) == old + sum a dz exactly, beta = 1 on an integer `old`: one dropped, doubled or misplaced pixel of any tile of any
    pixel split changes it."""
    _run_wgrad(case[0], dtype)


# cu_limit -> pixel splits (csrc/wgrad.hip rd_wgrad_route_plan): splits = ceil(cu_limit / blocks of the layer), at most the 8 x 32-tile count.
# The fp32 kernel deals 8 x 32 tiles; the bf16 kernels these cases take (wgrad_ws_kernel, wgrad_sym_kernel) deal 4 x 32 tiles.
WG_CU_LIMITS = {
    # case: {dtype: (tiles the kernel deals, cu_limit that gives a split count which does not divide them)}
    'c64_64_many_tiles': {'bf16': (120, 7), 'f32': (60, 25)},                    # 7 splits
    'sym_raw128_128_rawdz_many_tiles': {'bf16': (120, 14), 'f32': (60, 112)},    # 7 splits
    'c128_128': {'bf16': (6, 8), 'f32': (4, 48)},                                # 4 splits of 6 tiles / 3 splits of 4 tiles
}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(WG_CU_LIMITS))
def test_exact_wgrad_cu_limit(name, dtype):
    """The compute-unit budget every side-lane launch of the training step carries: it changes how the tiles are dealt to the persistent
    workgroups.  One pixel split, and a split count that does not divide the tile count; rd_wgrad_workspace() -- one partial per
    workgroup -- proves that the dealing really changed."""
    case = _BY_NAME(WG_CASES)[name]
    tiles, cu_ragged = WG_CU_LIMITS[name][dtype]
    assert tiles == case[4] * ((case[5] + (3 if dtype == 'bf16' else 7)) // (4 if dtype == 'bf16' else 8)) * ((case[6] + 31) // 32)
    ws_all = _run_wgrad(name, dtype, 0)
    ws_one = _run_wgrad(name, dtype, 1)
    ws_rag = _run_wgrad(name, dtype, cu_ragged)
    assert ws_one < ws_all and ws_all % ws_one == 0 and ws_rag % ws_one == 0        # ws_one is one split's partial: the whole device splits
    splits_rag = ws_rag // ws_one
    assert splits_rag > 1 and tiles % splits_rag != 0, (ws_all // ws_one, splits_rag, tiles)


# ------------------------------------------------------------------------------------ fused backward
@functools.lru_cache(maxsize=None)
def _fused_data(name):
    _, in_spec, Cout, dzs, N, H, W, gstart, bnbwd, _, _ = _BY_NAME(FUSED_CASES)[name]
    sl = X.slope(0.01) if 'leaky' in name else 0.0
    gen = _seed(name, 4)
    G = len(gstart) - 1
    ys, virt, prod = [], [], []
    for mode, Cd, has_norm in in_spec:
        z = X.stored((N, Cd, H, W), gen)
        sc, sh = X.scale((G, Cd), gen), X.shift((G, Cd), gen)
        y = ((z * _rows(sc, gstart, N) + _rows(sh, gstart, N)) if has_norm else z.clone()).requires_grad_(True)
        a = U.act(y, sl) if mode == L.SRC_AFFACT else y
        ys.append(y)
        virt.append(a)
        prod.append((z, sc, sh))
    a = torch.cat(virt, 1)
    w = X.weights((Cout, a.shape[1], 3, 3), gen).requires_grad_(True)
    if bnbwd:
        dzsrc = _bnbwd_pair((N, Cout, H, W), G, gstart, gen)
        dz = dzsrc[5]
    else:
        dz = X.grad((N, Cout, H, W), gen)
        dzsrc = (dz,)
    (F.conv2d(a, w, None, padding=1) * dz).sum().backward()
    w0 = torch.zeros(w.shape, dtype=torch.float64, requires_grad=True)
    (F.conv2d(a.detach().abs(), w0, None, padding=1) * dz.abs()).sum().backward()
    X.assert_exact_in_fp32(w0.grad, [a.detach(), dz, X.quantum(a.detach()) * X.quantum(dz)], name + ' dW')
    terms = F.conv_transpose2d(dz.abs(), w.detach().abs(), None, padding=1)
    dsts, c0 = [], 0
    for i, (mode, Cd, has_norm) in enumerate(in_spec):
        z, sc, sh = prod[i]
        gref = ys[i].grad
        old = X.grad(gref.shape, gen)
        X.assert_exact_in_fp32(terms[:, c0:c0 + Cd].max() + 2, [gref, dz], '%s.dst%d' % (name, i))
        c0 += Cd
        X.assert_exact_in_fp32(X.group_sums(gref.abs(), gstart), gref, name + ' sum g')
        X.assert_exact_in_fp32(X.group_sums((gref * z).abs(), gstart), gref * z, name + ' sum g z')
        dsts.append(dict(z=z, sc=sc, sh=sh, grad=gref, old=old, bstats=X.pair_sums(gref, gref * z, gstart)))
    return dict(w=w.detach(), dW=w.grad.float(), dzsrc=dzsrc, dz=dz, slope=sl, dsts=dsts, Cin=a.shape[1])


@pytest.mark.parametrize('case', FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_exact_fused_backward(case):
    """rd_conv_bwd_fused + rd_conv_bwd_fused_reduce: input gradient, bstats and dW all equal to the fp64 autograd reference bit for bit
    -- hence also to what the separate rd_conv + rd_wgrad launches give (test_exact_conv_gradient, test_exact_wgrad)."""
    name, in_spec, Cout, dzs, N, H, W, gstart, bnbwd, accumulate, cu_limit = case
    d = _fused_data(name)
    keep = U.Keep()
    DT = 'bf16'
    dt = U.DT[DT][0]
    G = len(gstart) - 1
    if bnbwd:
        g, z, P, Q, R, _ = d['dzsrc']
        src = U.make_src(keep, g, L.SRC_BNBWD, DT, scale=P, shift=R, ptr2=z, q=Q)
    elif dzs:                                                  # narrow gradient stored with a zero-padded channel tail (dlogits)
        padded = torch.zeros(N, dzs, H, W, dtype=torch.float64)
        padded[:, :Cout] = d['dz']
        src = U.make_src(keep, padded, L.SRC_RAW, DT)
    else:
        src = U.make_src(keep, d['dz'], L.SRC_RAW, DT)
    p = _conv_desc(keep, [src], d['w'], None, N, H, W, gstart, DT, 9, transpose=True)
    p.emode = 1
    p.c_split = in_spec[0][1] if len(in_spec) == 2 else d['Cin']
    p.cu_limit = cu_limit
    wg = L.RdWgrad()
    outs = []
    for i, (mode, Cd, has_norm) in enumerate(in_spec):
        t = d['dsts'][i]
        zd = keep(U.nhwc(t['z'], DT))
        scd, shd = keep(U.fdev(t['sc'])), keep(U.fdev(t['sh']))
        gbuf = keep(U.nhwc(t['old'] if accumulate else torch.full(t['old'].shape, float('nan')), DT))
        bst = keep(_stats_dev(G, Cd))
        dd = L.RdDst()
        dd.g = gbuf.data_ptr()
        if has_norm:
            dd.z, dd.scale, dd.shift, dd.bstats = zd.data_ptr(), scd.data_ptr(), shd.data_ptr(), bst.data_ptr()
        dd.kind, dd.act, dd.accumulate, dd.Cd, dd.slope, dd.n_off, dd.g_fixed = L.DST_PLAIN, int(mode == L.SRC_AFFACT), accumulate, Cd, d['slope'], 0, -1
        p.dst[i] = dd
        s = L.RdSrc()
        s.ptr = zd.data_ptr()
        if has_norm:
            s.scale, s.shift = scd.data_ptr(), shd.data_ptr()
        s.mode, s.C, s.slope, s.n_off, s.g_fixed = mode, Cd, d['slope'], 0, -1
        wg.a[i] = s
        outs.append((gbuf, bst))
    if len(in_spec) == 1:
        p.dst[1].kind = L.DST_NONE
    wg.na, wg.taps, wg.dz = len(in_spec), 9, src
    wg.N, wg.H, wg.W, wg.Cin, wg.Cout, wg.G = N, H, W, d['Cin'], Cout, G
    wg.gstart = L.gstart_array(gstart)
    dW = keep(torch.full((Cout, d['Cin'], 3, 3), float('nan'), device=U.dev()))
    wg.dW, wg.beta = dW.data_ptr(), 0.0
    lib = L.lib()
    assert lib.rd_conv_bwd_fused_ok(C.byref(p), C.byref(wg), dt) == 1, name
    part = keep(torch.full((lib.rd_conv_bwd_fused_workspace(C.byref(p), C.byref(wg), dt) // 4,), float('nan'), device=U.dev()))
    wg.partial = part.data_ptr()
    L.check(lib.rd_conv_bwd_fused(C.byref(p), C.byref(wg), dt, None), name)
    L.check(lib.rd_conv_bwd_fused_reduce(C.byref(p), C.byref(wg), dt, None), name + ' reduce')
    torch.cuda.synchronize()
    for i, (mode, Cd, has_norm) in enumerate(in_spec):
        t = d['dsts'][i]
        gbuf, bst = outs[i]
        X.assert_bits_equal(gbuf, _storage(t['grad'] + (t['old'] if accumulate else 0), DT), '%s dst%d' % (name, i), nhwc=True)
        if has_norm:
            X.assert_bits_equal(bst.sum(1), t['bstats'], '%s dst%d bstats' % (name, i))
    X.assert_bits_equal(dW, d['dW'], name + ' dW')


# ------------------------------------------------------------------------------------ elementwise kernels (csrc/bn.hip)
# smallest shapes with several workgroups and a ragged last one; three images in groups of 1 and 2
EN, EGS = 3, [0, 1, 3]


def _gs():
    return L.gstart_array(EGS)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stat_slots', [0, L.STAT_SLOTS_FOLD])
@pytest.mark.parametrize('store_y', [False, True], ids=['y_null', 'y_stored'])
def test_exact_up_stats(store_y, stat_slots, dtype):
    """rd_up_stats at 13 x 17 x 32 (2 workgroups in bf16, 4 in fp32): y = bilinear_x2(t) is a multiple of 1/16, its sums and the stored
    y are exact."""
    gen = _seed('up_stats')
    h, w, Cc = 13, 17, 32
    t = X.stored((EN, Cc, h, w), gen)
    y = F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)
    X.assert_exact_in_fp32(X.group_sums(y.abs(), EGS), y, 'sum y')
    X.assert_exact_in_fp32(X.group_sums(y * y, EGS) * 4, y * y, 'sum y^2')       # x 4: the kernel sums deviations from a pivot, |d| <= 2 max|y|
    td = U.nhwc(t, dtype)
    stats = _stats_dev(2, Cc)
    yd = torch.full((EN, 2 * h, 2 * w, Cc), float('nan'), dtype=U.DT[dtype][1], device=U.dev()) if store_y else None
    L.check(L.lib().rd_up_stats(L.ptr(td), L.ptr(stats), L.ptr(yd), EN, h, w, Cc, 2, _gs(), U.DT[dtype][0], stat_slots, None), 'up_stats')
    torch.cuda.synchronize()
    if stat_slots:
        assert float(stats[:, stat_slots:].abs().max()) == 0.0
    X.assert_bits_equal(stats.sum(1), X.pair_sums(y, y * y, EGS), 'up_stats %s' % dtype)
    if store_y:
        X.assert_bits_equal(yd, _storage(y, dtype), 'up_stats y', nhwc=True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_up_bwd(dtype):
    """rd_up_bwd at 13 x 11 x 32: dt = up2^T(P g + Q up2(t) + R), a multiple of 2^-10 of magnitude < 32: exact in fp32, one rounding
    into the storage type."""
    gen = _seed('up_bwd')
    h, w, Cc = 13, 11, 32
    t = X.stored((EN, Cc, h, w), gen).requires_grad_(True)
    y = F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)
    g2 = X.grad((EN, Cc, 2 * h, 2 * w), gen)
    P, Q, R = X.scale((2, Cc), gen), X.qcoef((2, Cc), gen), X.shift((2, Cc), gen)
    dzh = g2 * _rows(P, EGS, EN) + y.detach() * _rows(Q, EGS, EN) + _rows(R, EGS, EN)
    (y * dzh).sum().backward()
    X.assert_exact_in_fp32(4 * float(dzh.abs().max()), [t.grad, dzh, 2.0 ** -10], 'dt')
    dt = torch.full((EN, h, w, Cc), float('nan'), dtype=U.DT[dtype][1], device=U.dev())
    g2d, td = U.nhwc(g2, dtype), U.nhwc(t.detach(), dtype)               # named: the device tensors must outlive the launch
    Pd, Qd, Rd = U.fdev(P), U.fdev(Q), U.fdev(R)
    L.check(L.lib().rd_up_bwd(L.ptr(g2d), L.ptr(td), L.ptr(dt), L.ptr(Pd), L.ptr(Qd), L.ptr(Rd), EN, h, w, Cc, 2, _gs(), U.DT[dtype][0],
                              None, 0, None), 'up_bwd')
    torch.cuda.synchronize()
    X.assert_bits_equal(dt, _storage(t.grad, dtype), 'up_bwd %s' % dtype, nhwc=True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('with_bn', [True, False], ids=['coefficients', 'plain'])
def test_exact_pool(with_bn, dtype):
    """rd_pool_fwd / rd_pool_bwd at 13 x 11 x 64 on {-1, 0, 1}: nearly every window has a tie, the scatter goes to the FIRST maximum and
    takes the activation derivative there (0 at 0); accumulate 0 and 1; bstats exact."""
    gen = _seed('pool')
    Ho, Wo, Cc = 13, 11, 64
    z = X.stored((EN, Cc, 2 * Ho, 2 * Wo), gen)
    sc, sh = X.scale((2, Cc), gen), X.shift((2, Cc), gen)
    zd = U.nhwc(z, dtype)
    scd, shd = (U.fdev(sc), U.fdev(sh)) if with_bn else (None, None)
    out = torch.full((EN, Ho, Wo, Cc), float('nan'), dtype=U.DT[dtype][1], device=U.dev())
    L.check(L.lib().rd_pool_fwd(L.ptr(zd), L.ptr(scd), L.ptr(shd), 0.0 if with_bn else 1.0, L.ptr(out), EN, Ho, Wo, Cc, 2, _gs(),
                                U.DT[dtype][0], None, 0, None), 'pool_fwd')
    torch.cuda.synchronize()
    zz = z.clone().requires_grad_(True)
    pre = (zz * _rows(sc, EGS, EN) + _rows(sh, EGS, EN)) if with_bn else zz
    ref = F.max_pool2d(F.relu(pre) if with_bn else pre, 2)
    X.assert_bits_equal(out, _storage(ref.detach(), dtype), 'pool_fwd', nhwc=True)
    gp = X.grad((EN, Cc, Ho, Wo), gen)
    gpd = U.nhwc(gp, dtype)
    old = X.grad((EN, Cc, 2 * Ho, 2 * Wo), gen)
    pre.retain_grad()
    ref.backward(gp)
    gref = pre.grad
    X.assert_exact_in_fp32(X.group_sums(gref.abs(), EGS), gref, 'sum g')
    for accumulate in (0, 1):
        gbuf = U.nhwc(old if accumulate else torch.full(old.shape, float('nan')), dtype)
        bst = _stats_dev(2, Cc)
        L.check(L.lib().rd_pool_bwd(L.ptr(gpd), L.ptr(zd), L.ptr(scd), L.ptr(shd), 0.0 if with_bn else 1.0, 1 if with_bn else 0,
                                    L.ptr(gbuf), accumulate, L.ptr(bst) if with_bn else None, EN, Ho, Wo, Cc, 2, _gs(), U.DT[dtype][0],
                                    accumulate * L.STAT_SLOTS_FOLD, None), 'pool_bwd')
        torch.cuda.synchronize()
        X.assert_bits_equal(gbuf, _storage(gref + (old if accumulate else 0), dtype), 'pool_bwd acc %d' % accumulate, nhwc=True)
        if with_bn:
            X.assert_bits_equal(bst.sum(1), X.pair_sums(gref, gref * z, EGS), 'pool_bwd bstats acc %d' % accumulate)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_bn_apply(dtype):
    """rd_bn_apply at 13 x 11 x 64: act(a x + c) with ReLU and a dyadic leaky slope, and the two-operand form a x + b x2 + c."""
    gen = _seed('bn_apply')
    H, W, Cc = 13, 11, 64
    x, z = X.grad((EN, Cc, H, W), gen), X.stored((EN, Cc, H, W), gen)
    a, b, c = X.scale((2, Cc), gen), X.qcoef((2, Cc), gen), X.shift((2, Cc), gen)
    xd, zd = U.nhwc(x, dtype), U.nhwc(z, dtype)
    ad, bd, cd = U.fdev(a), U.fdev(b), U.fdev(c)
    out = torch.full((EN, H, W, Cc), float('nan'), dtype=U.DT[dtype][1], device=U.dev())
    for slope in (0.0, 0.25):
        L.check(L.lib().rd_bn_apply(L.ptr(xd), None, L.ptr(out), L.ptr(ad), None, L.ptr(cd), slope, EN, H, W, Cc, 2, _gs(),
                                    U.DT[dtype][0], None), 'apply fwd')
        torch.cuda.synchronize()
        X.assert_bits_equal(out, _storage(U.act(x * _rows(a, EGS, EN) + _rows(c, EGS, EN), slope), dtype), 'bn_apply slope %g' % slope, nhwc=True)
    L.check(L.lib().rd_bn_apply(L.ptr(xd), L.ptr(zd), L.ptr(out), L.ptr(ad), L.ptr(bd), L.ptr(cd), 1.0, EN, H, W, Cc, 2, _gs(),
                                U.DT[dtype][0], None), 'apply bwd')
    torch.cuda.synchronize()
    ref = x * _rows(a, EGS, EN) + z * _rows(b, EGS, EN) + _rows(c, EGS, EN)
    X.assert_bits_equal(out, _storage(ref, dtype), 'bn_apply two operands', nhwc=True)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cc', [3, 24, 256])
def test_exact_bn_stats(Cc, dtype):
    """rd_bn_stats at 40 x 56; 256 % C != 0 for C = 3 and 24 leaves threads of every workgroup idle."""
    gen = _seed('bn_stats', Cc)
    H, W = 40, 56
    x = X.stored((EN, Cc, H, W), gen)
    X.assert_exact_in_fp32(X.group_sums(x.abs(), EGS), x, 'sum x')
    X.assert_exact_in_fp32(X.group_sums(x * x, EGS) * 4, x * x, 'sum x^2')      # x 4: deviations from a pivot, |d| <= 2 max|x|
    stats = _stats_dev(2, Cc)
    xd = U.nhwc(x, dtype)
    L.check(L.lib().rd_bn_stats(L.ptr(xd), L.ptr(stats), EN, H, W, Cc, 2, _gs(), U.DT[dtype][0], None), 'bn_stats')
    torch.cuda.synchronize()
    X.assert_bits_equal(stats.sum(1), X.pair_sums(x, x * x, EGS), 'bn_stats C %d %s' % (Cc, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cc', [3, 16])
def test_exact_grad_in_and_to_nchw(Cc, dtype):
    """rd_nhwc_to_nchw with coefficients and activation, and rd_grad_in (mask by the activation derivative, 0 at 0; accumulate 0 and 1;
    bstats) at 9 x 11."""
    gen = _seed('grad_in', Cc)
    H, W = 9, 11
    z = X.stored((EN, Cc, H, W), gen)
    sc, sh = X.scale((2, Cc), gen), X.shift((2, Cc), gen)
    zd, scd, shd = U.nhwc(z, dtype), U.fdev(sc), U.fdev(sh)
    pre = z * _rows(sc, EGS, EN) + _rows(sh, EGS, EN)
    dy = X.grad((EN, Cc, H, W), gen)
    old = X.grad((EN, Cc, H, W), gen)
    dyd = dy.float().to(U.dev())
    for slope in (0.0, 0.25):
        back = torch.full((EN, Cc, H, W), float('nan'), device=U.dev())
        L.check(L.lib().rd_nhwc_to_nchw(L.ptr(zd), L.ptr(back), L.ptr(scd), L.ptr(shd), 1, slope, EN, Cc, H, W, 2, _gs(), U.DT[dtype][0], None), 'to_nchw')
        torch.cuda.synchronize()
        X.assert_bits_equal(back, U.act(pre, slope).float(), 'nhwc_to_nchw slope %g' % slope)
        gnew = dy * torch.where(pre > 0, 1.0, slope)
        X.assert_exact_in_fp32(X.group_sums(gnew.abs(), EGS), gnew, 'sum g')
        X.assert_exact_in_fp32(X.group_sums((gnew * z).abs(), EGS), gnew * z, 'sum g z')
        for accumulate in (0, 1):
            gbuf = U.nhwc(old if accumulate else torch.full(old.shape, float('nan')), dtype)
            bst = _stats_dev(2, Cc)
            L.check(L.lib().rd_grad_in(L.ptr(dyd), L.ptr(zd), L.ptr(gbuf), L.ptr(scd), L.ptr(shd), L.ptr(bst), 1, slope, accumulate, EN, Cc, H, W,
                                       2, _gs(), U.DT[dtype][0], None), 'grad_in')
            torch.cuda.synchronize()
            X.assert_bits_equal(gbuf, _storage(gnew + (old if accumulate else 0), dtype), 'grad_in slope %g acc %d' % (slope, accumulate), nhwc=True)
            X.assert_bits_equal(bst.sum(1), X.pair_sums(gnew, gnew * z, EGS), 'grad_in bstats slope %g acc %d' % (slope, accumulate))
    back = torch.full((EN, Cc, H, W), float('nan'), device=U.dev())
    L.check(L.lib().rd_nhwc_to_nchw(L.ptr(zd), L.ptr(back), None, None, 0, 0.0, EN, Cc, H, W, 2, _gs(), U.DT[dtype][0], None), 'to_nchw plain')
    torch.cuda.synchronize()
    X.assert_bits_equal(back, z.float(), 'nhwc_to_nchw plain')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cc', [2, 3, 8])
def test_exact_colsum(Cc, dtype):
    """rd_colsum over 1200 pixels stored with a channel stride of 8: the pad (ones) must not enter, beta 1 and 0."""
    gen = _seed('colsum', Cc)
    npix, cs = 1200, 8
    t = X.grad((npix, Cc), gen)
    td = torch.ones(npix, cs, dtype=U.DT[dtype][1], device=U.dev())
    td[:, :Cc] = t.to(U.DT[dtype][1]).to(U.dev())
    old = X.ints(-3, 3, (Cc,), gen)
    X.assert_exact_in_fp32(t.abs().sum(0) + old.abs(), [t, old], 'column sums')
    wsb = torch.full((8192,), float('nan'), device=U.dev())
    for beta in (1.0, 0.0):
        outc = old.float().to(U.dev())
        L.check(L.lib().rd_colsum(L.ptr(td), L.ptr(outc), L.ptr(wsb), npix, Cc, cs, beta, U.DT[dtype][0], None), 'colsum')
        torch.cuda.synchronize()
        X.assert_bits_equal(outc, (beta * old + t.sum(0)).float(), 'colsum C %d beta %g' % (Cc, beta))
