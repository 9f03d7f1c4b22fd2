"""CPU tests of the fused validation forward (ramdsir/infer.py, train.py --fused_val): the frozen-BatchNorm plan holds only conv and
pool launches, every conv takes the route it takes in the eval plans of the drop-in modules (the reason to expect the same bits), the
site record has one layout in C and ctypes, the numpy model of the coefficient kernel agrees with nn.BatchNorm2d.eval(), and the flag
refuses what it cannot do.  Plans are built as tests/plan_dump.py builds them: on CPU tensors, nothing is launched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plan_dump as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))

from ramdsir import _lib as L           # noqa: E402
from ramdsir import engine as E         # noqa: E402
from ramdsir import infer as I          # noqa: E402

MODS = [('enc', E.encoder_specs(3, 16)), ('dec', E.decoder_specs(16, 2))]
GEOMETRIES = [(1, 32, 32), (8, 256, 256)]
DTYPES = [torch.bfloat16, torch.float32]


def _frozen(dtype, N, H, W):
    bank = E.ParamBank(MODS, 'cpu')
    wpack = E.WeightPack(bank, MODS, dtype)
    return I.build_plan(bank, wpack, dtype, N, H, W), bank, wpack


def _module_eval_plans(dtype, N, H, W):
    """The eval plans Encoder.forward and Decoder.forward build for this geometry (networks/unet.py: the Plan defaults, training=False)."""
    def plan(mods, graph):
        bank = E.ParamBank(mods, 'cpu')
        pl = E.Plan(bank, dtype, N, [0, N], slope=0.0, training=False)
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


def _convs(pl):
    return [op for op in pl.fwd if op[0].__name__ == 'rd_conv']


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMETRIES)
def test_frozen_plan_holds_only_conv_and_pool_launches(dtype, geom):
    pl, bank, wpack = _frozen(dtype, *geom)
    names = [op[0].__name__ for op in pl.fwd]
    assert set(names) == {'rd_conv', 'rd_pool_fwd'}
    n_conv = sum(1 for m, specs in MODS for key, shape, kind, _ in specs if kind == 'param' and len(shape) == 4)
    assert names.count('rd_conv') == n_conv == 27
    enc, _ = _module_eval_plans(dtype, *geom)
    assert names.count('rd_pool_fwd') == [op[0].__name__ for op in enc.fwd].count('rd_pool_fwd') == 4
    assert pl.bwd == []
    for op in _convs(pl):
        assert not op[1][0]._obj.stats                      # no statistics anywhere
    # one site per BatchNorm of the two modules, C from 16 to 256
    n_bn = sum(1 for m, specs in MODS for key, *_ in specs if key.endswith('running_mean'))
    assert len(pl.bn_sites) == n_bn == 26 and {s[6] for s in pl.bn_sites} == {16, 32, 64, 128, 256}
    # the input has the module plan's channel stride (it picks the first conv's kernel), the logits the stride the plan gives them
    N, H, W = geom
    assert tuple(pl.x_in.buf.shape) == (N, H, W, 3) and pl.x_in.buf.dtype == dtype
    assert tuple(pl.out.buf.shape) == (N, H, W, 2)
    # every pointer of every launch lies in a buffer the plan, the bank or the pack owns (plan_dump raises otherwise)
    reg = PD.Registry()
    reg.bank(bank, wpack)
    reg.plan('pl', pl, [])
    d = PD.dump_plan('pl', pl, reg)
    assert len(d['fwd']) == 31
    table = I.site_table(pl.bn_sites)
    for i in range(len(pl.bn_sites)):
        for f in ('gamma', 'beta', 'running_mean', 'running_var', 'scale', 'shift'):
            assert reg.sym(getattr(table[i], f), 'site %d.%s' % (i, f)) is not None


def test_frozen_plan_refuses_what_it_cannot_freeze():
    bank = E.ParamBank(MODS, 'cpu')
    with pytest.raises(ValueError):
        E.Plan(bank, torch.float32, 2, [0, 2], training=True, frozen_bn=True)
    with pytest.raises(ValueError):
        E.Plan(bank, torch.float32, 2, [0, 1, 2], training=False, frozen_bn=True)
    with pytest.raises(ValueError):
        I.build_plan(bank, E.WeightPack(bank, MODS, torch.float32), torch.float32, 1, 40, 32)          # not a multiple of 16
    gn = [('enc', E.encoder_specs(3, 16, 'gn'))]
    bank = E.ParamBank(gn, 'cpu')
    pl = E.Plan(bank, torch.float32, 1, [0, 1], training=False, frozen_bn=True)
    E.build_encoder(pl, E.Act(pl, 1, 32, 32, 3), n=16, mname='enc', norm='gn')
    with pytest.raises(ValueError):
        pl.build(E.WeightPack(bank, gn, torch.float32))


def _route(p, dt):
    r = L.RdRoute()
    rc = L.lib().rd_conv_route(C.byref(p), dt, C.byref(r))
    return rc, r.kernel.decode().split('<')[0] if rc == 0 else None, list(r.grid), r.block, r.lds, list(r.iarg)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMETRIES + [(3, 48, 80)])
def test_every_conv_takes_the_route_of_the_module_eval_plans(dtype, geom):
    """Kernel (up to its template arguments), grid, block, LDS and integer arguments of each of the 27 conv launches equal those of
    the same layer in the Encoder / Decoder module plans in eval mode: the frozen plan differs from them in its sources' modes
    (RD_SRC_AFFACT where the decoder module reads a materialised RD_SRC_RAW tensor), its null statistics pointer and the padded
    channel stride of the image -- none of which may move a launch to another kernel or tiling."""
    pl, _, _ = _frozen(dtype, *geom)
    enc, dec = _module_eval_plans(dtype, *geom)
    dt = pl.dt
    ours, theirs = _convs(pl), _convs(enc) + _convs(dec)
    assert len(ours) == len(theirs) == 27
    for a, b in zip(ours, theirs):
        assert a[2]['layer'] == b[2]['layer']
        ra, rb = _route(a[1][0]._obj, dt), _route(b[1][0]._obj, dt)
        assert ra[0] == 0 and ra == rb, (a[2]['layer'], ra, rb)


def test_site_record_has_one_layout_in_c_and_ctypes(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(rd_bn_eval_site_t), '
           'offsetof(rd_bn_eval_site_t, scale), offsetof(rd_bn_eval_site_t, C), offsetof(rd_bn_eval_site_t, pad_));return 0;}')
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, off_scale, off_c, off_pad = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert (size, off_scale, off_c, off_pad) == (C.sizeof(L.RdBnEvalSite), L.RdBnEvalSite.scale.offset, L.RdBnEvalSite.C.offset,
                                                 L.RdBnEvalSite.pad_.offset) == (56, 32, 48, 52)


def test_coefficient_model_agrees_with_batchnorm_eval():
    """y = x * scale + shift with the model's float32 coefficients against nn.BatchNorm2d.eval() on the CPU.

    Tolerance, from float32 rounding (u = 2^-24) of the two formulations against the exact value
    y = (x - rm) * g / sqrt(rv + eps) + b, with s = g / sqrt(rv + eps) exact:
      the model rounds rv + eps, the square root, the division and the product with g: scale = s (1 + d), |d| <= 4u (first order);
      shift = b - rm * scale rounds the product and the difference: |shift - (b - rm s)| <= |rm s| 5u + |b - rm s| u;
      y' = x * scale + shift rounds the product and the sum: |y' - y| <= |x s| 5u + |rm s| 5u + |b - rm s| u + |y| u
           <= 6u (|x s| + |rm s| + |b|)  =: bound   (|b - rm s| <= |b| + |rm s|, |y| <= |x s| + |rm s| + |b|).
    torch evaluates the same quantity in float32 with its own order of at most as many roundings of terms no larger than these, so it
    lies within the same bound of the exact value, and the two float32 results within 2 * bound of each other."""
    rng = np.random.RandomState(5)
    Cc = 37
    g = rng.normal(0, 1.5, Cc).astype(np.float32)
    g[:4] = [-2.0, -0.25, 0.0, 3.0]
    b = rng.normal(0, 1, Cc).astype(np.float32)
    rm = rng.normal(0.5, 2, Cc).astype(np.float32)
    rv = rng.uniform(0.5, 2, Cc).astype(np.float32)
    rv[:4] = [0.0, 1e-12, 1e4, 1.0]
    x = rng.normal(0, 3, (2, Cc, 5, 7)).astype(np.float32)
    scale, shift = I.eval_coeffs_model(g, b, rm, rv)
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    bn = torch.nn.BatchNorm2d(Cc).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(g))
        bn.bias.copy_(torch.from_numpy(b))
        bn.running_mean.copy_(torch.from_numpy(rm))
        bn.running_var.copy_(torch.from_numpy(rv))
        ref = bn(torch.from_numpy(x)).numpy()
    got = x * scale[None, :, None, None] + shift[None, :, None, None]
    s = g.astype(np.float64) / np.sqrt(rv.astype(np.float64) + float(np.float32(bn.eps)))
    exact = (x.astype(np.float64) - rm[None, :, None, None]) * s[None, :, None, None] + b[None, :, None, None]
    bound = 6 * 2.0 ** -24 * (np.abs(x * s[None, :, None, None]) + np.abs(rm * s)[None, :, None, None] + np.abs(b)[None, :, None, None])
    assert bn.eps == E.EPS
    assert (np.abs(got - exact) <= bound).all(), float((np.abs(got - exact) / bound).max())
    assert (np.abs(got - ref) <= 2 * bound).all(), float((np.abs(got - ref) / bound).max())


def _main_args(extra):
    import train
    return train, train.parse_args(['--save_path', 'unused', '--ram', '--rec'] + extra)


def test_fused_val_flag_needs_a_resident_validation_and_batchnorm():
    train, args = _main_args(['--fused_val'])
    with pytest.raises(ValueError, match='--gpu_val'):
        train.main(args)
    train, args = _main_args(['--fused_val', '--gpu_val', '--norm', 'gn'])
    with pytest.raises(ValueError, match='--norm gn'):
        train.main(args)
    # without the flag the namespace is the one the rest of the code reads today, plus the flag switched off
    train, args = _main_args([])
    assert args.fused_val is False and not args.gpu_val and not args.gpu_val_volumes and args.norm == 'bn' and args.tb_images == 0
    train, args = _main_args(['--fused_val', '--gpu_val_volumes'])
    assert args.fused_val is True
