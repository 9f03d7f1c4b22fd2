"""-m gpu: the fused validation forward (ramdsir/infer.py EvalForward, csrc/infer.hip, train.py --fused_val) against the path it
replaces, bit for bit everywhere: the coefficient kernel against rd_bn_finalize_fwd in eval mode, the launch list against the drop-in
modules in eval mode, the NHWC heads against the NCHW entry points on the fp32 copy of the same logits, whole validation passes
against validate(...) without `forward`, and two trainings with and without the flag."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(autouse=True)
def _storage_dtype_restored():
    from ramdsir import modules as M
    yield
    M.set_storage_dtype(None)


def _dt(dtype):
    from ramdsir import _lib as L
    return L.RD_BF16 if dtype == BF16 else L.RD_F32


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ coefficients
def _site_tensors(rng, Cc):
    g = rng.normal(0, 1.5, Cc).astype(np.float32)
    g[:3] = [-2.0, -0.125, 0.0]
    rv = rng.uniform(0.5, 2, Cc).astype(np.float32)
    rv[:3] = [0.0, 1e-12, 1e4]
    b, rm = rng.normal(0, 1, Cc).astype(np.float32), rng.normal(0.5, 2, Cc).astype(np.float32)
    return [torch.from_numpy(t).to(DEV) for t in (g, b, rm, rv)]


def _run_coeffs(sites):
    """sites: [(gamma, beta, rm, rv, scale, shift, C)] -> return code of rd_bn_eval_coeffs over their device table."""
    from ramdsir import _lib as L, engine as E, infer as I
    raw = bytes(memoryview(I.site_table(sites)))
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    return L.lib().rd_bn_eval_coeffs(table.data_ptr(), len(sites), max(s[6] for s in sites), E.EPS, _st()), table


@pytest.mark.parametrize('channels', [[8], [16] * 3 + [32] * 3 + [64] * 3 + [128] * 3 + [256] * 3 + [128, 128, 64, 64, 64, 32, 32, 32, 16, 16, 16]])
def test_coefficients_equal_the_eval_finalize_bit_for_bit(channels):
    """One rd_bn_eval_coeffs launch over the table against one rd_bn_finalize_fwd(training = 0) per site: the same uint32 patterns.
    running_var holds 0, 1e-12 and 1e4, gamma negative values and 0."""
    from ramdsir import _lib as L, engine as E, infer as I
    rng = np.random.RandomState(len(channels))
    sites, refs = [], []
    for Cc in channels:
        g, b, rm, rv = _site_tensors(rng, Cc)
        sc, sh = torch.full((Cc,), 7.0, device=DEV), torch.full((Cc,), 7.0, device=DEV)
        sites.append((g, b, rm, rv, sc, sh, Cc))
        out = torch.zeros(4, Cc, device=DEV)
        d = L.RdBnFwd()
        d.scale, d.shift, d.mean, d.invstd = (out[i].data_ptr() for i in range(4))
        d.gamma[0], d.beta[0], d.running_mean[0], d.running_var[0] = g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr()
        d.count[0], d.C, d.G, d.eps, d.momentum, d.training = 1.0, Cc, 1, E.EPS, E.MOMENTUM, 0
        L.check(L.lib().rd_bn_finalize_fwd(C.byref(d), _st()), 'rd_bn_finalize_fwd')
        refs.append(out)
    rc, table = _run_coeffs(sites)
    assert rc == 0
    torch.cuda.synchronize()
    for i, ((g, b, rm, rv, sc, sh, Cc), ref) in enumerate(zip(sites, refs)):
        assert torch.equal(sc.view(torch.int32), ref[0].view(torch.int32)), i
        assert torch.equal(sh.view(torch.int32), ref[1].view(torch.int32)), i
        assert torch.isfinite(sc).all() and torch.isfinite(sh).all()
        ms, mh = I.eval_coeffs_model(g.cpu().numpy(), b.cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy())
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), ms.view(np.uint32)), i       # the numpy model states the kernel
        assert np.array_equal(sh.cpu().numpy().view(np.uint32), mh.view(np.uint32)), i


def test_coefficients_refuse_a_null_pointer_and_launch_nothing():
    from ramdsir import _lib as L, engine as E, infer as I
    rng = np.random.RandomState(1)
    sites = []
    for Cc in (8, 16):
        g, b, rm, rv = _site_tensors(rng, Cc)
        sites.append([g, b, rm, rv, torch.full((Cc,), 7.0, device=DEV), torch.full((Cc,), 7.0, device=DEV), Cc])
    arr = I.site_table(sites)
    for field in ('gamma', 'beta', 'running_mean', 'running_var', 'scale', 'shift'):
        bad = (L.RdBnEvalSite * 2)()
        C.memmove(bad, arr, C.sizeof(arr))
        setattr(bad[1], field, None)
        table = torch.frombuffer(bytearray(bytes(memoryview(bad))), dtype=torch.uint8).to(DEV)
        assert L.lib().rd_bn_eval_coeffs(table.data_ptr(), 2, 16, E.EPS, _st()) == -1, field
    table = torch.frombuffer(bytearray(bytes(memoryview(arr))), dtype=torch.uint8).to(DEV)
    assert L.lib().rd_bn_eval_coeffs(table.data_ptr(), 2, 8, E.EPS, _st()) == -1            # a site wider than max_C
    assert L.lib().rd_bn_eval_coeffs(None, 2, 16, E.EPS, _st()) == -1
    assert L.lib().rd_bn_eval_coeffs(table.data_ptr(), 0, 16, E.EPS, _st()) == -1
    torch.cuda.synchronize()
    for s in sites:
        assert bool((s[4] == 7.0).all()) and bool((s[5] == 7.0).all())                     # the outputs stay untouched
    assert L.lib().rd_bn_eval_coeffs(table.data_ptr(), 2, 16, E.EPS, _st()) == 0
    torch.cuda.synchronize()
    assert not bool((sites[0][4] == 7.0).all())


# ------------------------------------------------------------------------------------------------ forward
def _modules(seed, sharpen=10.0):
    """Encoder + Decoder with random parameters (BatchNorm affines included) and perturbed running statistics: mean != 0, var in
    [0.5, 2]; the output conv scaled so that the masks have structure."""
    from networks.unet import Encoder, Decoder
    torch.manual_seed(seed)
    enc, dec = Encoder().to(DEV), Decoder(num_classes=2).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in list(enc.modules()) + list(dec.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.numel()
                m.weight.copy_(torch.empty(n).uniform_(0.5, 1.5, generator=g) * (torch.rand(n, generator=g) < 0.9).float().mul(2).sub(1))
                m.bias.copy_(torch.empty(n).normal_(0, 0.3, generator=g))
                m.running_mean.copy_(torch.empty(n).normal_(0.2, 0.5, generator=g))
                m.running_var.copy_(torch.empty(n).uniform_(0.5, 2.0, generator=g))
            elif isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(torch.empty(m.bias.numel()).normal_(0, 0.1, generator=g))
        dec.out1.weight.mul_(sharpen)
    return enc.eval(), dec.eval()


def _fill(fwd, x):
    """x NCHW fp32 -> the plan's input through rd_nchw_to_nhwc (the conversion the Encoder module applies)."""
    from ramdsir import _lib as L
    N, Cc, H, W = x.shape
    inp = fwd.input(N, H, W)
    L.check(L.lib().rd_nchw_to_nhwc(x.contiguous().data_ptr(), inp.data_ptr(), N, Cc, H, W, inp.shape[3], fwd.dt, _st()), 'rd_nchw_to_nhwc')


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('dtype,shape', [(BF16, (1, 32, 32)), (BF16, (3, 48, 80)), (BF16, (8, 256, 256)), (F32, (3, 48, 80))])
def test_forward_equals_the_modules_bit_for_bit(dtype, shape):
    """EvalForward.from_modules(...).logits_nchw against seg_decoder(encoder(x)) of the same modules in eval mode and the same storage
    dtype: the same fp32 bit patterns.  Twice (no state leaks between calls), then after a parameter and a running statistic have
    changed and refresh() (freshness); without refresh() the old coefficients and weights would still be in use."""
    from ramdsir import modules as M
    from ramdsir.infer import EvalForward
    M.set_storage_dtype(dtype)
    enc, dec = _modules(seed=7)
    N, H, W = shape
    x = torch.empty(N, 3, H, W, device=DEV).uniform_(-1, 1, generator=torch.Generator(device=DEV).manual_seed(3))
    fwd = EvalForward.from_modules(enc, dec)
    assert fwd.dtype == dtype and fwd.launches(N, H, W) == {'rd_conv': 27, 'rd_pool_fwd': 4}
    with torch.no_grad():
        ref = dec(enc(x))
        fwd.refresh()
        _fill(fwd, x)
        raw = fwd.run(N, H, W)
        assert tuple(raw.shape) == (N, H, W, 2) and raw.dtype == dtype
        got = fwd.logits_nchw(N, H, W)
        assert torch.isfinite(ref).all() and float(ref.std()) > 0
        assert _same_bits(got, ref), float((got - ref).abs().max())
        fwd.run(N, H, W)
        assert _same_bits(fwd.logits_nchw(N, H, W), ref)
        enc.convd2.conv2.weight.mul_(1.25)
        enc.convd3.bn1.running_var.mul_(1.5)
        dec.convu2.bn3.bias.add_(0.25)
        dec.out1.bias.add_(0.5)
        ref2 = dec(enc(x))
        assert not torch.equal(ref2, ref)
        fwd.refresh()
        fwd.run(N, H, W)
        assert _same_bits(fwd.logits_nchw(N, H, W), ref2)


def test_eval_forward_refuses_what_it_does_not_cover():
    from networks.unet import Encoder, Decoder
    from ramdsir.infer import EvalForward
    with pytest.raises(ValueError, match='norm'):
        EvalForward.from_modules(Encoder(norm='gn').to(DEV), Decoder(norm='gn').to(DEV))
    with pytest.raises(ValueError, match='norm'):
        EvalForward.from_modules(Encoder().to(DEV), Decoder(norm='in').to(DEV))
    with pytest.raises(ValueError, match='GPU'):
        EvalForward.from_modules(Encoder(), Decoder())
    with pytest.raises(ValueError):
        EvalForward.from_trainer(object())
    fwd = EvalForward.from_modules(Encoder().to(DEV), Decoder().to(DEV))
    with pytest.raises(ValueError, match='16'):
        fwd.input(1, 40, 32)


# ------------------------------------------------------------------------------------------------ heads
def _nhwc(lg, dtype, cstride, rng):
    """NCHW fp32 logits -> (NHWC tensor in `dtype` with channel stride `cstride` whose pad channels hold junk, the fp32 NCHW copy of
    what it stores: the exactly widened values)."""
    B, K, H, W = lg.shape
    t = torch.from_numpy(rng.normal(0, 50, (B, H, W, cstride)).astype(np.float32)).to(DEV).to(dtype)
    t[..., :K] = torch.from_numpy(lg).to(DEV).permute(0, 2, 3, 1).to(dtype)
    return t.contiguous(), t[..., :K].float().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('cstride', [2, 8])
def test_threshold_nhwc_equals_threshold(dtype, cstride):
    """rd_val_threshold_nhwc against rd_val_threshold fed the NCHW fp32 copy of the same logits: S = (32, 48) to three native sizes
    in one call, and B = 33 tiny images (one more than RD_VAL_CHUNK)."""
    from ramdsir import gpu_val as G, _lib as L
    import gpu_val_cases as GC
    rng = np.random.RandomState(cstride)
    for sizes in ([(37, 53), (20, 17), (32, 48)], [(5 + i % 4, 3 + i % 5) for i in range(L.VAL_CHUNK + 1)]):
        B = len(sizes)
        lg = GC.cone_logits(seed=B, n=B, S=48)[:, :, :32, :] * 0.5 + 1.0          # (B, 2, 32, 48), values on both sides of the threshold
        t, copy = _nhwc(lg, dtype, cstride, rng)
        recs, nbytes = G.image_records(sizes)
        ref = G.threshold(copy, recs, B, nbytes)
        got = G.threshold_nhwc(t, recs, B, nbytes)
        assert torch.equal(got, ref), sizes[:3]
        assert 0.0 < float(ref.float().mean()) < 1.0                            # (the test data: both values occur)
    # bad records and arguments: -1, nothing launched
    mask = torch.full((nbytes,), 9, dtype=torch.uint8, device=DEV)
    lib, dt = L.lib(), _dt(dtype)
    assert lib.rd_val_threshold_nhwc(t.data_ptr(), dt, cstride, B, 32, 48, recs, mask.data_ptr(), nbytes - 1, _st()) == -1
    assert lib.rd_val_threshold_nhwc(t.data_ptr(), dt, 1, B, 32, 48, recs, mask.data_ptr(), nbytes, _st()) == -1
    assert lib.rd_val_threshold_nhwc(t.data_ptr(), 2, cstride, B, 32, 48, recs, mask.data_ptr(), nbytes, _st()) == -1
    assert lib.rd_val_threshold_nhwc(None, dt, cstride, B, 32, 48, recs, mask.data_ptr(), nbytes, _st()) == -1
    bad, _ = G.image_records([(4, 0)])
    assert lib.rd_val_threshold_nhwc(t.data_ptr(), dt, cstride, 1, 32, 48, bad, mask.data_ptr(), nbytes, _st()) == -1
    torch.cuda.synchronize()
    assert bool((mask == 9).all())


@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('bs', [3, 8])
def test_vol_stack_nhwc_equals_stack_then_layout_conversion(dtype, bs):
    """rd_vol_stack_nhwc against rd_vol_stack + rd_nchw_to_nhwc at (D, H, W) = (7, 16, 24): the unpadded stride the plan uses and one
    16-byte slot (pad channels zero), full batches and batches with empty slots."""
    from ramdsir import gpu_val_volumes as V, _lib as L
    D, H, W = 7, 16, 24
    rng = np.random.RandomState(bs)
    vol = torch.from_numpy(rng.normal(0, 1, (D, H, W)).astype(np.float32)).to(DEV)
    # bs 3: a full batch and a ragged one; bs 8: every frame of the volume and three empty slots; an all-empty batch; a gap
    batches = (V.frame_batches(D, bs) or [list(range(1, D - 1)) + [-1] * (bs - (D - 2))]) + [[-1] * bs, [2, -1, 5] + [-1] * (bs - 3)]
    assert any(-1 in f and max(f) > 0 for f in batches)
    for cs in (3, 8 if dtype == BF16 else 4):
        for frames in batches:
            ref = torch.full((bs, H, W, cs), 3.0, device=DEV).to(dtype)
            ref.zero_()
            L.check(L.lib().rd_nchw_to_nhwc(V.stack(vol, frames).data_ptr(), ref.data_ptr(), bs, 3, H, W, cs, _dt(dtype), _st()), 'nchw_to_nhwc')
            got = torch.full((bs, H, W, cs), 3.0, device=DEV).to(dtype)                    # junk everywhere: the kernel writes the pad too
            V.stack_nhwc(vol, frames, got)
            assert torch.equal(got.view(torch.int16 if dtype == BF16 else torch.int32), ref.view(torch.int16 if dtype == BF16 else torch.int32)), (cs, frames)
            assert not bool(got[..., 3:].any())
    out = torch.full((bs, H, W, 3), 3.0, device=DEV).to(dtype)
    lib, fr = L.lib(), V._frames
    assert lib.rd_vol_stack_nhwc(vol.data_ptr(), D, H, W, fr([D - 1] + [-1] * (bs - 1)), bs, out.data_ptr(), _dt(dtype), 3, _st()) == -1
    assert lib.rd_vol_stack_nhwc(vol.data_ptr(), D, H, W, fr([3, 2] + [-1] * (bs - 2)), bs, out.data_ptr(), _dt(dtype), 3, _st()) == -1
    assert lib.rd_vol_stack_nhwc(vol.data_ptr(), D, H, W, fr([1] + [-1] * (bs - 1)), bs, out.data_ptr(), _dt(dtype), 2, _st()) == -1
    assert lib.rd_vol_stack_nhwc(vol.data_ptr(), D, H, W, fr([1] + [-1] * (bs - 1)), bs, None, _dt(dtype), 3, _st()) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('shape,bs,cstride', [((7, 16, 24), 3, 2), ((12, 7, 9), 4, 2), ((7, 16, 24), 8, 8), ((12, 7, 9), 4, 3)])
def test_vol_argmax_nhwc_equals_argmax(dtype, shape, bs, cstride):
    """rd_vol_argmax_nhwc against rd_vol_argmax on the fp32 NCHW copy of the same logits: exact ties l1 == l0 (bf16 rounding adds
    more), gt_empty slices, empty slots, untouched slices; a plane size that is no multiple of four and a prediction buffer at an odd
    address take the element path."""
    from ramdsir import gpu_val_volumes as V, _lib as L
    D, H, W = shape
    rng = np.random.RandomState(D + bs + cstride)
    gt_empty = (rng.uniform(size=D) < 0.3).astype(np.uint8)
    gt_empty[1], gt_empty[2] = 1, 0
    e = torch.from_numpy(gt_empty).to(DEV)
    for shift in (0, 1):
        hold = [torch.full((D * H * W + 4,), 5, dtype=torch.uint8, device=DEV) for _ in range(2)]
        pred, want = (h[shift:shift + D * H * W] for h in hold)
        batches = (V.frame_batches(D, bs) or [list(range(1, D - 1)) + [-1] * (bs - (D - 2))]) + [[-1] * bs]
        n_tie = 0
        for frames in batches:
            lg = rng.normal(0, 1.5, (bs, 2, H, W)).astype(np.float32)
            tie = rng.uniform(size=(bs, H, W)) < 0.05
            lg[:, 1][tie] = lg[:, 0][tie]
            t, copy = _nhwc(lg, dtype, cstride, rng)
            n_tie += int((copy[:, 0] == copy[:, 1]).sum())
            V.argmax(copy, frames, e, want, shape)
            V.argmax_nhwc(t, frames, e, pred, shape)
        assert n_tie > 0
        assert torch.equal(hold[0], hold[1]), shift
        got = pred.cpu().numpy().reshape(shape)
        assert (got[1] == 0).all() and 0.1 < got[2].mean() < 0.9                           # an empty ground truth; a live slice
        assert (got[0] == 5).all() and (got[D - 1] == 5).all()                             # slices no batch reaches keep their contents
    lib, fr, dt = L.lib(), V._frames, _dt(dtype)
    pred.fill_(5)
    assert lib.rd_vol_argmax_nhwc(t.data_ptr(), dt, cstride, bs, H, W, fr([D - 1] + [-1] * (bs - 1)), e.data_ptr(), D, pred.data_ptr(), _st()) == -1
    assert lib.rd_vol_argmax_nhwc(t.data_ptr(), dt, 1, bs, H, W, fr([1] + [-1] * (bs - 1)), e.data_ptr(), D, pred.data_ptr(), _st()) == -1
    assert lib.rd_vol_argmax_nhwc(t.data_ptr(), dt, cstride, bs, H, W, fr([1] + [-1] * (bs - 1)), None, D, pred.data_ptr(), _st()) == -1
    torch.cuda.synchronize()
    assert bool((pred == 5).all())


# ------------------------------------------------------------------------------------------------ whole passes
@pytest.mark.parametrize('dtype', [BF16, F32])
def test_whole_fundus_pass_equals_the_module_pass(dtype):
    """11 synthetic test images of mixed native sizes, test batch 8 (a ragged batch of 3): thresholded masks, post-processed masks and
    the int32 counts (hence the Dice doubles) of validate(..., forward=EvalForward) equal those of validate(...), byte for byte."""
    from ramdsir import gpu_val as G, modules as M
    from ramdsir.infer import EvalForward
    M.set_storage_dtype(dtype)
    enc, dec = _modules(seed=21)
    rng = np.random.RandomState(4)
    sizes = [(37, 53), (64, 48), (80, 80), (100, 90), (256, 256), (33, 47), (300, 280), (64, 64), (51, 50), (90, 100), (128, 96)]
    n = len(sizes)
    low = torch.from_numpy(rng.normal(0, 1, (n, 3, 16, 16)).astype(np.float32))
    inputs = (torch.nn.functional.interpolate(low, size=(256, 256), mode='bilinear') + 0.2 * torch.randn(n, 3, 256, 256, generator=torch.Generator().manual_seed(5))).to(DEV)
    gt_offs, off = [], 0
    for h, w in sizes:
        gt_offs.append(off)
        off += 2 * h * w
    gt = torch.from_numpy((rng.uniform(size=off) < 0.4).astype(np.uint8)).to(DEV)
    res = G.ValResident(inputs.contiguous(), gt, gt_offs, sizes, ['img%d' % i for i in range(n)])
    fwd = EvalForward.from_modules(enc, dec)
    keep_a, keep_b = [], []
    dice_a = G.validate(enc, dec, res, 8, keep=keep_a)
    dice_b = G.validate(enc, dec, res, 8, keep=keep_b, forward=fwd)
    assert tuple(res.inputs_nhwc.shape) == (n, 256, 256, 3) and res.inputs_nhwc.dtype == dtype
    assert len(keep_a) == len(keep_b) == 2
    share = []
    for (ma, pa, _), (mb, pb, _) in zip(keep_a, keep_b):
        assert torch.equal(ma, mb) and torch.equal(pa, pb)
        share.append(float(ma.float().mean()))
    print('foreground share of the thresholded masks per batch:', share)
    assert any(0.0 < s < 1.0 for s in share)
    assert dice_a == dice_b and len(dice_b) == n
    assert G.validate(enc, dec, res, 8, forward=fwd) == dice_a              # a second pass: plans and the resident copy reused


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_whole_prostate_pass_equals_the_module_pass(dtype):
    """Three volumes with D = 9, 12 and 5 at 64 x 64, test batch 4: pred, post and the counts are identical."""
    from ramdsir import gpu_val_volumes as V, modules as M
    from ramdsir.infer import EvalForward
    M.set_storage_dtype(dtype)
    enc, dec = _modules(seed=22, sharpen=1.0)
    rng = np.random.RandomState(6)
    shapes = [(9, 64, 64), (12, 64, 64), (5, 64, 64)]
    volumes, gts, empties = [], [], []
    for D, H, W in shapes:
        v = rng.uniform(0, 0.3, (D, H, W)).astype(np.float32)
        v[1:D - 1, 20:44, 16:40] += 0.6
        g = np.zeros((D, H, W), np.uint8)
        g[1:D - 1, 20:44, 16:40] = 1
        g[2] = 0
        volumes.append(torch.from_numpy(v).to(DEV))
        gts.append(g.reshape(-1))
        empties.append(torch.from_numpy((g.reshape(D, -1).sum(1) == 0).astype(np.uint8)).to(DEV))
    res = V.VolResident(volumes, torch.from_numpy(np.concatenate(gts)).to(DEV), empties, shapes, ['v%d' % i for i in range(3)], 0)
    with torch.no_grad():                                   # centre the class margin: about half of the voxels on either side
        lg = dec(enc(V.stack(volumes[0], [1, 2, 3, 4])))
        dec.out1.bias[1] += float((lg[:, 0] - lg[:, 1]).median())
    fwd = EvalForward.from_modules(enc, dec)
    keep_a, keep_b = {}, {}
    dice_a = V.validate(enc, dec, res, 4, keep=keep_a)
    dice_b = V.validate(enc, dec, res, 4, keep=keep_b, forward=fwd)
    for i in range(3):
        assert np.array_equal(keep_a['pred'][i], keep_b['pred'][i]), i
        assert np.array_equal(keep_a['post'][i], keep_b['post'][i]), i
    print('foreground share of the predictions:', [float(p.mean()) for p in keep_b['pred']])
    assert all(0.02 < float(p.mean()) < 0.98 for p in keep_b['pred'])
    assert keep_a['counts'] == keep_b['counts'] and dice_a == dice_b


# ------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize('dtype', [BF16, F32])
def test_from_trainer_reads_the_pack_the_last_step_left_behind(dtype):
    """EvalForward.from_trainer on a small FusedTrainer whose storage dtype is the module path's: it shares ts.wpack and never
    repacks.  After two steps -- the first pipelined, the second the classical, non-pipelined one -- and a synchronize, logits_nchw
    equals the modules' forward, which repacks the current parameters itself: a stale pack or stale coefficients would show."""
    from networks.unet import Encoder, Decoder, Rec_Decoder
    from ramdsir import modules as M
    from ramdsir.infer import EvalForward
    from ramdsir.trainer import FusedTrainer
    M.set_storage_dtype(dtype)
    torch.manual_seed(31)
    enc, dec = Encoder().to(DEV), Decoder(num_classes=2).to(DEV)
    rec = Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(DEV)
    bs, S = [1, 2, 1], 32
    B = sum(bs)
    tr = FusedTrainer(enc, dec, rec, bs, S, S, dataset='fundus', consistency='kd', lr=2e-2, total_iters=8, dtype=dtype)
    fwd = EvalForward.from_trainer(tr)
    assert fwd.wpack is tr.ts.wpack and not fwd.owns_pack and fwd.dtype == dtype
    g = torch.Generator().manual_seed(32)

    def batch():
        src = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV)
        trg = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(DEV)
        disc = (torch.rand(B, 1, S, S, generator=g) > 0.5).float()
        mask = torch.cat([disc * (torch.rand(B, 1, S, S, generator=g) > 0.5).float(), disc], 1).to(DEV)
        return src, trg, torch.rand(B, generator=g).to(DEV), mask
    x = torch.empty(3, 3, S, S).uniform_(-1, 1, generator=g).to(DEV)

    def compare():
        torch.cuda.synchronize()
        with torch.no_grad():
            fwd.refresh()
            _fill(fwd, x)
            fwd.run(3, S, S)
            got = fwd.logits_nchw(3, S, S)
            enc.eval(), dec.eval()
            ref = dec(enc(x))
            enc.train(), dec.train()
        assert torch.isfinite(ref).all()
        assert _same_bits(got, ref), float((got - ref).abs().max())
        return ref
    ref0 = compare()
    b0, b1 = batch(), batch()
    tr.step(*b0, next_batch=b1)
    ref1 = compare()                                        # behind a pipelined step
    tr.step(*b1)
    ref2 = compare()                                        # behind the epoch's last, non-pipelined step
    assert not torch.equal(ref0, ref1) and not torch.equal(ref1, ref2)        # the parameters did move
    # a bf16 step validated by fp32 modules (train.py's default): the object owns its pack and refresh() repacks it
    if dtype == BF16:
        M.set_storage_dtype(F32)
        own = EvalForward.from_trainer(tr)
        assert own.owns_pack and own.dtype == F32 and own.wpack is not tr.ts.wpack
        fwd = own
        compare()


# ------------------------------------------------------------------------------------------------ train.py
def _csv_layout(line):
    return re.sub(r'[-+]?\d+\.\d+(e[-+]?\d+)?', '<f>', line)


def _train(data, out, dataset, extra):
    doms = '1,2,3' if dataset == 'fundus' else '1,2,3,4,5'
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs', doms,
           '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd', '--save_path', out,
           '--epochs', '2', '--max_iters', '4', '--num_workers', '0', '--log_every', '2', '--deterministic']
    return subprocess.run(cmd + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


def _same_training(tmp_path, data, dataset, base, marker):
    runs = []
    for name, extra in (('modules', base), ('fused', base + ['--fused_val'])):
        out = str(tmp_path / name)
        r = _train(data, out, dataset, extra)
        log = r.stdout.decode()
        assert r.returncode == 0, log[-3000:]
        assert (marker in log) == (name == 'fused'), log[-3000:]
        assert log.count('val_cup_dice' if dataset == 'fundus' else 'val_dice') == 2
        runs.append((torch.load(os.path.join(out, 'final_model.pth'), map_location='cpu'),
                     sorted(f for f in os.listdir(out) if f.startswith('model_')), open(os.path.join(out, '0_val_log.csv')).read()))
    (ck0, best0, csv0), (ck1, best1, csv1) = runs
    assert len(csv0.strip().splitlines()) == 2
    assert csv1 == csv0                                     # the text: every digit of both epochs' lines
    assert best1 == best0 and best0
    for part in ck0:
        assert list(ck0[part]) == list(ck1[part])
        for k in ck0[part]:
            assert torch.equal(ck0[part][k], ck1[part][k]), (part, k)


def test_train_cli_fused_val_fundus_gives_the_same_model_and_numbers(tmp_path):
    """Two --deterministic trainings of two epochs with --gpu_val, without and with --fused_val, in train.py's default dtypes (a bf16
    step validated in fp32 storage: EvalForward owns its pack).  The second epoch's CSV line is what catches stale weights or
    coefficients."""
    data = str(tmp_path / 'data')
    SD.make_fundus_tree(data, n_train=8, n_test=10, hw=(136, 152), vary=False)       # 10 test images: a batch of 8 and one of 2
    _same_training(tmp_path, data, 'fundus', ['--gpu_val'], 'fused_val: validation forward as one launch list per batch, fp32 storage, its own')


def test_train_cli_fused_val_prostate_gives_the_same_model_and_numbers(tmp_path):
    """The same for --gpu_val_volumes with --dtype f32: step and validation share one storage dtype, so EvalForward reads the step's
    own weight pack and never repacks -- the second epoch's line proves that pack fresh."""
    from test_gpu_gpu_val_volumes import _write_volumes
    data = str(tmp_path / 'data')
    SD.make_prostate_tree(data, n=4, S=64)
    _write_volumes(os.path.join(data, 'prostate', 'ISBI'), [('Case00', 10, np.float32, (3,)), ('Case01', 13, np.int16, (1, 6)),
                                                            ('Case02', 5, np.float32, ())])
    _same_training(tmp_path, data, 'prostate', ['--gpu_val_volumes', '--test_batch_size', '4', '--dtype', 'f32'],
                   "fused_val: validation forward as one launch list per batch, fp32 storage, the step's")
