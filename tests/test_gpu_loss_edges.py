"""-m gpu: rd_seg_loss, rd_rec_loss and rd_adam_step (csrc/loss.hip) at the sizes where their launch geometry changes, against plain
float64 references of the same operations.

tests/test_gpu_ops.py runs these kernels at 360 / 720 pixels, 288 elements per image and 1000 parameters: 3 blocks, 1 block, 4 blocks.
Every shape here is chosen from loss.hip's own formulas (restated in tests/loss_index_model.py and ASSERTED in
test_shapes_reach_the_edges_they_are_chosen_for, so a later change of a cap makes that test say which shape no longer reaches its edge):

  seg loss, seg_blocks = min(1024, ceil(npix / 256)), fast-path stride = blocks x 256 with SL_U = 5 pixels in flight per thread
    B=3, 45x67     9,045 px     36 blocks: seg_loss_final_kernel's `b += 32` loop takes a second trip for 4 of its 32 rows
    B=1, 513x515   264,195 px   1033 -> 1024 blocks (the cap); u = 1 valid for 2051 pixels, masked for the rest; u >= 2 all masked;
                                the generic path's grid-stride loop takes a second trip for those 2051; B = 1: the `n + B` offset
    B=2, 810x810   1,312,200 px the fast path's outer loop takes a second trip for 1480 pixels (5 x 262,144 = 1,310,720)
  rec loss, rec_bx = min(256, ceil(per_img / 1024)), rec_loss_final_kernel reads gs[g] * bx .. gs[g + 1] * bx
    B=5, 150x150x3 67,500 el    bx = 66, 4 trips per thread, the last ragged (16,812 of 16,896 threads)
    B=1, 300x300x3 270,000 el   bx = 264 -> 256 (the cap), 5 trips, G = 1
    B=16 / 20, 23x29x3          G = 16 = RD_MAX_GROUPS: the final kernel is one 1024-thread block
    B=1, 2048x2100x3 12,902,400 el: 319,486 indices past 12,582,914, the first one whose float-reciprocal split needs its correction
  Adam, blocks = min(4096, ceil(n / 256))
    n = 1,048,869  4098 -> 4096 blocks: the grid-stride loop takes a second, ragged trip for 293 elements

References are float64 (oracle/losses.py and torch's functionals with autograd for the segmentation losses, closed forms for the
restoration loss and Adam); tolerances are those of test_gpu_ops.py::test_seg_loss_* / test_rec_loss, Adam's are derived below.
Every output buffer holds NaN before the launch, and the workspace, the outputs and the loss slots lie between 4 KiB sentinel
regions that must come back intact."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ramdsir import _lib as L          # noqa: E402
import gpu_util as U                   # noqa: E402
import loss_index_model as M           # noqa: E402

DTYPES = ['f32', 'bf16']
GUARD, SENT = 4096, 0xA5
EPS24 = 2.0 ** -24                     # unit roundoff of float32

SMALL, CAP, TWO_TRIPS = (3, 45, 67), (1, 513, 515), (2, 810, 810)           # (B, H, W) of the segmentation cases


class Guarded:
    """`nbytes` of device memory as a tensor of `dtype` filled with `fill`, with GUARD sentinel bytes in front and behind."""
    def __init__(self, nbytes, dtype, fill=float('nan')):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=U.dev())
        self.t = self.raw[GUARD:GUARD + self.nbytes].view(dtype)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.nbytes:] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _scale(dtype):
    return 0.5 if dtype == 'bf16' else 5.0          # test_gpu_ops.py::test_seg_loss_* / test_rec_loss


# ------------------------------------------------------------------------------------ launch geometry
def test_shapes_reach_the_edges_they_are_chosen_for():
    """Arithmetic on seg_blocks / rec_bx / the Adam cap only: each shape of this file reaches the edge its docstring line names."""
    def seg(bhw):
        npix = bhw[0] * bhw[1] * bhw[2]
        nb = M.seg_blocks(npix)
        return npix, nb, nb * 256
    npix, nb, stride = seg(SMALL)
    assert (npix, nb) == (9045, 36) and 32 < nb < 64 and nb - 32 == 4            # second trip of `b += 32` for rows 0..3 only
    assert npix <= stride                                                        # every u >= 1 masked, as in test_gpu_ops.py
    npix, nb, stride = seg(CAP)
    assert npix == 264195 and (npix + 255) // 256 == 1033 and nb == 1024         # the cap
    assert npix - stride == 2051 and npix < 2 * stride                           # u = 1: 2051 valid lanes; u >= 2: none
    npix, nb, stride = seg(TWO_TRIPS)
    assert npix == 1312200 and nb == 1024 and npix - stride * M.SL_U == 1480     # second trip of the outer loop, 1480 pixels
    assert 0 < npix - stride * M.SL_U < stride
    assert seg((2, 10, 18))[1] == 2 and seg((2, 12, 20))[1] == 2
    # restoration loss
    per = 150 * 150 * 3
    assert per == 67500 and M.rec_bx(per) == 66 and math.ceil(per / (66 * 256)) == 4 and per - 3 * 66 * 256 == 16812
    per = 300 * 300 * 3
    assert per == 270000 and (per + 1023) // 1024 == 264 and M.rec_bx(per) == 256 and math.ceil(per / 65536) == 5
    assert M.rec_bx(23 * 29 * 3) == 2 and M.rec_bx(37 * 41 * 7) == 11 and M.rec_bx(37 * 41 * 1) == 2
    per = 2048 * 2100 * 3
    assert per == 12902400 and M.FIRST_WRONG_C3 < per < M.REC_LIMIT and per - M.FIRST_WRONG_C3 == 319486
    assert 2048 * 2731 * 3 == 16779264 >= M.REC_LIMIT
    assert L.MAXG == 16
    # Adam
    n = ADAM_N
    assert n == 1048869 and (n + 255) // 256 == 4098 and M.adam_blocks(n) == 4096 and n - 4096 * 256 == 293
    assert ADAM_HALF % 256 != 0 and 0 < ADAM_HALF < n


# ------------------------------------------------------------------------------------ segmentation losses
def seg_reference(lg, target, B, K, kind, cons, fdt):
    """The six loss values and d total / d logits, evaluated in `fdt` on the given (already storage-rounded) logits."""
    from oracle import losses as OL
    x = lg.to(fdt).requires_grad_(True)
    if kind == 0:
        t = target.to(fdt)
        p1, p2 = torch.sigmoid(x[:B]), torch.sigmoid(x[B:])
        comps = [OL.bce(p1, t), OL.dice_loss(p1, t), OL.bce(p2, t), OL.dice_loss(p2, t)]
    else:
        p1, p2 = torch.softmax(x[:B], 1), torch.softmax(x[B:], 1)
        comps = [F.cross_entropy(x[:B], target), OL.dice_loss_multi(p1, target, K, 0),
                 F.cross_entropy(x[B:], target), OL.dice_loss_multi(p2, target, K, 0)]
    c = OL.kd(p2, p1) if cons == 1 else (F.mse_loss(p2, p1) if cons == 2 else torch.zeros((), dtype=fdt))
    total = sum(comps) + 0.5 * c
    total.backward()
    return [float(v.detach()) for v in comps + [c, total]], x.grad


@functools.lru_cache(maxsize=2)
def seg_case(bhw, K, kind, cons, dtype, variant='hard'):
    """Seeded logits + target + the float64 reference, computed once per case and shared by every stride / repeat of it."""
    B, H, W = bhw
    gen = _gen('seg', bhw, K, kind, cons, dtype, variant)
    lg = U.rnd(2 * torch.randn(2 * B, K, H, W, generator=gen), dtype)
    if kind == 0:
        target = (torch.rand(B, K, H, W, generator=gen) > 0.6).float()
        if variant == 'soft':                                   # mask values in {0, 0.25, 1}: t * t != t in the dice denominator
            target = torch.where(torch.rand(B, K, H, W, generator=gen) > 0.5, target, 0.25 * target)
            assert sorted(set(target.flatten().tolist())) == [0.0, 0.25, 1.0]
    else:
        nlab = K - 1 if variant == 'absent' else K              # 'absent': the last class never occurs in the target
        target = torch.randint(0, nlab, (B, H, W), generator=gen)
        assert sorted(set(target.flatten().tolist())) == list(range(nlab))
    ref_losses, ref_grad = seg_reference(lg, target, B, K, kind, cons, torch.float64)
    return lg, target, ref_losses, ref_grad


def seg_call(lgd, target_dev, bhw, K, kind, cons, dtype, cs, with_grad=True, check_rc=True):
    """One rd_seg_loss call with guarded NaN-planted buffers -> (return code, losses[8] on the CPU, dlogits [2B][H][W][cs] or None)."""
    B, H, W = bhw
    tdt = U.DT[dtype][1]
    p = L.RdSegLoss()
    p.B, p.H, p.W, p.K, p.kind, p.consistency, p.cons_weight = B, H, W, K, kind, cons, 0.5
    p.dlogits_cstride = 0 if cs == K else cs
    ws_bytes = L.lib().rd_seg_loss_workspace(C.byref(p))
    assert ws_bytes == (M.seg_blocks(B * H * W) + 1) * M.NS_MAX * 4
    ws = Guarded(ws_bytes, torch.float32)                       # EXACTLY the workspace the library asks for
    losses = Guarded(8 * 4, torch.float32)
    dl = Guarded(2 * B * H * W * cs * torch.empty((), dtype=tdt).element_size(), tdt) if with_grad else None
    p.logits, p.target, p.partial, p.losses_out = lgd.data_ptr(), target_dev.data_ptr(), ws.ptr(), losses.ptr()
    p.dlogits = dl.ptr() if with_grad else None
    rc = L.lib().rd_seg_loss(C.byref(p), U.DT[dtype][0], None)
    torch.cuda.synchronize()
    assert ws.intact() and losses.intact() and (dl is None or dl.intact()), 'a sentinel region around the workspace / outputs was written'
    if check_rc:
        L.check(rc, 'segloss')
    return rc, losses.t.cpu(), (dl.t.view(2 * B, H, W, cs) if with_grad else None), ws


def check_seg(bhw, K, kind, cons, dtype, variant='hard', case=None):
    lg, target, ref_losses, ref_grad = case or seg_case(bhw, K, kind, cons, dtype, variant)
    lgd, td = U.nhwc(lg, dtype), target.to(U.dev())
    for cs in (K, 8) + ((4,) if K == 3 else ()):                # dense, padded to one 16-byte slot, and 3 in 4
        _, losses, dl, _ = seg_call(lgd, td, bhw, K, kind, cons, dtype, cs)
        got = U.from_nhwc(dl[..., :K])
        err = float((got - ref_grad.float()).abs().max()) / (float(ref_grad.float().pow(2).mean().sqrt()) + 1e-20)
        print('seg %s K=%d kind=%d cons=%d %s cs=%d: losses rel %.2e, dlogits max|diff|/rms %.2e' % (
            bhw, K, kind, cons, dtype, cs, max(abs(float(a) - b) / (abs(b) + 1e-30) for a, b in zip(losses[:6], ref_losses) if b != 0), err))
        np.testing.assert_allclose(losses[:6], ref_losses, rtol=2e-5, atol=1e-7)
        assert float(losses[6]) == 0.0 and float(losses[7]) == 0.0                  # written as zeros over the NaN pre-fill
        assert not bool(torch.isnan(dl[..., :K].float()).any())                    # every element written
        U.assert_close(got, ref_grad, dtype, 'dlogits cs=%d' % cs, scale=_scale(dtype))
        assert bool(torch.isnan(dl[..., K:].float()).all())                        # the pad is never written


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [0, 1, 2])
def test_seg_fast_path_36_blocks(dtype, cons):
    """kind 0, K = 2, 9045 pixels in 36 blocks: seg_loss_final_kernel's `b += 32` loop adds blocks 32..35 in a second trip."""
    check_seg(SMALL, 2, 0, cons, dtype)


@pytest.mark.parametrize('bhw,dtype,cons', [(CAP, 'f32', 1), (CAP, 'bf16', 2), (CAP, 'f32', 0), (TWO_TRIPS, 'f32', 2), (TWO_TRIPS, 'bf16', 1)])
def test_seg_fast_path_block_cap_and_second_outer_trip(bhw, dtype, cons):
    """kind 0, K = 2.  264,195 pixels: the 1024-block cap, the u = 1 slot valid in 2051 lanes and clamped + masked in the others of
    the same waves, B = 1 (the second half starts at image n + 1).  1,312,200 pixels: a second trip of the outer loop for 1480."""
    check_seg(bhw, 2, 0, cons, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [0, 1, 2])
def test_seg_fast_path_single_class(dtype, cons):
    """kind 0, K = 1 through the fast path's `k < K` guards (the k = 1 loads are clamped to class 0 and never accumulated)."""
    check_seg(SMALL, 1, 0, cons, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [1, 2])
@pytest.mark.parametrize('bhw,K', [(CAP, 3), (SMALL, 4)])
def test_seg_generic_path_sigmoid_three_and_four_classes(bhw, K, dtype, cons):
    """kind 0 with K in {3, 4}: the generic path (IEEE expf / logf / log1pf); at 264,195 pixels its grid-stride loop's second trip."""
    check_seg(bhw, K, 0, cons, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [1, 2])
@pytest.mark.parametrize('bhw,K,variant', [(CAP, 2, 'hard'), (SMALL, 4, 'hard'), ((2, 10, 18), 3, 'absent')])
def test_seg_softmax_path_up_to_four_classes(bhw, K, variant, dtype, cons):
    """kind 1.  K = 4 with labels from all four classes reads the per-class dice sums at 3 + 5 (k - 1) for k = 2, 3; K = 3 with
    class 2 absent from the target makes that class's dice term 1 - eps / (Z + eps)."""
    check_seg(bhw, K, 1, cons, dtype, variant)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [1, 2])
def test_seg_soft_targets(dtype, cons):
    """kind 0, K = 2, mask values in {0, 0.25, 1}: the dice denominator's sum of t * t is not the sum of t."""
    check_seg(SMALL, 2, 0, cons, dtype, 'soft')


SAT_VALUES = (30.0, 30.0, -30.0, -30.0, -120.0, -120.0)         # each against target 0 and target 1
SAT_TARGETS = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cons', [0, 2])
def test_seg_saturated_logits_follow_torch_float32_clamps(dtype, cons):
    """Logits of +30, -30 and -120 (all bf16 numbers): the float32 sigmoid is exactly 1, 9.4e-14 (p (1 - p) below the 1e-12 floor of
    ATen's binary_cross_entropy_backward) and exactly 0 in torch and in the kernel, so log p or log(1 - p) hits the -100 clamp.  The
    clamp positions are float32 semantics: the reference here is the FLOAT32 oracle.  (KD is infinite at p = 0 in the reference too,
    hence consistency 0 and 2 only.)"""
    bhw, K = (2, 12, 20), 2
    B, H, W = bhw
    gen = _gen('sat', dtype, cons)
    lg = U.rnd(2 * torch.randn(2 * B, K, H, W, generator=gen), dtype)
    mask = (torch.rand(B, K, H, W, generator=gen) > 0.6).float()
    for j, (v, t) in enumerate(zip(SAT_VALUES, SAT_TARGETS)):
        for k in range(K):
            lg[0, k, 0, j] = v                                  # first half, image 0
            lg[B + 1, k, 1, j] = v                              # second half, image 1
            mask[0, k, 0, j] = t
            mask[1, k, 1, j] = t
    assert torch.equal(U.rnd(lg, dtype), lg)
    p = torch.sigmoid(lg[0, 0, 0, :6])
    assert p[0] == 1 and p[1] == 1 and 0 < p[2] < 1e-12 and 0 < p[3] < 1e-12 and p[4] == 0 and p[5] == 0
    ref_losses, ref_grad = seg_reference(lg, mask, B, K, 0, cons, torch.float32)
    assert all(math.isfinite(v) for v in ref_losses) and bool(torch.isfinite(ref_grad).all())
    assert ref_losses[0] > 100.0 * 4 / mask.numel()             # the -100 clamp is in the reference's mean (4 elements at 100)
    check_seg(bhw, K, 0, cons, dtype, case=(lg, mask, ref_losses, ref_grad))        # assert_close requires every dlogits element finite


@pytest.mark.parametrize('kind,K,cons', [(0, 2, 1), (0, 4, 2), (1, 3, 1)])
def test_seg_losses_only_call_equals_the_call_with_dlogits(kind, K, cons):
    """dlogits == NULL: losses_out[0:6] bit for bit those of the full call, [6:8] zero, nothing else written (sentinels intact)."""
    lg, target, _, _ = seg_case(SMALL, K, kind, cons, 'f32')
    lgd, td = U.nhwc(lg, 'f32'), target.to(U.dev())
    _, full, _, _ = seg_call(lgd, td, SMALL, K, kind, cons, 'f32', K)
    _, only, none, _ = seg_call(lgd, td, SMALL, K, kind, cons, 'f32', K, with_grad=False)
    assert none is None
    assert torch.equal(_bits(full[:6]), _bits(only[:6]))
    assert float(only[6]) == 0.0 and float(only[7]) == 0.0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bhw,kind,K,cons', [(SMALL, 0, 2, 1), (CAP, 0, 2, 2), (SMALL, 1, 4, 1)])
def test_seg_loss_repeats_bit_for_bit(bhw, kind, K, cons, dtype):
    """The reductions are fixed-order: two identical calls give bitwise identical losses_out and dlogits."""
    lg, target, _, _ = seg_case(bhw, K, kind, cons, dtype)
    lgd, td = U.nhwc(lg, dtype), target.to(U.dev())
    _, l1, d1, _ = seg_call(lgd, td, bhw, K, kind, cons, dtype, K)
    _, l2, d2, _ = seg_call(lgd, td, bhw, K, kind, cons, dtype, K)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(d1), _bits(d2))


@pytest.mark.parametrize('kind,K', [(0, 0), (0, 5), (1, 1), (1, 5)])
def test_seg_loss_refuses_class_counts_outside_its_range(kind, K):
    """K = 0, K = 5 (> KMAX) and kind 1 with K = 1 return -1 and leave the NaN-planted outputs and workspace untouched."""
    bhw = (2, 10, 18)
    B, H, W = bhw
    lgd = torch.zeros(2 * B, H, W, 8, device=U.dev())
    td = torch.zeros(B, 8, H, W, device=U.dev()) if kind == 0 else torch.zeros(B, H, W, dtype=torch.int64, device=U.dev())
    rc, losses, dl, ws = seg_call(lgd, td, bhw, K, kind, 1, 'f32', 8, check_rc=False)
    assert rc == -1
    assert bool(torch.isnan(losses).all()) and bool(torch.isnan(dl).all()) and bool(torch.isnan(ws.t).all())


# ------------------------------------------------------------------------------------ restoration loss
def rec_reference(lg, tgt, gstart, lam):
    """float64, NHWC [B][H][W][C]: mse_loss(tanh(lg[group]), tgt[group]) per group and d (lam * sum) / d lg in closed form."""
    x, t = lg.double(), tgt.double()
    r = torch.tanh(x)
    d = r - t
    grad = torch.empty_like(x)
    mses = []
    for a, b in zip(gstart[:-1], gstart[1:]):
        cnt = float(d[a:b].numel())
        mses.append(float((d[a:b] * d[a:b]).sum() / cnt))
        grad[a:b] = (lam * 2.0 / cnt) * d[a:b] * (1.0 - r[a:b] * r[a:b])
    return mses, grad


def rec_call(lg, tgt, gstart, dtype, Ts, Ds, lam=0.1, explicit_strides=True):
    """One rd_rec_loss call on NHWC CPU tensors (values already storage-rounded): the target padded to Ts channels with 7.0, dlogits
    [B][H][W][Ds] planted with NaN, workspace of exactly rd_rec_loss_workspace bytes and mse_out[G] between sentinels."""
    B, H, W, Cc = lg.shape
    G = len(gstart) - 1
    tdt = U.DT[dtype][1]
    lgd = lg.to(tdt).to(U.dev())
    td = tgt.to(tdt)
    if Ts != Cc:
        td = torch.cat([td, torch.full((B, H, W, Ts - Cc), 7.0, dtype=tdt)], -1).contiguous()
    td = td.to(U.dev())
    ws_bytes = L.lib().rd_rec_loss_workspace(B, H, W, Cc)
    assert ws_bytes == B * M.rec_bx(H * W * Cc) * 4
    ws, out = Guarded(ws_bytes, torch.float32), Guarded(4 * G, torch.float32)
    dl = Guarded(B * H * W * Ds * lgd.element_size(), tdt)
    sa = (lambda s: s) if explicit_strides else (lambda s: 0 if s == Cc else s)
    rc = L.lib().rd_rec_loss(L.ptr(lgd), L.ptr(td), dl.ptr(), out.ptr(), ws.ptr(), B, H, W, Cc, sa(Ts), sa(Ds), G,
                             L.gstart_array(gstart), lam, U.DT[dtype][0], None)
    torch.cuda.synchronize()
    assert ws.intact() and out.intact() and dl.intact(), 'a sentinel region around the workspace / mse_out / dlogits was written'
    L.check(rc, 'recloss')
    return out.t.cpu(), dl.t.view(B, H, W, Ds)


def check_rec(B, H, W, Cc, gstart, dtype, Ts, Ds, explicit_strides=True):
    gen = _gen('rec', B, H, W, Cc, tuple(gstart), dtype)
    lg = U.rnd(torch.randn(B, H, W, Cc, generator=gen), dtype)
    tgt = U.rnd(torch.rand(B, H, W, Cc, generator=gen) * 2 - 1, dtype)
    mses, grad = rec_reference(lg, tgt, gstart, 0.1)
    out, dl = rec_call(lg, tgt, gstart, dtype, Ts, Ds, explicit_strides=explicit_strides)
    got = dl[..., :Cc].float().cpu()
    print('rec B=%d %dx%dx%d G=%d %s Ts=%d Ds=%d: mse rel %.2e, dlogits max|diff|/rms %.2e' % (
        B, H, W, Cc, len(gstart) - 1, dtype, Ts, Ds, max(abs(float(a) - b) / b for a, b in zip(out, mses)),
        float((got - grad.float()).abs().max()) / float(grad.float().pow(2).mean().sqrt())))
    np.testing.assert_allclose(out, mses, rtol=2e-5)
    assert not bool(torch.isnan(got).any())
    U.assert_close(got, grad, dtype, 'rec dlogits', scale=_scale(dtype))
    assert bool(torch.isnan(dl[..., Cc:].float()).all())        # the pad is never written


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cs', [3, 8])
def test_rec_loss_66_blocks_per_image(dtype, cs):
    """B = 5, 150 x 150 x 3, groups [0, 2, 3, 5]: bx = 66, so rec_loss_final_kernel's lo = gs[g] * bx is 0 / 132 / 198; four trips
    of the grid-stride loop, the last one ragged."""
    check_rec(5, 150, 150, 3, [0, 2, 3, 5], dtype, cs, cs)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cs', [3, 8])
def test_rec_loss_block_cap_single_group(dtype, cs):
    """B = 1, 300 x 300 x 3, G = 1: bx capped at 256, five trips of the grid-stride loop, one 64-thread final block."""
    check_rec(1, 300, 300, 3, [0, 1], dtype, cs, cs)


UNEVEN16 = [0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 19, 20]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,gstart', [(16, list(range(17))), (20, UNEVEN16)])
def test_rec_loss_sixteen_groups(B, gstart, dtype):
    """G = RD_MAX_GROUPS = 16 (the final kernel is a 1024-thread block), one image per group and uneven groups of 1 / 2 images."""
    assert len(gstart) == 17 and gstart[-1] == B
    check_rec(B, 23, 29, 3, gstart, dtype, 3, 8)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Cc,Ts,Ds', [(1, 1, 1), (2, 4, 2), (4, 4, 8), (7, 8, 8)])
def test_rec_loss_other_channel_counts(Cc, Ts, Ds, dtype):
    """C in {1, 2, 4, 7} through the float-reciprocal split (C = 7's reciprocal is inexact), Ts != Ds for two of them, and strides
    passed as 0 (= dense) where they equal C."""
    check_rec(3, 37, 41, Cc, [0, 1, 3], dtype, Ts, Ds, explicit_strides=False)


@functools.lru_cache(maxsize=1)
def _planted_indices():
    """A few hundred element indices of a 2048 x 2100 x 3 image, all above 12,582,912: indices whose uncorrected split is one too
    high (spread over the whole range, with the first and the last), their right neighbours, and the image's last element."""
    per = 2048 * 2100 * 3
    i = np.arange(per, dtype=np.int32)
    wrong = np.flatnonzero(M.raw_split(i, 3) != i // 3)
    assert wrong[0] == M.FIRST_WRONG_C3 and wrong.size > 1000
    pick = wrong[np.linspace(0, wrong.size - 1, 160).astype(np.int64)]
    idx = np.unique(np.concatenate([pick, pick[::2] + 1, [M.FIRST_WRONG_C3 - 1, per - 1]]))
    assert idx.min() > 12582912 and idx.max() == per - 1 and 200 < idx.size < 400
    assert len(set((idx % 3).tolist())) == 3                    # every channel occurs
    return idx, int(np.isin(idx, wrong).sum())


@pytest.mark.parametrize('dtype,cs', [('f32', 3), ('bf16', 3), ('f32', 8)])
def test_rec_loss_split_correction_above_12_58M_elements(dtype, cs):
    """B = 1, 2048 x 2100 x 3 = 12,902,400 elements: the only size range in which the `pix -= ...` correction of the float-reciprocal
    split fires (tests/test_cpu_loss_index.py).  Logits and target are zero except on the planted set, so tanh = 0 and dlogits = 0
    EXACTLY off it (1 - 2 * rcp(exp(0) + 1) = 0) and non-zero on it: an index that lands one pixel off is a misplaced non-zero,
    whatever the tolerance.  With dense strides pix * C + c == i even for an uncorrected split, so the padded case (target pad 7.0,
    dlogits pad NaN) is the one that sees a missing correction: it would read the pad and write into it."""
    H, W, Cc = 2048, 2100, 3
    idx, n_wrong = _planted_indices()
    assert n_wrong >= 160
    gen = _gen('planted')
    vals = (0.5 + torch.rand(idx.size, generator=gen)) * (1 - 2 * (torch.arange(idx.size) % 2))     # |x| in [0.5, 1.5), both signs
    lg = torch.zeros(H * W * Cc)
    lg[torch.from_numpy(idx.astype(np.int64))] = vals
    lg = U.rnd(lg, dtype).view(1, H, W, Cc)
    tgt = torch.zeros(1, H, W, Cc)
    mses, grad = rec_reference(lg, tgt, [0, 1], 0.1)
    out, dl = rec_call(lg, tgt, [0, 1], dtype, cs, cs)
    got = dl[..., :Cc].float().cpu().contiguous().view(-1)
    assert not bool(torch.isnan(got).any())                     # every element written
    nz = np.flatnonzero(got.numpy())
    assert np.array_equal(nz, idx), 'non-zero dlogits off the planted set, or zeros on it'
    np.testing.assert_allclose(out, mses, rtol=2e-5)
    # the tolerance is relative to the reference's RMS: taken over the planted elements (everything else is exactly zero, above)
    sel = torch.from_numpy(idx.astype(np.int64))
    U.assert_close(got[sel], grad.view(-1)[sel], dtype, 'rec dlogits 12.9M', scale=_scale(dtype))
    assert bool(torch.isnan(dl[..., Cc:].float()).all())


def _rec_refusal(B, H, W, Cc, Ts, Ds, G, gstart):
    lgd, td = torch.zeros(64, device=U.dev()), torch.zeros(64, device=U.dev())
    dl, out, ws = Guarded(256, torch.float32), Guarded(64, torch.float32), Guarded(256, torch.float32)
    rc = L.lib().rd_rec_loss(L.ptr(lgd), L.ptr(td), dl.ptr(), out.ptr(), ws.ptr(), B, H, W, Cc, Ts, Ds, G, L.gstart_array(gstart), 0.1,
                             L.RD_F32, None)
    torch.cuda.synchronize()
    assert rc == -1
    assert dl.intact() and out.intact() and ws.intact()
    assert bool(torch.isnan(dl.t).all()) and bool(torch.isnan(out.t).all()) and bool(torch.isnan(ws.t).all())


def test_rec_loss_refuses_images_of_2_to_24_elements():
    """2048 x 2731 x 3 = 16,779,264 >= 2^24: -1 before anything is read or written (the buffers passed hold 64 elements)."""
    _rec_refusal(1, 2048, 2731, 3, 3, 3, 1, [0, 1])


@pytest.mark.parametrize('G,Ts,Ds', [(0, 3, 3), (17, 3, 3), (1, 2, 3), (1, 3, 2)])
def test_rec_loss_argument_checks(G, Ts, Ds):
    """G = 0, G = 17 (> RD_MAX_GROUPS), a target or dlogits stride below C: -1, outputs untouched."""
    _rec_refusal(1, 4, 4, 3, Ts, Ds, G, [0, 1])


# ------------------------------------------------------------------------------------ Adam
ADAM_N = 1048576 + 256 + 37
ADAM_HALF = 524301
B1, B2, ADAM_EPS, BASE_LR = 0.9, 0.999, 1e-8, 2e-3


class AdamState:
    def __init__(self, p0, n_half, total_iters):
        n = p0.numel()
        self.p, self.m, self.v = p0.clone().to(U.dev()), torch.zeros(n, device=U.dev()), torch.zeros(n, device=U.dev())
        self.it = torch.zeros((), dtype=torch.int32, device=U.dev())
        self.hyper = torch.full((4,), float('nan'), device=U.dev())
        a = self.a = L.RdAdam()
        a.param, a.exp_avg, a.exp_avg_sq, a.n, a.n_half_lr = self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, n_half
        a.iter, a.hyper_out, a.base_lr, a.total_iters = self.it.data_ptr(), self.hyper.data_ptr(), BASE_LR, total_iters
        a.beta1, a.beta2, a.eps = B1, B2, ADAM_EPS

    def step(self, g):
        gd = g.to(U.dev())
        self.a.grad = gd.data_ptr()
        self.hyper.fill_(float('nan'))
        rc = L.lib().rd_adam_step(C.byref(self.a), None)
        torch.cuda.synchronize()
        return rc


def _f32(x):
    return float(np.float32(x))


def check_hyper(hyper, it, total_iters):
    """hyper_out of the call that ran iteration `it`: float64 expressions of adam_prepare_kernel rounded to float32, within one ulp
    (the device's double pow against Python's); the iteration number exactly."""
    lr = _f32(BASE_LR) * (1.0 if it == 0 else (1.0 - (it - 1) / total_iters) ** 0.9)
    want = [lr, 1.0 - _f32(B1) ** (it + 1), 1.0 - _f32(B2) ** (it + 1)]
    for k in range(3):
        w = np.float32(want[k])
        assert abs(float(hyper[k]) - float(w)) <= float(np.spacing(w)), (k, it, float(hyper[k]), float(w))
    assert float(hyper[3]) == float(it)


def adam_reference(p0, m0, v0, g, hyper, n_half):
    """One step in float64 from the device's own pre-step state and hyper_out, with the bound each output is held to.

    Roundings of adam_update_kernel (e = 2^-24, every operation correctly rounded; -ffp-contract=on may fuse one product of each sum
    into an fma, which only removes roundings):
      m = b1 * m0 + (1 - b1) * g          A = b1 m0 and Bt = (1 - b1) g round once each (1 - b1 is exact), the sum once:
                                          |dm| <= e (|A| + |Bt| + |m|).  Where A and Bt have one sign (always in the first step) this is
                                          2 e |m|; where they cancel, the two product roundings do not shrink with |m|.
      v = b2 * v0 + (1 - b2) * g * g      A2 = b2 v0 once, B2 = ((1 - b2) g) g twice, the sum once, all terms >= 0:
                                          |dv| <= e (2 A2 + 3 B2) <= 3 e v.
      u = (hlr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),  p = p0 - u
                                          sqrt(v): 1.5 e inherited + 1; sqrtf(bc2) 1; the quotient 1; + eps 1 (eps > 0): 5.5 e on the
                                          denominator; hlr / bc1 1 (0.5 * lr is exact); m / denom 1; the product 1: 8.5 e, held as 9 e |u|,
                                          plus m's own error carried through: (s / d) |dm|; then one rounding into param: e |p|.
    Each bound carries (1 + 1e-6) for the second-order terms and a few float32 denormal steps (1.4e-45) absolutely."""
    p0, m0, v0, g = (t.double().numpy() for t in (p0, m0, v0, g))
    lr, bc1, bc2 = (float(hyper[k]) for k in range(3))
    b1, b2, eps = _f32(B1), _f32(B2), _f32(ADAM_EPS)
    A, Bt = b1 * m0, (1.0 - b1) * g
    m = A + Bt
    A2, B2t = b2 * v0, (1.0 - b2) * g * g
    v = A2 + B2t
    s = np.where(np.arange(p0.size) < n_half, 0.5 * lr, lr) / bc1
    d = np.sqrt(v) / math.sqrt(bc2) + eps
    u = s * (m / d)
    p = p0 - u
    slack = 1.0 + 1e-6
    m_abs = EPS24 * (np.abs(A) + np.abs(Bt) + np.abs(m))
    m_tol = m_abs * slack + 3e-45
    v_tol = EPS24 * (2 * A2 + 3 * B2t) * slack + 5e-45
    p_tol = (EPS24 * np.abs(p) + 9 * EPS24 * np.abs(u) + (s / d) * m_abs) * slack + 1e-45
    return (p, m, v, u), (p_tol, m_tol, v_tol)


def _adam_grad(n, gen, planted):
    g = torch.randn(n, generator=gen)
    for pos, val in planted:
        g[pos] = val
    return g


@pytest.mark.parametrize('n_half', [ADAM_HALF, 0, ADAM_N])
def test_adam_past_the_block_cap_within_derived_float32_bounds(n_half):
    """n = 1,048,869 (4098 -> 4096 blocks, a ragged second trip for the last 293 elements), three steps, the half-LR boundary off
    every block boundary / at 0 / at n.  Per step: float64 reference from the state read back before the step (adam_reference).
    Measured on an MI355X: worst error / bound 0.997 (param), 0.94 (exp_avg), 0.92 (exp_avg_sq).  The plain per-element forms
    e |p| + 8 e |u|, 2 e |m| and 2 e |v| are printed for comparison; a correct float32 kernel does not meet them once the two
    terms of exp_avg cancel (steps 2 and 3: about 63,000 elements beyond 2 e |m|, 1,200 beyond 2 e |v|, 3 beyond the param form;
    an unfused numpy float32 restatement of the kernel gives the same counts), which is what adam_reference's bounds account for."""
    n, total = ADAM_N, 40
    gen = _gen('adam', n_half)
    # planted gradients, the same positions every step; each set reaches into the second trip (i >= 1,048,576) and both LR halves
    body = torch.randperm(n - 150, generator=gen)[:810]
    zero = torch.cat([body[:270], torch.arange(n - 30, n)])
    tiny = torch.cat([body[270:540], torch.arange(n - 90, n - 60)])
    huge = torch.cat([body[540:], torch.arange(n - 150, n - 120)])
    for s in (zero, tiny, huge):
        assert int((s < n_half).sum()) in ((0,) if n_half == 0 else (300,) if n_half == n else range(50, 251))
    planted = ((zero, 0.0), (tiny, 1e-20), (huge, 1e4))
    p0 = torch.randn(n, generator=gen)
    st = AdamState(p0, n_half, total)
    for step in range(3):
        g = _adam_grad(n, gen, planted)
        pre = [t.cpu() for t in (st.p, st.m, st.v)]
        L.check(st.step(g), 'adam')
        assert int(st.it) == step + 1
        hyper = st.hyper.cpu().numpy()
        check_hyper(hyper, step, total)
        (p, m, v, u), (p_tol, m_tol, v_tol) = adam_reference(pre[0], pre[1], pre[2], g, hyper, n_half)
        got = [t.cpu().double().numpy() for t in (st.p, st.m, st.v)]
        assert all(np.isfinite(x).all() for x in got)
        errs = [np.abs(got[0] - p), np.abs(got[1] - m), np.abs(got[2] - v)]
        issue = [EPS24 * np.abs(p) + 8 * EPS24 * np.abs(u) + 1e-45, 2 * EPS24 * np.abs(m), 2 * EPS24 * v]   # the plain per-element forms
        print('adam n_half=%d step %d: max err/bound param %.3f exp_avg %.3f exp_avg_sq %.3f; elements beyond e|p|+8e|u| / 2e|m| / 2e|v|: %d %d %d' % (
            n_half, step, *(float((e / t).max()) for e, t in zip(errs, (p_tol, m_tol, v_tol))),
            *(int((e > b).sum()) for e, b in zip(errs, issue))))
        for name, e, t in zip(('param', 'exp_avg', 'exp_avg_sq'), errs, (p_tol, m_tol, v_tol)):
            bad = np.flatnonzero(e > t)
            assert bad.size == 0, '%s step %d: %d elements beyond the bound, first %d: err %.3e bound %.3e' % (
                name, step, bad.size, bad[0], e[bad[0]], t[bad[0]])
        # zero gradient on zero moments: the parameter does not move (0 / (0 + eps) = 0), bit for bit
        z = zero.numpy()
        assert np.array_equal(got[0][z], p0.double().numpy()[z]) and not got[1][z].any() and not got[2][z].any()
        assert (got[2][tiny.numpy()] > 0).all()                 # (1 - b2) * 1e-40 is a float32 denormal, not flushed
    # the grid-stride loop's second trip moved the tail (but for the 30 zero and the 30 tiny gradients planted in it)
    assert int((st.p.cpu()[n - 293:] != p0[n - 293:]).sum()) >= 293 - 60


def test_adam_poly_lr_schedule_over_every_iteration():
    """n = 1000, total_iters = 7: hyper_out of all seven iterations (LR of iteration it was written from it - 1; the last one is
    base_lr * (1 - 5/7)^0.9), bias corrections 1 - beta^(it + 1), and the device-side counter."""
    n, total = 1000, 7
    gen = _gen('adam schedule')
    st = AdamState(torch.randn(n, generator=gen), 300, total)
    for it in range(total):
        L.check(st.step(torch.randn(n, generator=gen)), 'adam')
        check_hyper(st.hyper.cpu().numpy(), it, total)
        assert int(st.it) == it + 1
    assert bool(torch.isfinite(st.p).all())


def test_adam_honours_an_iteration_counter_written_from_the_host():
    """The counter lives on the device; a resumed run sets it from the host.  After one step, *iter = 5: the next call runs
    iteration 5 (its LR, its bias corrections, hyper_out[3] = 5) and leaves 6."""
    n, total = 1000, 7
    gen = _gen('adam resume')
    st = AdamState(torch.randn(n, generator=gen), 300, total)
    L.check(st.step(torch.randn(n, generator=gen)), 'adam')
    assert int(st.it) == 1
    st.it.fill_(5)
    g = torch.randn(n, generator=gen)
    pre = [t.cpu() for t in (st.p, st.m, st.v)]
    L.check(st.step(g), 'adam')
    hyper = st.hyper.cpu().numpy()
    check_hyper(hyper, 5, total)
    assert int(st.it) == 6
    (p, _, _, _), (p_tol, _, _) = adam_reference(pre[0], pre[1], pre[2], g, hyper, 300)
    assert (np.abs(st.p.cpu().double().numpy() - p) <= p_tol).all()


def test_adam_refuses_an_empty_bank():
    st = AdamState(torch.randn(8), 0, 7)
    st.a.n = 0
    before = _bits(st.p)
    assert st.step(torch.randn(8)) == -1
    assert torch.equal(_bits(st.p), before) and int(st.it) == 0 and bool(torch.isnan(st.hyper).all())
