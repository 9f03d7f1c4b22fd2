"""-m gpu: train.py --gpu_val_volumes -- the validation kernels (rd_vol_stack, rd_vol_argmax, rd_vol_post; csrc/val_volume.hip)
against the numpy model and scipy bit for bit, the whole validation pass against train.py::test_prostate on the same modules, and the
CLI end to end (the same model, the same keep-best files and the same CSV numbers with and without the flag)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_val_volumes_cases as VC
import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_SHARE = 1e-4            # voxels whose two fp32 softmax probabilities are equal although the logits differ: at most this share


def _reference(m):
    from utils.metrics import connectivity_region_analysis
    return connectivity_region_analysis(np.asarray(m, dtype=np.float64)).astype(np.uint8)


def _run_post(cases, with_gt=True):
    """Every volume of `cases` in ONE rd_vol_post call; returns (post volumes, counts (n, 3) or None, ground truths, slots)."""
    from ramdsir import gpu_val_volumes as V
    vols = [m for _, m in cases]
    n = len(vols)
    recs, nbytes = V.volume_records([m.shape for m in vols], slots=[n - 1 - i for i in range(n)])  # slots need not follow the call's order
    buf = np.concatenate([m.reshape(-1) for m in vols]).astype(np.uint8)
    assert buf.size == nbytes
    rng = np.random.RandomState(5)
    gts = [(rng.uniform(size=m.shape) < 0.4).astype(np.uint8) * rng.randint(1, 256, m.shape).astype(np.uint8) for m in vols]
    dev = torch.device('cuda:0')
    pred = torch.from_numpy(buf).to(dev)
    out = torch.full_like(pred, 7)
    gt = torch.from_numpy(np.concatenate([g.reshape(-1) for g in gts])).to(dev) if with_gt else None
    counts = torch.zeros((n, 3), dtype=torch.int32, device=dev) if with_gt else None
    poison = torch.full((64 << 20,), 0x5A, dtype=torch.uint8, device=dev)         # what the workspace may be carved from
    del poison
    V.post(pred, out, recs, n, gt, counts)
    torch.cuda.synchronize()
    assert torch.equal(pred.cpu(), torch.from_numpy(buf))                          # the input is not modified
    o = out.cpu().numpy()
    posts = [o[r.off:r.off + r.d * r.h * r.w].reshape(r.d, r.h, r.w) for r in list(recs)[:n]]
    return posts, None if counts is None else counts.cpu().numpy(), gts


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_post_kernels_equal_scipy_bit_for_bit_and_count_exactly(order):
    """Ragged (d, h, w), 384 x 384 slices, the empty volume and ties, all in ONE call that crosses a launch chunk, against
    utils.metrics.connectivity_region_analysis and numpy's counts; the Dice doubles against metrics.dc.  The reversed order runs the
    same volumes through other parts of the (uninitialised) workspace."""
    from ramdsir import _lib as L, gpu_val_volumes as V
    from utils.metrics import dc
    cases = VC.named_volumes() + VC.big_volumes()
    if order == 'reversed':
        cases = cases[::-1]
    n = len(cases)
    assert n > L.VAL_CHUNK
    assert any(m.shape[1:] == (384, 384) for _, m in cases) and any(not m.any() for _, m in cases) and any(VC.has_tie(m) for _, m in cases)
    posts, c, gts = _run_post(cases)
    for i, (name, m) in enumerate(cases):
        ref = _reference(m)
        assert np.array_equal(posts[i], ref), name
        g = gts[i] != 0
        want = [int(ref.sum()), int(g.sum()), int((ref.astype(bool) & g).sum())]
        assert c[n - 1 - i].tolist() == want, name
        assert V.dice_from_counts(*c[n - 1 - i].tolist()) == dc(ref.astype(bool), g), name
    # without targets: the same volumes, no counts
    posts2, _, _ = _run_post(cases, with_gt=False)
    assert all(np.array_equal(a, b) for a, b in zip(posts, posts2))


def test_post_on_many_small_random_volumes_in_one_call():
    """Small volumes are where ties are common: 400 of them, 13 launch chunks, one call."""
    rng = np.random.RandomState(12)
    cases = []
    for k in range(400):
        d, h, w = rng.randint(1, 9, 3)
        cases.append((str(k), (rng.uniform(size=(d, h, w)) < (0.2, 0.4, 0.6)[k % 3]).astype(np.uint8)))
    assert sum(VC.has_tie(m) for _, m in cases) >= 25
    posts, c, gts = _run_post(cases)
    for i, (name, m) in enumerate(cases):
        ref = _reference(m)
        assert np.array_equal(posts[i], ref), m
        assert c[len(cases) - 1 - i].tolist() == [int(ref.sum()), int((gts[i] != 0).sum()), int((ref.astype(bool) & (gts[i] != 0)).sum())]


def test_post_rejects_bad_records_and_launches_nothing():
    from ramdsir import _lib as L, gpu_val_volumes as V
    dev = torch.device('cuda:0')
    lib = L.lib()
    st = V._stream()

    def call(recs, n, pred, out, pred_bytes, gt, gt_bytes, counts, slots, ws, ws_bytes):
        return lib.rd_vol_post(L.ptr(pred), L.ptr(out), pred_bytes, L.ptr(gt), gt_bytes, L.ptr(counts), slots, L.ptr(ws), ws_bytes, recs, n, st)
    recs, nbytes = V.volume_records([(2, 4, 4), (3, 2, 5)])
    pred = torch.ones(nbytes, dtype=torch.uint8, device=dev)
    out = torch.full((nbytes,), 9, dtype=torch.uint8, device=dev)
    gt = torch.ones(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    ws_bytes = lib.rd_vol_post_workspace(recs, 2)
    assert ws_bytes == 16 + 2 * ((nbytes * 4 + 15) // 16 * 16)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    good = (recs, 2, pred, out, nbytes, gt, nbytes, counts, 2, ws, ws_bytes)

    def bad(**kw):
        a = dict(zip(('recs', 'n', 'pred', 'out', 'pred_bytes', 'gt', 'gt_bytes', 'counts', 'slots', 'ws', 'ws_bytes'), good))
        a.update(kw)
        return call(*[a[k] for k in ('recs', 'n', 'pred', 'out', 'pred_bytes', 'gt', 'gt_bytes', 'counts', 'slots', 'ws', 'ws_bytes')])
    assert bad(pred_bytes=nbytes - 1) == -1                                        # the second volume ends behind the buffer
    assert bad(gt_bytes=nbytes - 1) == -1
    assert bad(ws_bytes=ws_bytes - 1) == -1
    assert bad(slots=1) == -1                                                     # the second record's slot
    assert bad(counts=None) == -1                                                 # gt without counts
    assert bad(out=pred) == -1                                                    # in place
    for field, value in (('d', 0), ('h', 0), ('w', -1), ('off', -1), ('gt_off', -1), ('slot', -1), ('d', 1 << 30)):
        r2, _ = V.volume_records([(2, 4, 4), (3, 2, 5)])
        setattr(r2[1], field, value)
        assert bad(recs=r2) == -1, field
        if field in ('d', 'h', 'w', 'off'):
            assert lib.rd_vol_post_workspace(r2, 2) == -1, field
    torch.cuda.synchronize()
    assert int((out != 9).sum()) == 0 and int(counts.abs().sum()) == 0 and int(ws.sum()) == 0    # nothing was launched
    with pytest.raises(RuntimeError):
        V.post(pred, out[:nbytes - 1], recs, 2)
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [[32, 32, 32], [30, 30, 30]] and int(out.sum()) == nbytes
    # the frame lists of the other two entry points
    vol = torch.zeros((6, 4, 4), dtype=torch.float32, device=dev)
    x = torch.full((2, 3, 4, 4), 9.0, dtype=torch.float32, device=dev)
    p = torch.full((6 * 16,), 9, dtype=torch.uint8, device=dev)
    e = torch.zeros(6, dtype=torch.uint8, device=dev)
    for frames in ([0, 1], [1, 5], [2, 2], [3, 2], [-2, 1], [4, 6]):
        f = (L.i32 * 2)(*frames)
        assert lib.rd_vol_stack(L.ptr(vol), 6, 4, 4, f, 2, L.ptr(x), st) == -1, frames
        assert lib.rd_vol_argmax(L.ptr(x), 2, 4, 4, f, L.ptr(e), 6, L.ptr(p), st) == -1, frames
    torch.cuda.synchronize()
    assert int((x != 9).sum()) == 0 and int((p != 9).sum()) == 0


@pytest.mark.parametrize('shape,bs', [((10, 64, 64), 4), ((13, 48, 80), 4), ((5, 7, 9), 4), ((3, 5, 5), 4), ((40, 16, 16), 36), ((9, 384, 384), 8)])
def test_stack_kernel_equals_the_model_bit_for_bit(shape, bs):
    """Every batch of a volume, including short and empty ones, H * W not a multiple of four (the scalar kernel), more slots than a launch
    chunk, and a volume at an address that is not 16-byte aligned."""
    from ramdsir import gpu_val_volumes as V
    rng = np.random.RandomState(sum(shape))
    vol = rng.normal(0, 1, shape).astype(np.float32)
    vol[0, 0, 0] = np.nan
    dev = torch.device('cuda:0')
    D = shape[0]
    hold = torch.empty(vol.size + 1, dtype=torch.float32, device=dev)
    for shift in (0, 1):
        v = hold[shift:shift + vol.size].view(shape)
        v.copy_(torch.from_numpy(vol))
        batches = V.frame_batches(D, bs) + [[-1] * bs, [D - 2] + [-1] * (bs - 1)] if D > 2 else [[-1] * bs]
        assert batches
        for frames in batches:
            got = V.stack(v, frames).cpu().numpy()
            assert got.shape == (bs, 3) + shape[1:]
            assert np.array_equal(got.view(np.uint32), V.stack_model(vol, frames).view(np.uint32)), (frames, shift)


def _cone_logits(rng, B, H, W):
    """Two-class logits with structure: a few cones on class 1 against a flat class 0, plus noise; some exact ties."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    lg = rng.normal(0, 1.5, (B, 2, H, W)).astype(np.float32)
    for b in range(B):
        cy, cx, r = rng.uniform(0.2 * H, 0.8 * H), rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.1, 0.3) * min(H, W)
        lg[b, 1] += 8.0 * np.clip(1.0 - np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / r, 0, None) - 3.0
    tie = rng.uniform(size=(B, H, W)) < 0.01
    lg[:, 1][tie] = lg[:, 0][tie]
    return lg


@pytest.mark.parametrize('shape,bs', [((10, 384, 384), 4), ((13, 48, 80), 4), ((7, 7, 9), 3), ((40, 16, 16), 36)])
def test_argmax_kernel_equals_the_model_and_torch(shape, bs):
    """rd_vol_argmax against argmax_model on the same logits bit for bit, with no band; against torch's softmax + max on the device
    wherever torch's two probabilities differ (softmax is monotone: the rules can only disagree where fp32 softmax collapses different
    logits to equal probabilities; such voxels are counted, printed and capped)."""
    from ramdsir import gpu_val_volumes as V
    D, H, W = shape
    rng = np.random.RandomState(D + H + W)
    dev = torch.device('cuda:0')
    gt_empty = (rng.uniform(size=D) < 0.3).astype(np.uint8)
    gt_empty[1] = 1
    e = torch.from_numpy(gt_empty).to(dev)
    hold = torch.full((D * H * W + 4,), 0, dtype=torch.uint8, device=dev)
    n_cmp = n_tie = 0
    for shift in (0, 1):
        pred = hold[shift:shift + D * H * W]
        V.zero(hold)
        want = np.zeros(shape, np.uint8)
        batches = V.frame_batches(D, bs)
        assert batches
        for frames in batches:
            lg = _cone_logits(rng, bs, H, W)
            t = torch.from_numpy(lg).to(dev)
            V.argmax(t, frames, e, pred, shape)
            V.argmax_model(lg, frames, gt_empty, want)
            sm = torch.softmax(t, dim=1)
            ref = torch.max(sm, dim=1)[1]
            differ = (sm[:, 0] != sm[:, 1]).cpu().numpy()
            got = pred.cpu().numpy().reshape(shape)
            for b, jj in enumerate(frames):
                if jj < 0 or gt_empty[jj]:
                    continue
                assert np.array_equal(got[jj][differ[b]], ref[b].cpu().numpy().astype(np.uint8)[differ[b]]), (jj, shift)
                n_cmp += differ[b].size
                n_tie += int((~differ[b] & (lg[b, 0] != lg[b, 1])).sum())
        got = pred.cpu().numpy().reshape(shape)
        assert np.array_equal(got, want), shift
        assert 0.005 < got.mean() < 0.5
        assert not got[gt_empty.astype(bool)].any() and not got[0].any() and not got[D - 1].any()
        assert int(hold[D * H * W + shift:].sum()) == 0 and (shift == 0 or int(hold[0]) == 0)    # nothing written around the volume
    print('argmax %s: %d voxels compared with torch, %d left out (equal fp32 probabilities, different logits)' % (shape, n_cmp, n_tie))
    assert n_cmp > 0 and n_tie <= TIE_SHARE * n_cmp


def _states(sharpen):
    """tests/test_gpu_gpu_val.py's fixed checkpoint: a random-init network with a scaled output conv (structured masks)."""
    from oracle import unet as OU
    enc, dec = OU.encoder_state(seed=11), OU.decoder_state(num_classes=2, seed=12)
    dec['out1.weight'] = dec['out1.weight'] * sharpen
    return enc, dec


def _csv_layout(line):
    return re.sub(r'[-+]?\d+\.\d+(e[-+]?\d+)?', '<f>', line)


def _csv_values(text):
    return [[float(v) for v in re.findall(r'[-+]?\d+\.\d+(?:e[-+]?\d+)?', l)] for l in text.strip().splitlines()]


def _write_volumes(dom, specs, seed=3):
    """NIfTI volumes of one site: a bright block with noise; (name, D, dtype, empty ground-truth slices)."""
    from utils import nifti
    os.makedirs(dom)
    rng = np.random.RandomState(seed)
    for name, D, dtype, empty in specs:
        img = rng.uniform(0, 60, (D, 64, 64))
        msk = np.zeros((D, 64, 64), np.uint8)
        img[1:D - 1, 20:44, 16:40] += 150
        msk[1:D - 1, 20:44, 16:40] = 1
        msk[2:D - 2, 28:36, 24:32] = 2
        for z in empty:
            msk[z] = 0
        nifti.write_volume(os.path.join(dom, name + '.nii.gz'), img.astype(dtype))
        nifti.write_volume(os.path.join(dom, name + '_segmentation.nii.gz'), msk)


def test_whole_pass_equals_test_prostate(tmp_path):
    """test_prostate_gpu and test_prostate on the same modules: ragged D (10, 13, 5 with batches of 4; 3: no batch at all), one int16
    volume, slices with an empty ground truth.  Wherever a volume has no tie voxel the prediction volumes are identical and the Dice
    are the same doubles; the CSV lines have one layout and equal numbers; validation leaves parameters, buffers and random states
    as they were."""
    base = str(tmp_path / 'data' / 'prostate')
    _write_volumes(os.path.join(base, 'BIDMC'), [('Case00', 10, np.float32, (3,)), ('Case01', 13, np.int16, (1, 6, 7)),
                                                 ('Case02', 5, np.float64, ()), ('Case03', 3, np.float32, ())])
    enc, dec = _states(sharpen=10.0)
    ck = str(tmp_path / 'ck.pth')
    torch.save({'encoder_state_dict': enc, 'seg_decoder_state_dict': dec}, ck)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'gpu_val_volumes_driver.py'), base, '4', ck, str(tmp_path / 'out'), '4']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    log = r.stdout.decode()
    assert r.returncode == 0, log[-3000:]
    res = json.loads([l for l in log.splitlines() if l.startswith('RESULT ')][-1][7:])
    print({k: res[k] for k in ('files', 'shapes', 'dtypes', 'ties', 'foreground', 'empty_gt', 'dice_host', 'dice_gpu', 'ret_host', 'ret_gpu')})
    assert sorted(s[0] for s in res['shapes']) == [3, 5, 10, 13] and 'int16' in res['dtypes']
    assert sum(res['empty_gt']) >= 4
    assert any(0.0 < f < 1.0 for f in res['foreground'])                          # the predictions are not all empty
    assert res['untouched']
    assert all(res['same_pred'])                                                  # the kernels' argmax on the pass's own logits
    for i, n_tie in enumerate(res['ties']):
        if n_tie == 0:
            assert res['same_post'][i], i
            assert res['dice_gpu'][i] == res['dice_host'][i], i
    if not any(res['ties']):
        assert res['ret_gpu'] == res['ret_host']
        host_csv, gpu_csv = res['csv']
        assert len(gpu_csv.strip().splitlines()) == 1 and _csv_layout(gpu_csv) == _csv_layout(host_csv)
        assert _csv_values(gpu_csv) == _csv_values(host_csv)
    total = sum(s[0] * s[1] * s[2] for s in res['shapes'])
    assert sum(res['ties']) <= TIE_SHARE * total, res['ties']
    assert _csv_layout(res['csv'][1]) == _csv_layout(res['csv'][0])


def _train(data, out, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', 'prostate', '--domain_idxs',
           '1,2,3,4,5', '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', out, '--epochs', '2', '--max_iters', '4', '--num_workers', '0', '--log_every', '2', '--deterministic',
           '--test_batch_size', '4']
    return subprocess.run(cmd + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


def test_train_cli_gpu_val_volumes_gives_the_same_model_and_numbers(tmp_path):
    """Two epochs (two validations) without the flag, with it, and with it beside --gpu_data: final_model.pth bit for bit (validation
    disturbs neither the training state nor a random generator), the same keep-best files, the same CSV numbers; the preload line
    only with the flag."""
    data = str(tmp_path / 'data')
    SD.make_prostate_tree(data, n=4, S=64)
    _write_volumes(os.path.join(data, 'prostate', 'ISBI'), [('Case00', 10, np.float32, (3,)), ('Case01', 13, np.int16, (1, 6)),
                                                            ('Case02', 5, np.float32, ())])
    runs = []
    for name, extra in (('host', []), ('vol', ['--gpu_val_volumes']), ('both', ['--gpu_val_volumes', '--gpu_data'])):
        out = str(tmp_path / name)
        r = _train(data, out, extra)
        log = r.stdout.decode()
        assert r.returncode == 0, log[-3000:]
        assert ('gpu_val_volumes: 3 volumes' in log) == ('--gpu_val_volumes' in extra)
        assert log.count('val_dice') == 2
        runs.append((torch.load(os.path.join(out, 'final_model.pth'), map_location='cpu'),
                     sorted(f for f in os.listdir(out) if f.startswith('model_')), open(os.path.join(out, '0_val_log.csv')).read()))
    ck0, best0, csv0 = runs[0]
    assert len(_csv_values(csv0)) == 2
    for ck, best, csv in runs[1:]:
        for part in ck0:
            assert list(ck0[part]) == list(ck[part])
            for k in ck0[part]:
                assert torch.equal(ck0[part][k], ck[part][k]), (part, k)
        assert best == best0
        assert _csv_layout(csv) == _csv_layout(csv0)
        assert _csv_values(csv) == _csv_values(csv0)
