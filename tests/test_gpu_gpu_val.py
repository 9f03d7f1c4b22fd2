"""-m gpu: train.py --gpu_val -- the validation kernels (rd_val_threshold, rd_val_post; csrc/val_post.hip) against scipy bit for
bit and against F.interpolate under the band rule, the whole validation pass against train.py::test_fundus on the same modules,
and the CLI end to end (the same model, the same keep-best files and the same CSV numbers with and without the flag)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import gpu_val_cases as GC
import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICE_TOL = 2e-3             # tests/test_gpu_eval_parity.py: a handful of border pixels may cross the threshold


def _pack(stacks):
    from ramdsir import gpu_val as G
    recs, nbytes = G.image_records([m.shape[1:] for m in stacks])
    buf = np.concatenate([m.reshape(-1) for m in stacks]).astype(np.uint8)
    assert buf.size == nbytes
    return recs, nbytes, buf


def _unpack(buf, recs, n):
    return [buf[r.off:r.off + 2 * r.h * r.w].reshape(2, r.h, r.w) for r in list(recs)[:n]]


@pytest.mark.parametrize('order', ['forward', 'reversed'])
def test_post_kernels_equal_scipy_bit_for_bit_and_count_exactly(order):
    """Stages b and c: every plane of the fixed set in ONE call (mixed sizes, several launch chunks), against
    utils.metrics.postprocess_binary and numpy's counts; the Dice doubles against post_and_dice.  The reversed order runs the same
    planes through other parts of the (uninitialised, reused) workspace."""
    from ramdsir import _lib as L, gpu_val as G
    from utils.metrics import post_and_dice, postprocess_binary
    cases = GC.stacks()
    if order == 'reversed':
        cases = cases[::-1]
    stacks = [m for _, m in cases]
    n = len(stacks)
    assert n > 2 * L.VAL_CHUNK
    rng = np.random.RandomState(5)
    gts = [(rng.uniform(size=m.shape) < 0.4).astype(np.uint8) * rng.randint(1, 256, m.shape).astype(np.uint8) for m in stacks]
    recs, nbytes, buf = _pack(stacks)
    for i in range(n):
        recs[i].gt_off = recs[i].off
        recs[i].slot = n - 1 - i                                                   # slots need not follow the call's order
    dev = torch.device('cuda:0')
    mask = torch.from_numpy(buf).to(dev)
    gt = torch.from_numpy(np.concatenate([g.reshape(-1) for g in gts])).to(dev)
    counts = torch.zeros((n, 2, 3), dtype=torch.int32, device=dev)
    poison = torch.full((64 << 20,), 0x5A, dtype=torch.uint8, device=dev)         # what the workspace may be carved from
    del poison
    out = G.post(mask, recs, n, nbytes, gt, counts)
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu(), torch.from_numpy(buf))                          # the input is not modified
    posts = _unpack(out.cpu().numpy(), recs, n)
    c = counts.cpu().numpy()
    for i, (name, m) in enumerate(cases):
        ref = postprocess_binary(m)
        assert np.array_equal(posts[i], ref), name
        g = gts[i] != 0
        for s in range(2):
            want = [int(ref[s].sum()), int(g[s].sum()), int((ref[s].astype(bool) & g[s]).sum())]
            assert c[n - 1 - i, s].tolist() == want, (name, s)
        dice = tuple(G.dice_from_counts(*c[n - 1 - i, s].tolist()) for s in range(2))
        assert dice == post_and_dice((m, gts[i])), name
    # without targets: the same masks, no counts
    out2 = G.post(mask, recs, n, nbytes)
    assert torch.equal(out2, out)


def test_post_rejects_bad_records():
    from ramdsir import _lib as L, gpu_val as G
    recs, nbytes = G.image_records([(4, 4)])
    dev = torch.device('cuda:0')
    mask = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError):
        G.post(mask, recs, 1, nbytes - 1)                                         # the buffer is smaller than the record says
    recs[0].h = 0
    with pytest.raises(ValueError):
        G.post(mask, recs, 1, nbytes)


def test_threshold_kernel_against_interpolate_on_the_device():
    """Stage a, one call with three images of different native sizes, against torch on the same device: the band rule; and against
    the numpy model, which the kernel's arithmetic follows operation by operation."""
    from ramdsir import gpu_val as G
    logits = GC.cone_logits(seed=99, n=len(GC.SIZES))
    dev = torch.device('cuda:0')
    lg = torch.from_numpy(logits).to(dev)
    recs, nbytes = G.image_records(GC.SIZES)
    mask = G.threshold(lg, recs, len(GC.SIZES), nbytes)
    got = _unpack(mask.cpu().numpy(), recs, len(GC.SIZES))
    for i, (H, W) in enumerate(GC.SIZES):
        ref = (F.interpolate(torch.sigmoid(lg[i:i + 1]), size=(H, W), mode='bilinear') > 0.75)[0].to(torch.uint8).cpu().numpy()
        assert 0.01 < ref.mean() < 0.3
        GC.assert_band_rule(got[i], ref, logits[i], H, W, 'kernel against torch on the device')
        GC.assert_band_rule(got[i], G.resize_threshold_model(logits[i], H, W), logits[i], H, W, 'kernel against the numpy model')


def _states(sharpen):
    """tests/test_gpu_eval_parity.py's fixed checkpoint: a random-init network with a scaled output conv (structured masks)."""
    from oracle import unet as OU
    enc, dec = OU.encoder_state(seed=11), OU.decoder_state(num_classes=2, seed=12)
    dec['out1.weight'] = dec['out1.weight'] * sharpen
    return enc, dec


def _csv_layout(line):
    return re.sub(r'[-+]?\d+\.\d+(e[-+]?\d+)?', '<f>', line)


def _csv_values(text):
    return [[float(v) for v in re.findall(r'[-+]?\d+\.\d+(?:e[-+]?\d+)?', l)] for l in text.strip().splitlines()]


def test_whole_pass_equals_test_fundus(tmp_path):
    """test_fundus_gpu and test_fundus on the same modules, a tree whose test images all differ in size (non-square) plus one
    800 x 800 image: wherever the two thresholded masks agree the per-image Dice are the same doubles; the CSV lines have one layout;
    validation leaves parameters, buffers and random states as they were."""
    data = str(tmp_path / 'data')
    base = SD.make_fundus_tree(data, n_train=1, n_test=6, hw=(136, 152), vary=True)
    rng = np.random.RandomState(3)
    ri = os.path.join(base, 'Domain1', 'test', 'ROIs', 'image', 'd1_test_02.png')
    Image.fromarray(SD._smooth_rgb(rng, 800, 800)).save(ri)
    Image.fromarray(SD._disc_mask(rng, 800, 800)).save(ri.replace('/image/', '/mask/'))
    enc, dec = _states(sharpen=10.0)
    ck = str(tmp_path / 'ck.pth')
    torch.save({'encoder_state_dict': enc, 'seg_decoder_state_dict': dec}, ck)
    # batches of one: the host path's loader stacks the native-size targets of a batch, so they must agree in size
    cmd = [sys.executable, os.path.join(ROOT, 'tests', 'gpu_val_driver.py'), base, ck, str(tmp_path / 'out'), '1']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    log = r.stdout.decode()
    assert r.returncode == 0, log[-3000:]
    res = json.loads([l for l in log.splitlines() if l.startswith('RESULT ')][-1][7:])
    print({k: res[k] for k in ('sizes', 'same_mask', 'foreground', 'ret_host', 'ret_gpu')})
    assert len(res['sizes']) == 6 and [800, 800] in res['sizes'] and len(set(map(tuple, res['sizes']))) == 6
    assert any(h != w for h, w in res['sizes'])
    assert res['untouched']
    assert all(res['same_post'])                                                   # stage b on the pass's own masks
    for i, same in enumerate(res['same_mask']):
        if same:
            assert res['dice_gpu'][i] == res['dice_host'][i], i
        else:
            assert np.allclose(res['dice_gpu'][i], res['dice_host'][i], atol=DICE_TOL), i
    if all(res['same_mask']):
        assert res['ret_gpu'] == res['ret_host']
    assert abs(res['ret_gpu'] - res['ret_host']) <= 100 * DICE_TOL
    host_csv, gpu_csv = res['csv']
    assert len(gpu_csv.strip().splitlines()) == 1 and _csv_layout(gpu_csv) == _csv_layout(host_csv)
    assert np.allclose(_csv_values(gpu_csv), _csv_values(host_csv), atol=DICE_TOL)


def _train(data, out, extra=(), dataset='fundus'):
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs',
           '1,2,3', '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', out, '--epochs', '2', '--max_iters', '4', '--num_workers', '0', '--log_every', '2', '--deterministic']
    return subprocess.run(cmd + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


def test_train_cli_gpu_val_gives_the_same_model_and_numbers(tmp_path):
    """Two epochs (two validations) without the flag, with it, and with it beside --gpu_data: final_model.pth bit for bit (validation
    disturbs neither the training state nor a random generator), the same keep-best files, the same CSV numbers."""
    data = str(tmp_path / 'data')
    SD.make_fundus_tree(data, n_train=8, n_test=10, hw=(136, 152), vary=False)       # 10 test images: a batch of 8 and one of 2
    runs = []
    for name, extra in (('host', []), ('gpu_val', ['--gpu_val']), ('both', ['--gpu_val', '--gpu_data'])):
        out = str(tmp_path / name)
        r = _train(data, out, extra)
        log = r.stdout.decode()
        assert r.returncode == 0, log[-3000:]
        assert ('gpu_val: 10 test images' in log) == ('--gpu_val' in extra)
        assert log.count('val_cup_dice') == 2
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
        assert np.allclose(_csv_values(csv), _csv_values(csv0), atol=DICE_TOL)


def test_train_cli_gpu_val_refuses_prostate(tmp_path):
    r = _train(str(tmp_path), str(tmp_path / 'out'), ['--gpu_val'], dataset='prostate')
    assert r.returncode != 0 and b'--gpu_val covers the in-training Fundus validation only' in r.stdout
