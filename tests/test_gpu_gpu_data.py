"""-m gpu: train.py --gpu_data -- the augmentation kernels (rd_fundus_batch / rd_prostate_batch) against the host path bit for
bit, train.py's loader construction through both paths, and the CLI end to end (the same checkpoint with and without the flag)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fundus_tree(root, n_train=4):
    """synth_data's varying sizes (non-square) plus one 800 x 800 ROI with its mask (the real ROIs' size)."""
    base = SD.make_fundus_tree(root, n_train=n_train, n_test=1, vary=True)
    rng = np.random.RandomState(3)
    ri = os.path.join(base, 'Domain2', 'train', 'ROIs', 'image', 'd2_train_00.png')
    Image.fromarray(SD._smooth_rgb(rng, 800, 800)).save(ri)
    Image.fromarray(SD._disc_mask(rng, 800, 800)).save(ri.replace('/image/', '/mask/'))
    return base


def _host_fundus(rec, S=256):
    """The host path's pixels for one record: PIL, as Fundus_Multi + Resize + RandomScaleCrop compute them."""
    from dataset.transform import fundus_mask
    ik, pk, sw, sh, cx, cy, lam = rec
    mk = _host_fundus.masks[ik]
    img = Image.open(ik).resize((S, S), Image.BILINEAR)
    m = Image.open(mk).convert('L').resize((S, S), Image.NEAREST)
    if (sw, sh) != (S, S):
        img, m = img.resize((sw, sh), Image.BILINEAR), m.resize((sw, sh), Image.NEAREST)
    box = (cx, cy, cx + S, cy + S)
    other = np.array(Image.open(pk).resize((S, S), Image.BILINEAR))
    return np.array(img.crop(box)), other, np.float32(lam), fundus_mask(np.array(m.crop(box)))


def test_fundus_batch_kernel_matches_pil_bit_for_bit(tmp_path):
    from ramdsir.gpu_data import FundusParams, FundusResident, _key
    base = _fundus_tree(str(tmp_path))
    dss = [FundusParams(base_dir=base, split='train', domain_idx_list=[d], is_out_domain=True, test_domain_idx=0) for d in (1, 2, 3)]
    res = FundusResident(dss, workers=4)
    _host_fundus.masks = {_key(base, l.split(' ')[0]): _key(base, l.split(' ')[1]) for ds in dss for l in ds.id_path}
    assert res.desc.band_rows >= 1 and res.desc.src_rows >= 50                     # the 800 x 800 source is resident
    # coin off; only w; only h; both; exactly S and 1.5 S; crops at 0 and at the largest offset
    geo = [(256, 256, 0, 0), (384, 256, 128, 0), (300, 256, 0, 0), (256, 300, 0, 44), (256, 384, 0, 0), (257, 383, 1, 127),
           (384, 384, 128, 128), (384, 384, 0, 0), (320, 290, 17, 5), (383, 257, 127, 1)]
    keys = list(_host_fundus.masks)
    allkeys = list(res.slot)
    rng = random.Random(4)
    recs = [(k, rng.choice(allkeys), sw, sh, cx, cy, rng.randint(1, 10) / 10) for k in keys for (sw, sh, cx, cy) in geo]
    assert len(recs) > 48                                                           # more than one launch chunk
    for batch in (recs[:16], recs):
        got = [t.cpu() for t in res.on_device([batch[:5], batch[5:]])]
        torch.cuda.synchronize()
        for i, rec in enumerate(batch):
            a, p, lam, m = _host_fundus(rec)
            assert np.array_equal(got[0][i].numpy(), a), ('src', rec)
            assert np.array_equal(got[1][i].numpy(), p), ('trg', rec)
            assert got[2][i].item() == lam and np.array_equal(got[3][i].numpy(), m), ('lam / mask', rec)


def _args(dataset, gpu_data, domains, test, extra=()):
    import train as T
    argv = ['--dataset', dataset, '--domain_idxs', domains, '--test_domain_idx', str(test), '--save_path', 'unused', '--num_workers', '0',
            '--is_out_domain'] + list(extra) + (['--gpu_data'] if gpu_data else [])
    return T.parse_args(argv)


def _steps(dataset, data_root, gpu_data, bsl, domains, world=1, rank=0, n=20, test=0):
    """train.py's construction (make_loaders, the shape peek, per-epoch set_epoch, iter(zip(*loaders))) with num_workers=0, seeded
    like --deterministic: the first n steps' on_device tuples."""
    import train as T
    from ramdsir import gpu_data as G
    args = _args(dataset, gpu_data, domains, test)
    random.seed(1337); np.random.seed(1337); torch.manual_seed(1337)
    dom = [int(i) for i in domains.split(',')]
    raw, samplers, loaders, max_len = T.make_loaders(args, data_root, world, rank, bsl, dom)
    res = G.preload(dataset, [dl.dataset for dl in raw], workers=4) if gpu_data else None
    next(iter(raw[0]))
    out = []
    for epoch in range(100):
        for sp in samplers:
            if sp is not None:
                sp.set_epoch(epoch)
        for batches in zip(*loaders):
            if res is not None:
                t = res.on_device(batches)
            else:
                t = tuple(torch.cat([b[k] for b in batches], 0).cuda(non_blocking=True) for k in range(4))
            out.append(tuple(x.cpu() for x in t))
            if len(out) == n:
                return out, max_len
    return out, max_len


def _truncate(path, n):
    lines = open(path).read().split('\n')[:n]
    open(path, 'w').write('\n'.join(lines) + '\n')


@pytest.mark.parametrize('world,rank', [(1, 0), (2, 1)])
def test_fundus_loaders_equal_host_path(tmp_path, world, rank):
    base = _fundus_tree(str(tmp_path), n_train=10)
    _truncate(os.path.join(base, 'Domain3_train.list'), 6)                          # lists of different lengths: cycle replay
    _truncate(os.path.join(base, 'Domain4_train.list'), 8)
    bsl = [2, 1, 2]
    host, ml = _steps('fundus', base, False, bsl, '1,2,3', world, rank)
    gpu, ml2 = _steps('fundus', base, True, bsl, '1,2,3', world, rank)
    assert ml == ml2 and len(host) == len(gpu) == 20
    for s, (h, g) in enumerate(zip(host, gpu)):
        for k in range(4):
            assert h[k].dtype == g[k].dtype and torch.equal(h[k], g[k]), (s, k)


def test_prostate_loaders_equal_host_path(tmp_path):
    base = SD.make_prostate_tree(str(tmp_path), n=4, S=32)
    for f in ('d3_s00.npy', 'd3_s01.npy'):                                          # a shorter domain
        for sub in ('image', 'mask'):
            os.remove(os.path.join(base, 'Domain3', sub, f))
    bsl = [2, 1, 2, 2, 1]
    host, _ = _steps('prostate', base, False, bsl, '1,2,3,4,5')
    gpu, _ = _steps('prostate', base, True, bsl, '1,2,3,4,5')
    assert len(host) == len(gpu) == 20
    for s, (h, g) in enumerate(zip(host, gpu)):
        for k in range(4):
            assert h[k].dtype == g[k].dtype and torch.equal(h[k], g[k]), (s, k)


def _train(data, dataset, out, gpu_data, extra=()):
    domains = '1,2,3' if dataset == 'fundus' else '1,2,3,4,5'
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs',
           domains, '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', out, '--epochs', '3', '--max_iters', '6', '--num_workers', '0', '--log_every', '2', '--deterministic']
    cmd += list(extra) + (['--gpu_data'] if gpu_data else [])
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_gpu_data_gives_the_same_model(tmp_path, dataset):
    data = str(tmp_path / 'data')
    if dataset == 'fundus':
        base = _fundus_tree(data, n_train=8)
        os.remove(os.path.join(base, 'Domain1_test.list'))                          # no in-training evaluation
    else:
        SD.make_prostate_tree(data, n=4, S=64)
    cks = []
    for gd in (False, True):
        out = str(tmp_path / ('out%d' % gd))
        r = _train(data, dataset, out, gd)
        log = r.stdout.decode()
        assert r.returncode == 0, log[-3000:]
        assert ('gpu_data:' in log) == gd
        cks.append(torch.load(os.path.join(out, 'final_model.pth'), map_location='cpu'))
    for part in cks[0]:
        a, b = cks[0][part], cks[1][part]
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (part, k)


def test_train_cli_gpu_data_refuses_a_non_rgb_image(tmp_path):
    data = str(tmp_path / 'data')
    base = _fundus_tree(data, n_train=8)
    bad = os.path.join(base, 'Domain2', 'train', 'ROIs', 'image', 'd2_train_03.png')
    Image.open(bad).convert('L').save(bad)
    r = _train(data, 'fundus', str(tmp_path / 'out'), True)
    log = r.stdout.decode()
    assert r.returncode != 0 and 'd2_train_03.png has mode L' in log, log[-3000:]
