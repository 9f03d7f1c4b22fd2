#!/usr/bin/env python3
"""End-to-end throughput of train.py --dataset prostate with in-training validation: a synthetic tree of (S, S, 3) .npy training slices
in the reference's layout plus NIfTI volumes of the held-out site (S x S slices, 20-60 of them per volume, float32 and int16, a ball of
prostate in the middle slices, .nii.gz), then the drop-in CLI with --gpu_data.  Prints train.py's per-epoch `validation + checkpoint`
lines and its `train throughput` line.
    python scripts/e2e_prostate_throughput.py [--n 6] [--iters 12] [--volumes 30] [--size 384] [--gpu_val_volumes] [--tree DIR]
--gpu_val_volumes: train.py's GPU validation path; --tree DIR: build the tree in DIR, or use the one already there (several runs on
the same files).  The volumes are piecewise constant (8 x 8 blocks), so that writing and compressing them takes seconds: gunzip is
cheaper for the host path here than on scans."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'ram-dsir_amd')]
import numpy as np

import synth_data as SD
from utils import nifti


def make_volumes(dom, n, S, seed=20223):
    os.makedirs(dom)
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S]
    vox = 0
    for k in range(n):
        D = int(rng.randint(20, 61))
        low = rng.uniform(0, 400, (D, S // 8, S // 8))
        img = np.repeat(np.repeat(low, 8, axis=1), 8, axis=2)
        cz, cy, cx, r = D / 2.0, rng.uniform(0.4, 0.6) * S, rng.uniform(0.4, 0.6) * S, rng.uniform(0.12, 0.2) * S
        zz = np.arange(D)[:, None, None]
        ball = ((zz - cz) * (2.5 * r / D)) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        img[ball] += 500
        msk = ball.astype(np.uint8)
        msk[ball & ((yy - cy) ** 2 + (xx - cx) ** 2 < (0.5 * r) ** 2)] = 2
        nifti.write_volume(os.path.join(dom, 'Case%02d.nii.gz' % k), img.astype(np.float32 if k % 2 else np.int16))
        nifti.write_volume(os.path.join(dom, 'Case%02d_segmentation.nii.gz' % k), msk)
        vox += D * S * S
    return vox


ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=6)              # slices per training domain: n / 2 iterations per epoch
ap.add_argument('--iters', type=int, default=12)
ap.add_argument('--volumes', type=int, default=30)
ap.add_argument('--size', type=int, default=384)
ap.add_argument('--workers', type=int, default=8)
ap.add_argument('--gpu_val_volumes', action='store_true')
ap.add_argument('--tree', default=None)
a = ap.parse_args()
with tempfile.TemporaryDirectory() as out_tmp:
    tmp = a.tree or out_tmp
    if not os.path.isdir(os.path.join(tmp, 'prostate', 'ISBI')):
        t0 = time.time()
        SD.make_prostate_tree(tmp, n=a.n, S=a.size)
        vox = make_volumes(os.path.join(tmp, 'prostate', 'ISBI'), a.volumes, a.size)
        print('tree: 6 domains x %d slices of %dx%d, %d volumes (%.1f M voxels) in %.1f s' % (a.n, a.size, a.size, a.volumes, vox / 1e6,
                                                                                              time.time() - t0), flush=True)
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', tmp, '--dataset', 'prostate', '--domain_idxs',
           '1,2,3,4,5', '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd',
           '--save_path', os.path.join(out_tmp, 'out'), '--epochs', '1000', '--max_iters', str(a.iters), '--num_workers', str(a.workers),
           '--log_every', '50', '--gpu_data'] + (['--gpu_val_volumes'] if a.gpu_val_volumes else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    keys = ('throughput', 'epoch ', 'gpu_data:', 'gpu_val_volumes:', 'val_dice', 'Error', 'error')
    print('\n'.join(l for l in out.splitlines() if any(k in l for k in keys))[-4000:])
    sys.exit(r.returncode)
