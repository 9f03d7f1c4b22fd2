#!/usr/bin/env python3
"""End-to-end throughput of train.py with real files: a synthetic Fundus tree of 800x800 RGB PNG ROIs
(the size of the reference's ROIs) + gray masks in the reference's list layout, then the drop-in CLI with the reference's
loader settings (train.py:558: batch [3,6,7] for target 0, num_workers=8 per domain loader, pin_memory, shuffle,
Resize(256) + RandomScaleCrop(256)).  Prints train.py's `train throughput` line; compare with bench.py's resident-input
number at --size 256.   python scripts/e2e_train_throughput.py [--n 48] [--iters 120] [--workers 8] [--gpu_data] [--gpu_val] [--n_test 8] [--tb_images N] [--tb_every_iter] [--tb_health] [--log_every N] [--ckpt_every N]
--gpu_data: train.py's GPU-resident data path (decode once, one augmentation launch per step; --workers sizes the preload pool).
--gpu_val: train.py's GPU validation path; --n_test: test images per domain (the real lists hold 51-80).
--tb_images N: train.py's TensorBoard image grids every N iterations (also prints the writer thread's host time per logging iteration).
--tb_every_iter / --tb_health: train.py's per-step record ring; --log_every N: how often train.py reads the losses back (default 50).
--ckpt_every N: train.py's resumable-state snapshot every N epochs (also prints the writer thread's per-stage line).
--tree DIR: build the tree in DIR, or use the one already there (several runs on the same files)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests')]
import synth_data as SD

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=160)            # 160 / 3 = 53 iterations per epoch, like the real lists (train.py:210)
ap.add_argument('--iters', type=int, default=270)
ap.add_argument('--workers', type=int, default=8)
ap.add_argument('--dtype', default='bf16')
ap.add_argument('--gpu_data', action='store_true')
ap.add_argument('--gpu_val', action='store_true')
ap.add_argument('--fused_val', action='store_true')
ap.add_argument('--n_test', type=int, default=8)
ap.add_argument('--tb_images', type=int, default=0)
ap.add_argument('--tb_every_iter', action='store_true')
ap.add_argument('--tb_health', action='store_true')
ap.add_argument('--log_every', type=int, default=50)
ap.add_argument('--ckpt_every', type=int, default=0)
ap.add_argument('--tree', default=None)
a = ap.parse_args()
with tempfile.TemporaryDirectory() as out_tmp:
    tmp = a.tree or out_tmp
    if not os.path.exists(os.path.join(tmp, 'fundus', 'Domain1_test.list')):
        t0 = time.time()
        SD.make_fundus_tree(tmp, n_train=a.n, n_test=a.n_test, hw=(800, 800), vary=False)
        print('tree: 4 domains x (%d train + %d test) PNGs of ~800x800 in %.1f s' % (a.n, a.n_test, time.time() - t0), flush=True)
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', tmp, '--dataset', 'fundus', '--domain_idxs', '1,2,3',
           '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency', '--consistency_type', 'kd', '--save_path',
           os.path.join(out_tmp, 'out'), '--epochs', '1000', '--max_iters', str(a.iters), '--num_workers', str(a.workers), '--log_every', str(a.log_every),
           '--dtype', a.dtype] + (['--gpu_data'] if a.gpu_data else []) + (['--gpu_val'] if a.gpu_val else []) + \
          (['--fused_val'] if a.fused_val else []) + \
          (['--tb_images', str(a.tb_images)] if a.tb_images else []) + \
          (['--tb_every_iter'] if a.tb_every_iter else []) + (['--tb_health'] if a.tb_health else []) + \
          (['--ckpt_every', str(a.ckpt_every)] if a.ckpt_every else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print('\n'.join(l for l in out.splitlines() if 'throughput' in l or 'epoch ' in l or 'gpu_data:' in l or 'gpu_val:' in l or 'tb_images:' in l or l.startswith('ckpt:') or 'Error' in l or 'error' in l)[-3000:])
    sys.exit(r.returncode)
