#!/usr/bin/env python3
"""train.py --gpu_data in isolation: a synthetic Fundus tree of 800x800 PNG ROIs, train.py's loader construction over the parameter
datasets (batch [3,6,7], num_workers=0), the preload, then per step (a) the host time of the draws (next(zip(*loaders))) and
of the launch (FundusResident.on_device), (b) the device time of one rd_fundus_batch launch (events around --reps launches).
Prints one JSON line.   python scripts/gpu_data_bench.py [--n 48] [--steps 200] [--reps 200]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'ram-dsir_amd'), ROOT]
import numpy as np
import torch

import synth_data as SD

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=48)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--reps', type=int, default=200)
a = ap.parse_args()
import train as T
from ramdsir import gpu_data as G

with tempfile.TemporaryDirectory() as tmp:
    SD.make_fundus_tree(tmp, n_train=a.n, n_test=1, hw=(800, 800), vary=False)
    args = T.parse_args(['--save_path', 'unused', '--domain_idxs', '1,2,3', '--test_domain_idx', '0', '--is_out_domain', '--gpu_data',
                         '--num_workers', '0'])
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    bsl = T.fundus_batch_list[0]
    raw, samplers, loaders, max_len = T.make_loaders(args, os.path.join(tmp, 'fundus'), 1, 0, bsl, [1, 2, 3])
    t0 = time.time()
    res = G.preload('fundus', [dl.dataset for dl in raw], workers=16)
    t_pre = time.time() - t0
    draws, launch, it = [], [], iter(zip(*loaders))
    out = None
    for s in range(a.steps):
        t0 = time.perf_counter()
        b = next(it, None)
        if b is None:
            it = iter(zip(*loaders))
            b = next(it)
        t1 = time.perf_counter()
        out = res.on_device(b)
        t2 = time.perf_counter()
        draws.append(t1 - t0)
        launch.append(t2 - t1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        res.on_device(b)
    e0.record()
    for _ in range(a.reps):
        res.on_device(b)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({'batch': sum(bsl[:3]), 'resident_gb': round(res.nbytes / 1e9, 3), 'preload_s': round(t_pre, 2),
                      'band_rows': res.desc.band_rows, 'lds_rows': [res.desc.src_rows, res.desc.mid_rows],
                      'host_draws_ms_median': round(1e3 * float(np.median(draws)), 4),
                      'host_launch_ms_median': round(1e3 * float(np.median(launch)), 4),
                      'device_us_per_batch_incl_launch_gaps': round(1e3 * e0.elapsed_time(e1) / a.reps, 2)}))
