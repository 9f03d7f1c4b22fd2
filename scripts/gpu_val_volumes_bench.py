#!/usr/bin/env python3
"""The --gpu_val_volumes kernels on volumes of the kind a trained network gives (csrc/val_volume.hip): N volumes of 20-60 slices of
384 x 384, logits of a noisy ball with specks around it, in batches of 8 like train.py's validation.  Prints the time of one pass by
stage (device events around whole passes, warmed up; no forward pass) and what scipy takes for one of the volumes on one core.
    python scripts/gpu_val_volumes_bench.py [--n 30] [--batch 8] [--passes 5]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ram-dsir_amd')]
import numpy as np
import torch

from ramdsir import gpu_val_volumes as V
from utils.metrics import connectivity_region_analysis

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=30)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--passes', type=int, default=5)
a = ap.parse_args()
S = 384
dev = torch.device('cuda:0')
rng = np.random.RandomState(0)
gen = torch.Generator(device=dev).manual_seed(0)
yy, xx = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing='ij')
shapes = [(int(rng.randint(20, 61)), S, S) for _ in range(a.n)]
offs = np.concatenate([[0], np.cumsum([d * h * w for d, h, w in shapes])]).tolist()
volumes, logits, gt_empty = [], [], []
for D, _, _ in shapes:
    volumes.append(torch.randn((D, S, S), device=dev, generator=gen))
    cy, cx, r = rng.uniform(0.4, 0.6) * S, rng.uniform(0.4, 0.6) * S, rng.uniform(0.12, 0.2) * S
    zz = torch.arange(D, device=dev, dtype=torch.float32)[:, None, None]
    d = torch.sqrt(((zz - D / 2.0) * (2.5 * r / D)) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2)
    lg = torch.zeros((D + a.batch, 2, S, S), device=dev)                  # padded: a short last batch still reads `batch` slots
    lg[:D, 1] = 0.5 * (r - d) + 1.5 * torch.randn((D, S, S), device=dev, generator=gen) - 2.0      # a ragged rim, specks outside
    logits.append(lg)
    e = np.zeros(D, np.uint8)
    e[:D // 5] = 1
    e[D - D // 5:] = 1
    gt_empty.append(torch.from_numpy(e).to(dev))
gt = (torch.rand(offs[-1], device=dev, generator=gen) < 0.3).to(torch.uint8)
pred, out = torch.empty(offs[-1], dtype=torch.uint8, device=dev), torch.empty(offs[-1], dtype=torch.uint8, device=dev)
groups = [(V.volume_records(shapes[i:j], offs[i:j], slots=range(i, j))[0], j - i) for i, j in V.post_groups(shapes)]
ws = torch.empty(max(V.L.lib().rd_vol_post_workspace(r, m) for r, m in groups), dtype=torch.uint8, device=dev)


def one_pass(stages):
    counts = torch.zeros((a.n, 3), dtype=torch.int32, device=dev)
    if 'argmax' in stages:
        V.zero(pred)
    for i, (D, _, _) in enumerate(shapes):
        for frames in V.frame_batches(D, a.batch):
            if 'stack' in stages:
                V.stack(volumes[i], frames)
            if 'argmax' in stages:                           # logits of the batch's frames: slot b holds frame frames[0] + b
                V.argmax(logits[i][frames[0]:frames[0] + a.batch], frames, gt_empty[i], pred[offs[i]:offs[i + 1]], shapes[i])
    if 'post' in stages:
        for recs, m in groups:
            V.post(pred, out, recs, m, gt, counts, ws)
    return counts


def timed(stages):
    one_pass(stages)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.passes):
        one_pass(stages)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.passes


one_pass(('argmax',))
torch.cuda.synchronize()
vox = offs[-1]
print('%d volumes, %.1f M voxels, batches of %d, %d batches per pass, foreground %.3f, post-processing in %d calls, workspace %.0f MB'
      % (a.n, vox / 1e6, a.batch, sum(len(V.frame_batches(D, a.batch)) for D, _, _ in shapes), float(pred.float().mean()), len(groups),
         ws.numel() / 1e6))
print('rd_vol_stack (2.5-D batches): %.2f ms per pass' % timed(('stack',)))
print('rd_zero + rd_vol_argmax: %.2f ms per pass' % timed(('argmax',)))
print('rd_vol_post (largest component, counts): %.2f ms per pass' % timed(('post',)))
print('all stages: %.2f ms per pass' % timed(('stack', 'argmax', 'post')))
p0 = pred[offs[0]:offs[1]].cpu().numpy().reshape(shapes[0]).astype(np.float64)
t0 = time.time()
connectivity_region_analysis(p0)
print('scipy connectivity_region_analysis, one volume of %d slices on one core: %.1f ms' % (shapes[0][0], (time.time() - t0) * 1e3))
