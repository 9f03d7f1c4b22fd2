#!/usr/bin/env python3
"""The --gpu_val kernels on masks of the kind a trained network gives (csrc/val_post.hip): N images of 800x800, a noisy disc with
a cup inside, islands and pinholes, in batches of 8 like train.py's validation.  Prints the time of one pass by stage (device
events around the whole pass, warmed up) and what scipy takes for the same planes on one core.
    python scripts/gpu_val_bench.py [--n 80] [--batch 8] [--passes 5]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ram-dsir_amd')]
import numpy as np
import torch

from ramdsir import gpu_val as G
from utils.metrics import postprocess_binary

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=80)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--passes', type=int, default=5)
a = ap.parse_args()
S, H, W = 256, 800, 800
rng = np.random.RandomState(0)
yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
logits = np.empty((a.n, 2, S, S), np.float32)
for i in range(a.n):
    cy, cx, r = rng.uniform(0.4 * S, 0.6 * S), rng.uniform(0.4 * S, 0.6 * S), rng.uniform(0.2, 0.35) * S
    d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
    for c, rad in ((0, 0.5 * r), (1, r)):
        logits[i, c] = 0.5 * (rad - d) + rng.normal(0, 1.5, (S, S)) + 1.1       # sigmoid > 0.75 inside, a ragged rim, specks outside
dev = torch.device('cuda:0')
lg = torch.from_numpy(logits).to(dev)
gt = torch.from_numpy((rng.uniform(size=a.n * 2 * H * W) < 0.3).astype(np.uint8)).to(dev)
sizes = [(H, W)] * a.n
gt_offs = [2 * H * W * i for i in range(a.n)]


def one_pass(stage):
    counts = torch.zeros((a.n, 2, 3), dtype=torch.int32, device=dev)
    masks = []
    for b0 in range(0, a.n, a.batch):
        b1 = min(b0 + a.batch, a.n)
        recs, nbytes = G.image_records(sizes[b0:b1], gt_offs[b0:b1], range(b0, b1))
        if stage in ('a', 'all'):
            m = G.threshold(lg[b0:b1], recs, b1 - b0, nbytes)
        else:
            m = stage[b0 // a.batch]
        masks.append(m)
        if stage != 'a':
            G.post(m, recs, b1 - b0, nbytes, gt, counts)
    return masks, counts


def timed(stage):
    one_pass(stage)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.passes):
        one_pass(stage)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.passes


masks, _ = one_pass('a')
torch.cuda.synchronize()
fg = float(torch.cat(masks).float().mean())
print('%d images of %dx%d in batches of %d, foreground %.3f' % (a.n, H, W, a.batch, fg))
print('stage a (sigmoid + resize + threshold): %.2f ms per pass' % timed('a'))
print('stages b + c (components, holes, counts): %.2f ms per pass' % timed(masks))
print('all stages: %.2f ms per pass' % timed('all'))
m0 = masks[0].cpu().numpy()[:2 * H * W].reshape(2, H, W)
t0 = time.time()
for _ in range(3):
    postprocess_binary(m0)
print('scipy postprocess_binary, one image on one core: %.1f ms' % ((time.time() - t0) / 3 * 1e3))
