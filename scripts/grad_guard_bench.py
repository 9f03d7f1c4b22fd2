#!/usr/bin/env python3
"""What train.py --clip_grad_norm / --skip_nonfinite costs (profiles/grad_guard.md), on a C2 trainer (bench.py's flagship shape:
B = 8, bf16) at --size 400 and at --size 128: the time of a pipelined training step

    off     the unguarded step (one native launch list that ends in Adam + repack)
    open    the guarded tail with max_norm = 1e30 (nothing is clipped)
    clip    the guarded tail with max_norm = half the median of the norms the open guard reads in front of the measurement

as windows of STEPS steps between two device events with five steps of lead, the variants alternating in one process over ROUNDS
rounds.  Medians, minima and maxima are printed, one JSON line per variant.

--root TREE measures the package of another checkout of this repository (its ram-dsir_amd/, built there): with --variants off this is
how the parent commit's step is measured by the same script, process by process in alternation with this tree's.

    python scripts/grad_guard_bench.py [--size 400] [--steps 40] [--rounds 7] [--variants off,open,clip] [--root TREE] [--label NAME]"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=400)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--variants', type=str, default='off,open,clip')
ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', type=str, default='this tree')
a = ap.parse_args()
sys.path[:0] = [os.path.join(os.path.abspath(a.root), 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir.trainer import FusedTrainer

variants = a.variants.split(',')
assert set(variants) <= {'off', 'open', 'clip'}, variants
dev = torch.device('cuda', 0)
torch.manual_seed(0)
bs = [2, 3, 3]
B, S = sum(bs), a.size
tr = FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(dev), bs,
                  S, S, dataset='fundus', consistency='kd', lr=2e-3, total_iters=100000, dtype=torch.bfloat16)
gen = torch.Generator(device=dev).manual_seed(5)
batches = []
for i in range(4):
    src = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    trg = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    tgt = (torch.rand(B, 2, S, S, device=dev, generator=gen) > 0.5).float()
    batches.append((src, trg, torch.rand(B, device=dev, generator=gen), tgt))
taken = 0                                                   # steps so far: every call trains on the batch the previous one announced


def step():
    global taken
    tr.step(*batches[taken % 4], next_batch=batches[(taken + 1) % 4])
    taken += 1


guards = {'off': None}
if 'open' in variants or 'clip' in variants:
    guards['open'] = tr.enable_grad_guard(1e30)
    norms = []
    for _ in range(9):
        step()
        norms.append(guards['open'].read()['norm'])
    max_norm = statistics.median(norms) / 2
    if 'clip' in variants:
        guards['clip'] = tr.enable_grad_guard(max_norm)
    print(json.dumps({'what': 'norms read in front of the measurement', 'median': statistics.median(norms), 'min': min(norms), 'max': max(norms),
                      'clip_max_norm': max_norm}))


def window(name):
    g = guards[name]
    tr._guard = tr.ts._guard = g
    if g is not None:
        g.sync_shadow()                                     # (the other variants have moved the buffers since this guard last ran)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(a.steps + 5):
        if i == 5:                                          # five steps of lead: the host is ahead of the device from here on
            e0.record()
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


for v in variants:
    window(v)                                               # warm-up
times = {v: [] for v in variants}
for _ in range(a.rounds):
    for v in variants:
        times[v].append(window(v))
for v in variants:
    t = times[v]
    print(json.dumps({'tree': a.label, 'size': S, 'variant': v, 'ms_per_step_median': round(statistics.median(t), 4), 'min': round(min(t), 4),
                      'max': round(max(t), 4), 'windows': len(t), 'steps_per_window': a.steps}))
for v in variants[1:]:
    d = [x - y for x, y in zip(times[v], times[variants[0]])]
    print(json.dumps({'tree': a.label, 'size': S, 'what': '%s - %s, per-round differences (us)' % (v, variants[0]),
                      'median': round(1e3 * statistics.median(d), 2), 'min': round(1e3 * min(d), 2), 'max': round(1e3 * max(d), 2)}))
for v in variants:
    if guards.get(v) is not None:
        w = guards[v].read()
        print(json.dumps({'tree': a.label, 'size': S, 'variant': v, 'steps': w['steps'], 'clipped': w['clipped'], 'skipped': w['skipped']}))
