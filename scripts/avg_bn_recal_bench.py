#!/usr/bin/env python3
"""What train.py --avg_bn_recal K costs (profiles/avg_bn_recal.md), on bench.py's C2 and C3 trainers with K = 16:

  (1) the capture: the time of a pipelined training step (averaging on in both variants) with and without the copy of the step's
      clean input into the ring armed -- windows of STEPS steps between two device events, five steps of lead in front of the first
      event, the two variants alternating in one process over ROUNDS rounds;
  (2) the pass: K forward lists + K rd_bn_recal launches + one weight repack over a full ring, between two device events on an idle
      stream (as at an epoch end, which train.py has just synchronised) and as host wall time around it, ROUNDS times; and the
      device time of rd_bn_recal alone, REPS calls between two events.

Medians, minima and maxima are printed.   python scripts/avg_bn_recal_bench.py [--config C2] [--k 16] [--steps 40] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir import _lib as L, avg_bn as AB
from ramdsir.trainer import FusedTrainer

CONFIGS = {'C2': dict(dataset='fundus', bs=[2, 3, 3], size=400, consistency='kd', lr=2e-3),
           'C3': dict(dataset='prostate', bs=[2, 2, 2, 2, 2], size=384, consistency='mse', lr=1e-3)}

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='C2', choices=sorted(CONFIGS))
ap.add_argument('--k', type=int, default=16)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=50)
a = ap.parse_args()
cfg = CONFIGS[a.config]

dev = torch.device('cuda', 0)
torch.manual_seed(0)
bs, S, fundus = cfg['bs'], cfg['size'], cfg['dataset'] == 'fundus'
B = sum(bs)
tr = FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=len(bs)).to(dev),
                  bs, S, S, dataset=cfg['dataset'], consistency=cfg['consistency'], lr=cfg['lr'], total_iters=100000, dtype=torch.bfloat16)
tr.enable_avg_weights('uniform', 0.999, 0)
recal = tr.enable_avg_bn_recal(a.k)
ring = recal.ring

gen = torch.Generator(device=dev).manual_seed(5)
batches = []
for i in range(4):
    if fundus:
        src = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
        trg = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
        tgt = (torch.rand(B, 2, S, S, device=dev, generator=gen) > 0.5).float()
    else:
        src = torch.rand(B, S, S, 3, device=dev, generator=gen) * 2 - 1
        trg = torch.rand(B, S, S, 3, device=dev, generator=gen) * 2 - 1
        tgt = (torch.rand(B, S, S, device=dev, generator=gen) > 0.7).long()
    batches.append((src, trg, torch.rand(B, device=dev, generator=gen), tgt))

taken = 0                                                   # steps so far: every call trains on the batch the previous one announced


def window(armed):
    global taken
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(a.steps + 5):
        if i == 5:                                          # five steps of lead: the host is ahead of the device from here on
            e0.record()
        if armed:
            ring.count = i % a.k                            # every step of the window copies, into the entries in turn
            tr.arm_bn_capture()
        tr.step(*batches[taken % 4], next_batch=batches[(taken + 1) % 4])
        taken += 1
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


print('%s: %s, batch %s at %d x %d, bf16; ring of %d entries, %.1f MB per entry; %d BatchNorm sites, max C %d'
      % (a.config, cfg['dataset'], bs, S, S, a.k, ring.buf[0].numel() * ring.buf.element_size() / 1e6, recal.forward.n_sites,
         recal.forward.max_c))
window(False), window(True)                                  # warm-up
steps = {False: [], True: []}
for _ in range(a.rounds):
    for armed in (False, True):
        steps[armed].append(window(armed))
for armed in (False, True):
    t = steps[armed]
    print(json.dumps({'what': 'pipelined step, %s' % ('capture armed in every step' if armed else 'no capture'),
                      'ms_per_step_median': round(statistics.median(t), 4), 'min': round(min(t), 4), 'max': round(max(t), 4),
                      'windows': len(t), 'steps_per_window': a.steps}))
diff = statistics.median([x - y for x, y in zip(steps[True], steps[False])])
print(json.dumps({'what': 'armed - plain, median of the per-round differences', 'us': round(1e3 * diff, 2),
                  'ratio_to_the_plain_step': round(diff / statistics.median(steps[False]), 5)}))

# ---- (2) the pass over a full ring
ring.count = a.k
recal.run_pass()                                            # warm-up (plan buffers touched, modules loaded)
torch.cuda.synchronize()
dev_ms, wall_ms = [], []
for _ in range(a.rounds):
    ring.count = a.k
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    recal.run_pass()
    e1.record()
    torch.cuda.synchronize()
    wall_ms.append(1e3 * (time.perf_counter() - t0))
    dev_ms.append(e0.elapsed_time(e1))
step_ms = statistics.median(steps[False])
for name, t in (('device events', dev_ms), ('host wall clock, synchronised', wall_ms)):
    med = statistics.median(t)
    print(json.dumps({'what': 'one pass: %d forward lists + %d rd_bn_recal + 1 repack, %s' % (a.k, a.k, name), 'ms_median': round(med, 3),
                      'min': round(min(t), 3), 'max': round(max(t), 3), 'in_plain_steps': round(med / step_ms, 2)}))
print(json.dumps({'what': 'launches of one batch of the pass', **recal.forward.launches()}))

fwd = recal.forward
scratch = torch.zeros(64, dtype=torch.float32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
ker = []
for _ in range(a.rounds):
    L.check(L.lib().rd_box_probe(1, scratch.data_ptr(), None, 60000, stream), 'filler')      # the host gets ahead of the device
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(a.reps):
        L.check(AB.run(fwd.arr, fwd.table_dev, fwd.n_sites, fwd.max_c, 1 + r % 7), 'rd_bn_recal')
    e1.record()
    torch.cuda.synchronize()
    ker.append(e0.elapsed_time(e1) * 1e3 / a.reps)
print(json.dumps({'what': 'rd_bn_recal alone, %d sites, back to back' % fwd.n_sites, 'us_per_call_median': round(statistics.median(ker), 2),
                  'min': round(min(ker), 2), 'max': round(max(ker), 2)}))
