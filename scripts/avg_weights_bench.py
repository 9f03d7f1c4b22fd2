#!/usr/bin/env python3
"""What train.py --avg_weights costs (profiles/avg_weights.md), on a C2 trainer (bench.py's flagship shape):

  (1) the device time of rd_avg_step on the trainer's real range table -- averaging (k > 0: 12 bytes per parameter) and copying
      (k <= 0: 8 bytes per parameter) -- against rd_box_probe's streaming copy of the parameter arena on this box.  Every candidate is
      enqueued REPS times between two events BEHIND a few milliseconds of MFMA filler (rd_box_probe which 1), so that the host is
      ahead of the device and the window holds back-to-back device work, not enqueue gaps;
  (2) the time of a pipelined training step with and without the pass armed: windows of STEPS steps between two events, the two
      variants alternating in one process over ROUNDS rounds.

Medians, minima and maxima are printed.   python scripts/avg_weights_bench.py [--size 400] [--reps 50] [--steps 40] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir import _lib as L, avg as AV
from ramdsir.trainer import FusedTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=400)
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=7)
a = ap.parse_args()

dev = torch.device('cuda', 0)
torch.manual_seed(0)
bs = [2, 3, 3]
B, S = sum(bs), a.size
tr = FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(dev), bs,
                  S, S, dataset='fundus', consistency='kd', lr=2e-3, total_iters=100000, dtype=torch.bfloat16)
wa = tr.enable_avg_weights('ema', 0.999, 0)
tr._avg = None                                              # armed per window below
lib = L.lib()
stream = torch.cuda.current_stream().cuda_stream
scratch = torch.zeros(64, dtype=torch.float32, device=dev)
nbytes = sum(t.numel() * t.element_size() for _, t, _, _ in wa.ranges)
n16 = tr.bank.params.numel() * 4 // 16 * 16
copy_dst = torch.empty(n16, dtype=torch.uint8, device=dev)
counter = torch.zeros((), dtype=torch.int32, device=dev)    # the kernel reads it: 0 -> every range is copied, 100 -> averaged


def avg_call():
    L.check(AV.run(wa.arr, wa.table_dev, wa.n, wa.chunks, counter.data_ptr(), L.AVG_EMA, wa.w, 0, stream), 'rd_avg_step')


def set_counter(v):
    def f():
        counter.fill_(v)
        torch.cuda.synchronize()
    return f


cands = {
    'rd_avg_step averaging (%d ranges)' % wa.n: (set_counter(100), avg_call, 12 * tr.bank.params.numel()),
    'rd_avg_step copying (%d ranges)' % wa.n: (set_counter(0), avg_call, 8 * tr.bank.params.numel()),
    'rd_box_probe streaming copy of the arena': (lambda: None, lambda: L.check(lib.rd_box_probe(0, tr.bank.params.data_ptr(), copy_dst.data_ptr(), n16, stream), 'box'),
                                                 2 * n16),
}
for prep, f, _ in cands.values():
    prep()
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {k: [] for k in cands}
for _ in range(a.rounds):
    for name, (prep, f, _) in cands.items():
        prep()
        L.check(lib.rd_box_probe(1, scratch.data_ptr(), None, 60000, stream), 'filler')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
print('averaged model: %d parameters + %d bytes of buffers in %d ranges (%d chunks of %d bytes); %d calls per window, %d windows per candidate'
      % (tr.bank.params.numel(), nbytes - 4 * tr.bank.params.numel(), wa.n, wa.chunks, L.AVG_CHUNK, a.reps, a.rounds))
for name, t in times.items():
    med = statistics.median(t)
    print(json.dumps({'what': name, 'us_per_call_median': round(med, 2), 'min': round(min(t), 2), 'max': round(max(t), 2),
                      'GBps': round(cands[name][2] / med / 1e3, 1)}))

# ---- (2) the step, with and without the pass armed
gen = torch.Generator(device=dev).manual_seed(5)
batches = []
for i in range(4):
    src = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    trg = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    tgt = (torch.rand(B, 2, S, S, device=dev, generator=gen) > 0.5).float()
    batches.append((src, trg, torch.rand(B, device=dev, generator=gen), tgt))


taken = 0                                                   # steps so far: every call trains on the batch the previous one announced


def window(armed):
    global taken
    tr._avg = wa if armed else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(a.steps + 5):
        if i == 5:                                          # five steps of lead: the host is ahead of the device from here on
            e0.record()
        tr.step(*batches[taken % 4], next_batch=batches[(taken + 1) % 4])
        taken += 1
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


window(False), window(True)                                  # warm-up
steps = {False: [], True: []}
for _ in range(a.rounds):
    for armed in (False, True):
        steps[armed].append(window(armed))
for armed in (False, True):
    t = steps[armed]
    print(json.dumps({'what': 'pipelined step, %s' % ('rd_avg_step armed' if armed else 'no averaging'), 'ms_per_step_median': round(statistics.median(t), 4),
                      'min': round(min(t), 4), 'max': round(max(t), 4), 'windows': len(t), 'steps_per_window': a.steps}))
print(json.dumps({'what': 'armed - plain, median of the per-round differences (us)',
                  'us': round(1e3 * statistics.median([x - y for x, y in zip(steps[True], steps[False])]), 2)}))
