#!/usr/bin/env python3
"""What train.py --tb_hist costs (profiles/tb_hist.md), on a C2 trainer (bench.py's flagship shape):

  (a) the device time of rd_hist alone on the trainer's real range table, for weights,grads and for all four arenas -- REPS calls
      between two events BEHIND a few milliseconds of MFMA filler (rd_box_probe which 1), so that the host is ahead of the device and
      the window holds back-to-back device work -- beside the floor it cannot beat: the bytes it reads over the HBM rate of
      profiles/r03_hbm_ceiling.txt (--hbm_tbps).  With RAMDSIR_DEBUG_LIB=1 RD_HIST_LDS_LIMITS=0 in the environment the debug build's
      variant that reads the limits through L2 is what gets timed (the product build copies them into LDS);
  (b) the time of a pipelined training step whose trainer has the histograms enabled but is not at a logging iteration, against a
      trainer without them: windows of STEPS steps between two events, alternating in one process over ROUNDS rounds.  --step_only
      prints the windows of ONE variant (--tb_hist N: enabled, armed where iteration % N == 0, which the windows avoid; 0: not enabled)
      of the package under --tree, so that two checkouts -- this one and its parent commit -- can be timed in alternation from a shell;
  (c) per logging iteration: the device time of the armed step's extra work (rd_hist + the copy, events around enqueue()), the bytes
      copied, and the writer thread's time (utils/tfevents.py QueuedWriter.seconds['histo']) over ROUNDS logging iterations.

    python scripts/tb_hist_bench.py [--size 400] [--reps 20] [--steps 40] [--rounds 7]
    python scripts/tb_hist_bench.py --step_only --tb_hist 100 [--tree PATH]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=400)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--hbm_tbps', type=float, default=5.06, help='profiles/r03_hbm_ceiling.txt: the 1 GiB copy')
ap.add_argument('--step_only', action='store_true')
ap.add_argument('--only_a', action='store_true', help='stop behind (a)')
ap.add_argument('--tb_hist', type=int, default=100)
ap.add_argument('--tree', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
sys.path[:0] = [os.path.join(a.tree, 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir import _lib as L
from ramdsir.trainer import FusedTrainer

dev = torch.device('cuda', 0)
bs = [2, 3, 3]
B, S = sum(bs), a.size


def trainer():
    torch.manual_seed(0)
    return FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(dev), bs,
                        S, S, dataset='fundus', consistency='kd', lr=2e-3, total_iters=100000, dtype=torch.bfloat16)


gen = torch.Generator(device=dev).manual_seed(5)
batches = []
for i in range(4):
    src = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    trg = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
    tgt = (torch.rand(B, 2, S, S, device=dev, generator=gen) > 0.5).float()
    batches.append((src, trg, torch.rand(B, device=dev, generator=gen), tgt))


class Loop:
    """A trainer and its iteration count: every call trains on the batch the previous one announced, arming as train.py does."""

    def __init__(self, every):
        self.tr, self.taken, self.every = trainer(), 0, every
        if every:
            self.tr.enable_tb_hist()

    def step(self):
        if self.every and self.taken % self.every == 0:
            self.tr.arm_tb_hist()
        self.tr.step(*batches[self.taken % 4], next_batch=batches[(self.taken + 1) % 4])
        if self.every and self.taken % self.every == 0:
            self.tr.take_tb_hist().raw()
        self.taken += 1

    def window(self, steps):
        """ms per step over `steps` steps that hold no logging iteration, behind five steps of lead."""
        assert not self.every or self.every > steps + 5
        while self.every and (-self.taken) % self.every < steps + 5:       # the next logging iteration would fall into the window
            self.step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(steps + 5):
            if i == 5:
                e0.record()
            self.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps


def report(what, t, unit='ms_per_step', digits=4, **more):
    print(json.dumps(dict({'what': what, unit + '_median': round(statistics.median(t), digits), 'min': round(min(t), digits),
                           'max': round(max(t), digits), 'windows': len(t)}, **more)), flush=True)


if a.step_only:
    loop = Loop(a.tb_hist)
    loop.window(a.steps)                                    # warm-up
    report('pipelined step, %s, tree %s' % ('--tb_hist %d at non-logging iterations' % a.tb_hist if a.tb_hist else 'no histograms', a.tree),
           [loop.window(a.steps) for _ in range(a.rounds)], steps_per_window=a.steps)
    sys.exit(0)

from ramdsir import tb_hist as H
from utils import tfevents

lib = L.lib()
stream = torch.cuda.current_stream().cuda_stream
scratch = torch.zeros(64, dtype=torch.float32, device=dev)
variant = 'limits through L2 (debug build)' if os.environ.get('RAMDSIR_DEBUG_LIB') == '1' and os.environ.get('RD_HIST_LDS_LIMITS') == '0' else 'limits in LDS'

# ---- (a) rd_hist alone
plain = Loop(0)
for _ in range(6):
    plain.step()                                            # real gradients and moments in the arenas
torch.cuda.synchronize()
step_ms = statistics.median([plain.window(a.steps) for _ in range(3)])
for what in (H.DEFAULT_WHAT, H.KINDS):
    h = H.TbHist(plain.tr.bank, what)
    for _ in range(3):
        h.launch(stream)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.rounds):
        L.check(lib.rd_box_probe(1, scratch.data_ptr(), None, 60000, stream), 'filler')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            h.launch(stream)
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    nbytes = 4 * plain.tr.bank.n * len(what)
    med = statistics.median(t)
    report('rd_hist alone, %s: %d ranges, %d chunks, %s' % (','.join(what), h.n, h.chunks, variant), t, 'us_per_call', 2,
           bytes_read=nbytes, floor_us_at_hbm_rate=round(nbytes / (a.hbm_tbps * 1e6), 2), GBps=round(nbytes / med / 1e3, 1),
           share_of_step_pct=round(100 * med / (1e3 * step_ms), 2), step_ms=round(step_ms, 4))

if a.only_a:
    sys.exit(0)

# ---- (b) the step at non-logging iterations, enabled against not enabled, alternating
on = Loop(a.tb_hist)
for loop in (plain, on):
    loop.window(a.steps)
steps = {False: [], True: []}
for _ in range(a.rounds):
    for loop, key in ((plain, False), (on, True)):
        steps[key].append(loop.window(a.steps))
report('pipelined step, no histograms', steps[False], steps_per_window=a.steps)
report('pipelined step, --tb_hist %d at non-logging iterations' % a.tb_hist, steps[True], steps_per_window=a.steps)
print(json.dumps({'what': 'enabled - plain, median of the per-round differences (us)',
                  'us': round(1e3 * statistics.median([x - y for x, y in zip(steps[True], steps[False])]), 2)}), flush=True)

# ---- (c) a logging iteration: enqueue() behind a drained device, the copy, the writer thread
for what in (H.DEFAULT_WHAT, H.KINDS):
    h = H.TbHist(on.tr.bank, what)
    h.enqueue(stream).raw()
    dev_t = []
    with tempfile.TemporaryDirectory() as tmp:
        wr = tfevents.QueuedWriter(tmp)
        for it in range(a.rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pending = h.enqueue(stream)
            e1.record()
            torch.cuda.synchronize()
            dev_t.append(e0.elapsed_time(e1) * 1e3)
            wr.add_histograms_at(it, pending)
        wr.close()
        sec = wr.seconds['histo']
        size = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
    report('logging iteration, %s: rd_hist + copy of %d bytes, device time' % (','.join(what), h.copy_bytes), dev_t, 'us', 1,
           writer_ms_per_iteration=dict(fetch_and_trim=round(1e3 * sec['wait'] / sec['calls'], 2), encode=round(1e3 * sec['encode'] / sec['calls'], 2),
                                        write=round(1e3 * sec['write'] / sec['calls'], 2)),
           records_per_iteration=sec['records'] // sec['calls'], event_file_bytes_per_iteration=size // sec['calls'])
