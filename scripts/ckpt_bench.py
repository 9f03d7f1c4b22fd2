#!/usr/bin/env python3
"""Device time of rd_snapshot at the real state size (profiles/ckpt.md): the gather and the scatter of a C2 trainer's ranges against
torch.Tensor.copy_ of the same number of bytes (one contiguous device-to-device copy) and rd_box_probe's streaming copy on this box.

Every candidate is enqueued REPS times between two events BEHIND a few milliseconds of MFMA filler (rd_box_probe which 1), so that the
host is ahead of the device and the window holds back-to-back device work, not enqueue gaps; the candidates alternate over ROUNDS
rounds and the median, minimum and maximum per call are printed.   python scripts/ckpt_bench.py [--size 400] [--reps 20] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir import _lib as L, ckpt as CK
from ramdsir.trainer import FusedTrainer

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=400)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=7)
a = ap.parse_args()

dev = torch.device('cuda', 0)
torch.manual_seed(0)
bs = [2, 3, 3]
tr = FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(dev), bs,
                  a.size, a.size, dataset='fundus', consistency='kd', lr=2e-3, total_iters=1000, dtype=torch.bfloat16)
st = CK.TrainState(tr)
lib = L.lib()
stream = torch.cuda.current_stream().cuda_stream
n16 = st.blob_bytes // 16 * 16
src = torch.randint(0, 255, (n16,), dtype=torch.uint8, device=dev)
dst = torch.empty_like(src)
scratch = torch.zeros(64, dtype=torch.float32, device=dev)
# the three arenas alone: what the ~190 small ranges cost on top
big = st.named[:3]
big_table, _ = CK.layout(big)
big_arr, big_chunks = CK.build_table([(t.data_ptr(), e['bytes'], e['offset']) for (_, t), e in zip(big, big_table)])
big_dev = CK.upload_table(big_arr, 3, dev)
sums = st.dev.data_ptr() + st.blob_bytes


def snap(direction):
    L.check(CK.run(st.arr, st.table_dev, st.n, st.chunks, st.dev.data_ptr(), st.blob_bytes, sums, direction, stream), 'rd_snapshot')


def snap_big():
    L.check(CK.run(big_arr, big_dev, 3, big_chunks, st.dev.data_ptr(), st.blob_bytes, sums, 0, stream), 'rd_snapshot')


cands = {
    'rd_snapshot gather (%d ranges)' % st.n: lambda: snap(0),
    'rd_snapshot scatter (%d ranges)' % st.n: lambda: snap(1),
    'rd_snapshot gather (the 3 arenas only)': snap_big,
    'torch copy_ (one contiguous copy)': lambda: dst.copy_(src),
    'rd_box_probe streaming copy': lambda: L.check(lib.rd_box_probe(0, src.data_ptr(), dst.data_ptr(), n16, stream), 'box'),
}
for f in cands.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {k: [] for k in cands}
for _ in range(a.rounds):
    for name, f in cands.items():
        L.check(lib.rd_box_probe(1, scratch.data_ptr(), None, 60000, stream), 'filler')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
print('state: %d bytes in %d ranges (%d chunks of %d bytes); %d calls per window, %d windows per candidate' %
      (st.blob_bytes, st.n, st.chunks, L.SNAP_CHUNK, a.reps, a.rounds))
for name, t in times.items():
    med = statistics.median(t)
    print(json.dumps({'what': name, 'us_per_call_median': round(med, 2), 'min': round(min(t), 2), 'max': round(max(t), 2),
                      'GBps_read_plus_write': round(2 * st.blob_bytes / med / 1e3, 1)}))
st.close()
