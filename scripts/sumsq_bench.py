#!/usr/bin/env python3
"""What the fixed-order sum of squares (csrc/sumsq_pass.h) costs behind its two entry points (profiles/sumsq_pass.md), on a gradient
arena of the bench shape's size (ParamBank.n of the real modules, the three Adam groups as the trainer hands them to the step log):
windows of CALLS back-to-back calls between two device events, the variants alternating in one process over ROUNDS rounds;
microseconds per call.
    health  rd_step_log with the health pass (two launches)
    plain   rd_step_log without it (one launch)
    guard   rd_grad_guard (two launches)

Only entry points are used.  --root TREE measures the package of another checkout of this repository (its ram-dsir_amd/, built
there): this is how a parent commit is measured by the same script, process by process in alternation with this tree's.

    python scripts/sumsq_bench.py [--calls 200] [--rounds 5] [--root TREE] [--label NAME]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', type=str, default='this tree')
a = ap.parse_args()
sys.path[:0] = [os.path.join(os.path.abspath(a.root), 'ram-dsir_amd')]

import torch

from ramdsir import _lib as L, guard as G, step as S, step_log as SL

VARIANTS = ('health', 'plain', 'guard')
dev = torch.device('cuda', 0)
bank, _ = S.make_bank(dev, 3, 16, 2, 3)
r = bank.module_range
ranges = [r['enc'][0], r['enc'][1], r['dec'][1], r['rec'][1]]
gen = torch.Generator(device=dev).manual_seed(5)
bank.grads.copy_(torch.randn(bank.n, device=dev, generator=gen) * 1e-3)
words = lambda k: torch.zeros(k, dtype=torch.float32, device=dev)       # noqa: E731
logs = {'health': SL.StepLog(words(8), words(3), words(4), bank.grads, ranges, rows=4), 'plain': SL.StepLog(words(8), words(3), words(4), rows=4)}
workspace = torch.empty(G.workspace_bytes(bank.n) // 8, dtype=torch.float64, device=dev)
state = torch.zeros(G.STATE_BYTES // 8, dtype=torch.int64, device=dev)
gd = L.RdGradGuard()
gd.grad, gd.n, gd.max_norm, gd.workspace, gd.state = bank.grads.data_ptr(), bank.n, 1.0, workspace.data_ptr(), state.data_ptr()
lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
calls = {'health': lambda: lib.rd_step_log(C.byref(logs['health'].desc), st), 'plain': lambda: lib.rd_step_log(C.byref(logs['plain'].desc), st),
         'guard': lambda: lib.rd_grad_guard(C.byref(gd), st)}
print(json.dumps({'tree': a.label, 'elements': bank.n, 'ranges': ranges, 'chunks_health': sum(-(-(ranges[k + 1] - ranges[k]) // L.LOG_CHUNK) for k in range(3)),
                  'chunks_guard': -(-bank.n // L.LOG_CHUNK)}))


def window(name):
    f = calls[name]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(a.calls + 20):
        if i == 20:
            e0.record()
        assert f() == 0
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / a.calls              # microseconds per call


for v in VARIANTS:
    window(v)                                               # warm-up
times = {v: [] for v in VARIANTS}
for _ in range(a.rounds):
    for v in VARIANTS:
        times[v].append(window(v))
for v in VARIANTS:
    t = times[v]
    print(json.dumps({'tree': a.label, 'variant': v, 'us_per_call_median': round(statistics.median(t), 4), 'min': round(min(t), 4),
                      'max': round(max(t), 4), 'windows': [round(x, 4) for x in t], 'calls_per_window': a.calls}))
