#!/usr/bin/env python3
"""What the gradient accumulation of train.py --accum_steps costs (profiles/accum.md), on a C2 trainer (bench.py's flagship shape:
B = 8, bf16, fundus) at --size 400.

--mode kernel   one call alone on the trainer's real arenas: windows of CALLS back-to-back calls between two device events, the
                variants alternating in one process over ROUNDS rounds; microseconds per call
                    adam    rd_adam_step (a one-thread prepare launch and the update launch: 7 words per parameter)
                    first   rd_grad_accum at k = 0 of 3: the copy, 2 words per parameter (1 read, 1 written)
                    middle  rd_grad_accum at k = 1 of 3: the sum, 3 words per parameter (2 read, 1 written)
                    last    rd_grad_accum at k = 2 of 3: the mean in place, 3 words per parameter (2 read, 1 written)
--mode step     the time of a pipelined training step, as scripts/optim_bench.py measures it: windows of STEPS steps with five steps
                of lead
                    off     the plain step (one native launch list that ends in rd_adam_step + repack)
                    acc2    enable_grad_accum(2): the list ends at the encoder backward, rd_grad_accum follows at every step and
                            rd_adam_step + repack as direct calls at every second one

--root TREE measures the package of another checkout of this repository (its ram-dsir_amd/, built there): with --variants adam (or
off) this is how the parent commit is measured by the same script, process by process in alternation with this tree's.

    python scripts/accum_bench.py --mode kernel [--calls 200] [--rounds 7] [--variants adam,first,middle,last] [--root TREE] [--label NAME]
    python scripts/accum_bench.py --mode step [--size 400] [--steps 40] [--rounds 7] [--variants off,acc2]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--mode', choices=['kernel', 'step'], default='kernel')
ap.add_argument('--size', type=int, default=400)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--variants', type=str, default=None)
ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', type=str, default='this tree')
a = ap.parse_args()
sys.path[:0] = [os.path.join(os.path.abspath(a.root), 'ram-dsir_amd')]

import torch

from networks.unet import Encoder, Decoder, Rec_Decoder
from ramdsir import _lib as L
from ramdsir.trainer import FusedTrainer

variants = (a.variants or ('adam,first,middle,last' if a.mode == 'kernel' else 'off,acc2')).split(',')
dev = torch.device('cuda', 0)
torch.manual_seed(0)
bs = [2, 3, 3]
B, S = sum(bs), a.size if a.mode == 'step' else 64          # the arenas do not depend on the image size
tr = FusedTrainer(Encoder().to(dev), Decoder(num_classes=2).to(dev), Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).to(dev), bs,
                  S, S, dataset='fundus', consistency='kd', lr=2e-3, total_iters=100000, dtype=torch.bfloat16)
bank, ts = tr.bank, tr.ts


def report(times, unit, per):
    for v in variants:
        t = times[v]
        print(json.dumps({'tree': a.label, 'mode': a.mode, 'variant': v, '%s_median' % unit: round(statistics.median(t), 4),
                          'min': round(min(t), 4), 'max': round(max(t), 4), 'windows': len(t), per: a.calls if a.mode == 'kernel' else a.steps}))
    for v in variants[1:]:
        d = [x - y for x, y in zip(times[v], times[variants[0]])]
        print(json.dumps({'tree': a.label, 'what': '%s - %s, per-round differences (%s)' % (v, variants[0], unit),
                          'median': round(statistics.median(d), 4), 'min': round(min(d), 4), 'max': round(max(d), 4)}))


if a.mode == 'kernel':
    assert set(variants) <= {'adam', 'first', 'middle', 'last'}, variants
    gen = torch.Generator(device=dev).manual_seed(5)
    bank.grads.copy_(torch.randn(bank.n, device=dev, generator=gen) * 1e-3)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    calls = {'adam': lambda: lib.rd_adam_step(C.byref(ts.ad), st)}
    if set(variants) - {'adam'}:
        from ramdsir import accum as A
        acc = A.GradAccum(tr, 3)
        acc.acc.copy_(bank.grads)
        g, p, inv = bank.grads.data_ptr(), acc.acc.data_ptr(), float(acc.inv)
        for name, k in (('first', 0), ('middle', 1), ('last', 2)):
            calls[name] = (lambda k: lambda: lib.rd_grad_accum(g, p, bank.n, k, 3, inv, st))(k)
        print(json.dumps({'elements': bank.n, 'grad_phase': (g >> 2) & 3, 'acc_phase': (p >> 2) & 3}))

    def window(name):
        f = calls[name]
        if name in ('middle', 'last'):
            acc.acc.zero_()                                 # repeated sums stay finite: the timing is of finite data
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.calls + 20):
            if i == 20:
                e0.record()
            assert f() == 0
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # microseconds per call

    for v in variants:
        window(v)                                           # warm-up
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(window(v))
    print(json.dumps({'what': 'traffic per call in bytes', 'adam': 28 * bank.n, 'first': 8 * bank.n, 'middle': 12 * bank.n, 'last': 12 * bank.n,
                      'note': 'words per parameter: adam 4 read + 3 written, first 1 + 1, middle and last 2 + 1'}))
    report(times, 'us_per_call', 'calls_per_window')
else:
    assert set(variants) <= {'off', 'acc2'}, variants
    assert a.steps % 2 == 0, 'whole windows of two'
    gen = torch.Generator(device=dev).manual_seed(5)
    batches = []
    for i in range(4):
        src = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
        trg = (torch.rand(B, S, S, 3, device=dev, generator=gen) * 255).to(torch.uint8)
        tgt = (torch.rand(B, 2, S, S, device=dev, generator=gen) > 0.5).float()
        batches.append((src, trg, torch.rand(B, device=dev, generator=gen), tgt))
    taken = 0
    accums = {'off': None}
    if 'acc2' in variants:
        accums['acc2'] = tr.enable_grad_accum(2)

    def step():
        global taken
        tr.step(*batches[taken % 4], next_batch=batches[(taken + 1) % 4])
        taken += 1

    def window(name):
        if 'acc2' in variants:
            tr._accum = ts._accum = accums[name]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(a.steps + 5):
            if i == 5:                                      # five steps of lead: the host is ahead of the device from here on
                e0.record()
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for v in variants:
        window(v)                                           # warm-up
    times = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            times[v].append(window(v))
    report(times, 'ms_per_step', 'steps_per_window')
