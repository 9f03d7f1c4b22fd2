#!/usr/bin/env python3
"""Whole validation passes on a resident synthetic set, through the drop-in modules and through the fused forward (train.py
--fused_val; ramdsir/infer.py): Fundus -- N images of 800x800 (inputs 256x256), test batch 8; Prostate -- volumes of the real plane
size (384x384) with ragged slice counts, test batch 8.  Random-init networks: the time does not depend on the weights.

Per run: --passes passes after one warm-up pass; device time from events around the passes, host time = wall clock from the start of
a pass until it reaches its only synchronisation (the copy of the counts).  The two paths alternate, --runs runs each.  The storage
dtype is the module path's (fp32 unless RAMDSIR_DTYPE=bf16 or --dtype), the one train.py validates in.
    python scripts/fused_val_bench.py [--dataset fundus|prostate|both] [--n 80] [--batch 8] [--passes 5] [--runs 3] [--dtype f32|bf16]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ram-dsir_amd')]
import numpy as np
import torch

from networks.unet import Encoder, Decoder
from ramdsir import gpu_val as G, gpu_val_volumes as V, modules as M
from ramdsir.infer import EvalForward

ap = argparse.ArgumentParser()
ap.add_argument('--dataset', default='both', choices=['fundus', 'prostate', 'both'])
ap.add_argument('--n', type=int, default=80)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--passes', type=int, default=5)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--dtype', default=None, choices=['f32', 'bf16'])
a = ap.parse_args()
if a.dtype:
    M.set_storage_dtype(torch.bfloat16 if a.dtype == 'bf16' else torch.float32)
dev = torch.device('cuda:0')
rng = np.random.RandomState(0)
torch.manual_seed(0)
enc, dec = Encoder().to(dev).eval(), Decoder(num_classes=2).to(dev).eval()
fwd = EvalForward.from_modules(enc, dec)


class EnqueueClock:
    """Stamps the moment a pass reaches Tensor.cpu(), its only synchronisation: everything before it is enqueue."""

    def __enter__(self):
        self.orig, self.t = torch.Tensor.cpu, None
        clock = self

        def cpu(t, *args, **kw):
            clock.t = time.perf_counter()
            return clock.orig(t, *args, **kw)
        torch.Tensor.cpu = cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self.orig


def run(one_pass):
    one_pass()                                              # warm-up: plans, caches
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = 0.0
    e0.record()
    for _ in range(a.passes):
        with EnqueueClock() as c:
            t0 = time.perf_counter()
            one_pass()
        host += c.t - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.passes, 1e3 * host / a.passes


def module_launches(batch_launches):
    """Launches of one batch through the modules, from their plans: both launch lists, the weight repack and the arena clear of each
    module (modules.run_fused), the layout conversions at the module boundaries, the batch's own kernels around the forward pass."""
    out = {}
    for m in (enc, dec):
        pl = max((p for pool in m._plans.values() for p in pool), key=lambda p: p.N)
        for op in pl.fwd:
            out[op[0].__name__] = out.get(op[0].__name__, 0) + 1
        out['rd_pack_weights_batched'] = out.get('rd_pack_weights_batched', 0) + 1
        out['memset (statistics arena)'] = out.get('memset (statistics arena)', 0) + 1
    out['rd_nchw_to_nhwc'] = 1 + 5
    out['rd_nhwc_to_nchw'] = 5 + 1
    out.update(batch_launches)
    return out


def report(name, shape, passes, mod_extra, fused_extra):
    print('\n%s' % name)
    runs = {'modules': [], 'fused': []}
    for r in range(a.runs):
        for path in ('modules', 'fused'):
            runs[path].append(run(passes[path]))
    lm = module_launches(mod_extra)
    lf = dict(fwd.launches(*shape), **fused_extra)
    print('  launches per batch, modules: %d  %s' % (sum(lm.values()), lm))
    print('  launches per batch, fused:   %d  %s   (+ per pass: rd_bn_eval_coeffs%s)'
          % (sum(lf.values()), lf, ', rd_pack_weights_batched' if fwd.owns_pack else ''))
    for path in ('modules', 'fused'):
        print('  %-8s device ms per pass: %s   host ms per pass: %s' % (path, ' '.join('%8.2f' % d for d, _ in runs[path]),
                                                                      ' '.join('%8.2f' % h for _, h in runs[path])))
    for k, what in ((0, 'device'), (1, 'host')):
        m, f = [r[k] for r in runs['modules']], [r[k] for r in runs['fused']]
        spread, gain = max(m) - min(m), np.mean(m) - np.mean(f)
        print('  %s: modules %.2f ms (spread %.2f), fused %.2f ms: %.2f ms less, %s the spread of the module runs'
              % (what, np.mean(m), spread, np.mean(f), gain, 'MORE than' if gain > spread else 'NOT more than'))


if a.dataset in ('fundus', 'both'):
    S, H, W = 256, 800, 800
    inputs = torch.from_numpy(rng.normal(0, 1, (a.n, 3, S, S)).astype(np.float32)).to(dev)
    gt = torch.from_numpy((rng.uniform(size=a.n * 2 * H * W) < 0.3).astype(np.uint8)).to(dev)
    res = G.ValResident(inputs, gt, [2 * H * W * i for i in range(a.n)], [(H, W)] * a.n, ['i%d' % i for i in range(a.n)])
    a_, b_ = G.validate(enc, dec, res, a.batch), G.validate(enc, dec, res, a.batch, forward=fwd)
    assert a_ == b_, 'the two paths disagree'
    post = {'val_post kernels': 10}
    report('Fundus: %d images of %dx%d, inputs %dx%d, test batch %d, %s storage' % (a.n, H, W, S, S, a.batch, fwd.dtype),
           (a.batch, S, S), {'modules': lambda: G.validate(enc, dec, res, a.batch), 'fused': lambda: G.validate(enc, dec, res, a.batch, forward=fwd)},
           dict(post, rd_val_threshold=1), dict(post, rd_val_threshold_nhwc=1, **{'copy (resident slice -> plan input)': 1}))

if a.dataset in ('prostate', 'both'):
    shapes = [(d, 384, 384) for d in (20, 24, 17, 28, 15, 22)]
    volumes = [torch.from_numpy(rng.uniform(0, 1, s).astype(np.float32)).to(dev) for s in shapes]
    vox = sum(d * h * w for d, h, w in shapes)
    gtv = torch.from_numpy((rng.uniform(size=vox) < 0.2).astype(np.uint8)).to(dev)
    empty = [torch.from_numpy((rng.uniform(size=d) < 0.2).astype(np.uint8)).to(dev) for d, _, _ in shapes]
    resv = V.VolResident(volumes, gtv, empty, shapes, ['v%d' % i for i in range(len(shapes))], 0)
    ka, kb = {}, {}
    V.validate(enc, dec, resv, a.batch, keep=ka)
    V.validate(enc, dec, resv, a.batch, keep=kb, forward=fwd)
    assert ka['counts'] == kb['counts'], 'the two paths disagree'
    report('Prostate: volumes %s, test batch %d, %s storage' % (shapes, a.batch, fwd.dtype), (a.batch, 384, 384),
           {'modules': lambda: V.validate(enc, dec, resv, a.batch), 'fused': lambda: V.validate(enc, dec, resv, a.batch, forward=fwd)},
           dict(rd_vol_stack=1, rd_vol_argmax=1), dict(rd_vol_stack_nhwc=1, rd_vol_argmax_nhwc=1))
