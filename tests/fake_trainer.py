"""What the host-side code reads of a FusedTrainer, built on the CPU, and a training-state snapshot of it: shared by the CPU tests of
ramdsir/ckpt.py, avg.py, guard.py, optim.py, accum.py and of the step's tail (test_cpu_step_tail.py).  No GPU call is made."""
import types

import torch

from ramdsir import _lib as L, ckpt as CK, engine as E


def fake_trainer(seed=3):
    """The bank with Adam moments, iter / hyper and the Adam descriptor of its TrainStep, the modules' specs."""
    mods = [('enc', E.encoder_specs()), ('dec', E.decoder_specs()), ('rec', E.rec_decoder_specs(16, 3, 3))]
    bank = E.ParamBank(mods, 'cpu')
    bank.ensure_adam()
    g = torch.Generator().manual_seed(seed)
    for t in (bank.params, bank.exp_avg, bank.exp_avg_sq):
        t.copy_(torch.randn(t.shape, generator=g))
    for k, t in bank.buffers.items():
        t.copy_(torch.randint(1, 1000, t.shape, generator=g).to(t.dtype))
    ts = types.SimpleNamespace(iter=torch.tensor(41, dtype=torch.int32), hyper=torch.tensor([2e-3, 0.5, 1e-3, 41.0]), dtype=torch.bfloat16)
    ad = L.RdAdam()                                         # as TrainStep.__init__ fills it
    ad.param, ad.grad = bank.params.data_ptr(), bank.grads.data_ptr()
    ad.exp_avg, ad.exp_avg_sq = bank.exp_avg.data_ptr(), bank.exp_avg_sq.data_ptr()
    ad.n, ad.n_half_lr = bank.n, bank.module_range['enc'][1]
    ad.iter, ad.hyper_out = ts.iter.data_ptr(), ts.hyper.data_ptr()
    ad.base_lr, ad.total_iters, ad.beta1, ad.beta2, ad.eps = 2e-3, 100, 0.9, 0.999, 1e-8
    ts.ad = ad
    modules = {m: types.SimpleNamespace(_specs=s) for m, s in mods}
    return types.SimpleNamespace(bank=bank, ts=ts, modules=modules)


def fake_state(tr, extra_ranges=None, meta=None):
    """The snapshot of `tr` as ckpt.TrainState would write it.  extra_ranges: [(name, tensor)] behind the trainer's ranges, or the
    object whose named_ranges() they are (an avg.WeightAverage, a guard.GradGuard, an accum.GradAccum)."""
    extra = extra_ranges.named_ranges() if hasattr(extra_ranges, 'named_ranges') else list(extra_ranges or ())
    named = CK.trainer_ranges(tr) + extra
    table, total = CK.layout(named)
    blob = torch.zeros(total, dtype=torch.uint8)
    for (name, t), e in zip(named, table):
        raw = t.contiguous().view(-1).view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
        blob[e['offset']:e['offset'] + e['bytes']] = raw
        e['s1'], e['s2'] = CK.checksums(raw.numpy())
    return CK.make_state(table, blob, meta or dict(epoch=1, iter_num=41, previous_best=12.5), dict(manifest=CK.trainer_manifest(tr)))
