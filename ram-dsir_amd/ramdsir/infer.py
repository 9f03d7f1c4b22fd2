"""The fused inference path: Encoder + Decoder forward with frozen BatchNorm as ONE native launch list per batch geometry -- the
forward-only counterpart of step.TrainStep (train.py --fused_val; csrc/infer.hip).

A plan is an engine.Plan(training=False, frozen_bn=True) that holds both modules: its list is one rd_conv per nn.Conv2d and the
encoder's four rd_pool_fwd, walked by one rd_run_list call.  The decoder reads the encoder's raw outputs through the loaders
(act(bn(z)) formed on read, as everywhere), so nothing between the NHWC storage-dtype input and the NHWC storage-dtype logits is ever
materialised, and no NCHW tensor exists.  The BatchNorm coefficients depend only on the parameters and the running statistics: ONE
rd_bn_eval_coeffs launch per plan and pass (refresh()) replaces a finalize launch per site and batch.

Every other plan option is a module plan's, so every conv takes the route (kernel, grid, block) it takes when the drop-in modules of
networks/unet.py run in eval mode, and forms the same bits: tests/test_cpu_fused_val.py pins the routes, tests/test_gpu_fused_val.py
the logits.
"""
import numpy as np
import torch

from . import _lib as L
from ._lib import _stream
from . import engine as E
from . import modules as M


def eval_coeffs_model(gamma, beta, running_mean, running_var, eps=E.EPS):
    """rd_bn_eval_coeffs in numpy, float32 operation by float32 operation in the kernel's order:
    invstd = 1 / sqrt(running_var + eps); scale = gamma * invstd; shift = beta - running_mean * scale."""
    f32 = np.float32
    g, b, rm, rv = (np.asarray(t, dtype=f32) for t in (gamma, beta, running_mean, running_var))
    invstd = (f32(1) / np.sqrt((rv + f32(eps)).astype(f32)).astype(f32)).astype(f32)
    scale = (g * invstd).astype(f32)
    shift = (b - (rm * scale).astype(f32)).astype(f32)
    return scale, shift


def build_plan(bank, wpack, dtype, N, H, W, in_channels=3, n=16, num_classes=2, slope=0.0):
    """The frozen plan of (N, H, W) over modules 'enc' and 'dec' of `bank`.  Launches nothing (works on CPU tensors: the plan tests).
    Returns the plan with .x_in (the input Act) and .out (the logits Act).
    The input's channel stride is in_channels, as in the Encoder module's plan, NOT the 16-byte slot of the training step: the stride
    picks the first conv's kernel (csrc/conv_small_fwd.hip rd_route_small_fwd wants whole slots, `s.C % 8`; the unpadded image goes
    to conv_small_stage_kernel), and this plan's contract is the module path's arithmetic launch for launch, not a new tuning."""
    if H % 16 or W % 16:
        raise ValueError('EvalForward: H and W must be multiples of 16 (four 2x2 max-pools), got %dx%d' % (H, W))
    pl = E.Plan(bank, dtype, N, [0, N], slope=slope, training=False, frozen_bn=True)
    pl.x_in = E.Act(pl, N, H, W, in_channels, name='input')
    feats = E.build_encoder(pl, pl.x_in, n=n, mname='enc')
    pl.out = E.build_decoder(pl, feats, n=n, num_classes=num_classes, mname='dec')
    pl.build(wpack)
    return pl


def site_table(sites):
    """The rd_bn_eval_site_t rows of Plan.bn_sites as a ctypes array."""
    arr = (L.RdBnEvalSite * max(len(sites), 1))()
    for i, (g, b, rm, rv, sc, sh, Cc) in enumerate(sites):
        arr[i].gamma, arr[i].beta, arr[i].running_mean, arr[i].running_var = g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr()
        arr[i].scale, arr[i].shift, arr[i].C = sc.data_ptr(), sh.data_ptr(), int(Cc)
    return arr


class _Bound:
    """One built plan: the launch list, the device table of its BatchNorm sites."""

    def __init__(self, plan):
        self.plan = plan
        self.list = E.LaunchList(tuple(plan.fwd), ())
        self.n_sites = len(plan.bn_sites)
        self.max_c = max(s[6] for s in plan.bn_sites)
        raw = bytes(memoryview(site_table(plan.bn_sites)))
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(plan.device)     # complete when .to() returns (pageable source)

    def coeffs(self):
        L.check(L.lib().rd_bn_eval_coeffs(self.table.data_ptr(), self.n_sites, self.max_c, E.EPS, _stream()), 'rd_bn_eval_coeffs')


class EvalForward:
    """Encoder + Decoder forward with frozen BatchNorm as one launch list per batch geometry."""

    def __init__(self, bank, wpack, owns_pack, dtype, in_channels, n, num_classes, slope):
        if torch.device(bank.device).type != 'cuda':
            raise ValueError('EvalForward runs HIP kernels: the parameters must be on the GPU (there is no CPU fallback)')
        self.bank, self.wpack, self.owns_pack, self.dtype = bank, wpack, owns_pack, dtype
        self.dt = L.RD_BF16 if dtype == torch.bfloat16 else L.RD_F32
        self.c, self.n, self.k, self.slope = in_channels, n, num_classes, slope
        self._plans = {}

    # ---- construction
    @staticmethod
    def _check_modules(encoder, seg_decoder):
        for m, what in ((encoder, 'encoder'), (seg_decoder, 'seg_decoder')):
            if getattr(m, '_norm', None) != 'bn':
                raise ValueError('EvalForward covers BatchNorm networks (--norm bn): the %s has norm=%r (gn / in keep the statistics of the '
                                 'input itself: there is nothing to freeze)' % (what, getattr(m, '_norm', None)))
        if encoder._slope != seg_decoder._slope:
            raise ValueError('EvalForward: encoder and seg_decoder must share one activation')

    @classmethod
    def from_trainer(cls, fused_trainer, dtype=None):
        """Shares the trainer's parameter arena.  dtype: the storage dtype of the pass, default the module path's (modules.storage_dtype():
        what `seg_decoder(encoder(x))` would run in, so that validation gives the same bits with and without this class).  Where that
        is the trainer's own dtype the plans read ts.wpack and nothing is ever repacked: every step -- pipelined or not, single-GPU or
        data-parallel -- ends in segment C = [rd_adam_step, rd_pack_weights_batched] on the main stream behind the join of every lane
        (step.TrainStep._build_ops / step()), so once the step's stream is synchronised ts.wpack is the pack of the current
        parameters.  Otherwise (a bf16 step validated by fp32 modules: train.py's default) the object owns a pack in `dtype` and
        refresh() repacks once per pass."""
        ts = getattr(fused_trainer, 'ts', None)
        if ts is None or not hasattr(fused_trainer, 'bank'):
            raise ValueError('EvalForward.from_trainer needs a FusedTrainer (the fused step of --norm bn)')
        enc, dec = fused_trainer.modules['enc'], fused_trainer.modules['dec']
        cls._check_modules(enc, dec)
        dtype = M.storage_dtype() if dtype is None else dtype
        bank = fused_trainer.bank
        if dtype == ts.dtype:
            wpack, owns = ts.wpack, False
        else:
            wpack, owns = E.WeightPack(bank, [('enc', enc._specs), ('dec', dec._specs)], dtype), True
        return cls(bank, wpack, owns, dtype, enc._c, enc._n, dec._k, enc._slope)

    @classmethod
    def from_modules(cls, encoder, seg_decoder, dtype=None):
        """Binds both modules into ONE ParamBank (they keep working on their own: their tensors alias the arena) and owns a WeightPack
        that refresh() repacks.  dtype: default modules.storage_dtype()."""
        cls._check_modules(encoder, seg_decoder)
        p = next(encoder.parameters())
        if not (p.is_cuda and next(seg_decoder.parameters()).is_cuda):
            raise ValueError('EvalForward runs HIP kernels: the modules must be on the GPU (there is no CPU fallback)')
        dtype = M.storage_dtype() if dtype is None else dtype
        mods = [('enc', encoder._specs), ('dec', seg_decoder._specs)]
        bank = E.ParamBank(mods, p.device)
        encoder.bind(bank, 'enc', None)
        seg_decoder.bind(bank, 'dec', None)
        return cls(bank, E.WeightPack(bank, mods, dtype), True, dtype, encoder._c, encoder._n, seg_decoder._k, encoder._slope)

    # ---- plans
    def _bound(self, N, H, W):
        key = (int(N), int(H), int(W))
        b = self._plans.get(key)
        if b is None:
            b = self._plans[key] = _Bound(build_plan(self.bank, self.wpack, self.dtype, *key, in_channels=self.c, n=self.n,
                                                     num_classes=self.k, slope=self.slope))
            b.coeffs()                  # a geometry first met in the middle of a pass: the parameters are those of refresh()
        return b

    def refresh(self):
        """Once per pass, after the parameters or running statistics have changed: [the weight repack, where this object owns the pack]
        + ONE rd_bn_eval_coeffs per plan built so far.  On the current stream; nothing synchronises."""
        if self.owns_pack:
            self.wpack.refresh(_stream())
        for b in self._plans.values():
            b.coeffs()

    def input(self, N, H, W):
        """The NHWC storage-dtype input tensor [N][H][W][cstride] of the (N, H, W) plan, to be filled in place (cstride = its last
        dimension; a channel past in_channels would be padding and must stay zero)."""
        return self._bound(N, H, W).plan.x_in.buf

    def run(self, N, H, W):
        """ONE rd_run_list call on the current stream.  Returns the plan-owned NHWC storage-dtype logits [N][H][W][num_classes]."""
        b = self._bound(N, H, W)
        b.list.run(torch.cuda.current_stream(), {})
        return b.plan.out.buf

    def logits_nchw(self, N, H, W):
        """fp32 NCHW copy of the logits of the last run() through rd_nhwc_to_nchw (what the Decoder module returns): tests, debugging."""
        pl = self._bound(N, H, W).plan
        return M.materialize(pl.out, pl)

    def launches(self, N, H, W):
        """Launch counts of one batch by entry point (scripts/fused_val_bench.py)."""
        out = {}
        for op in self._bound(N, H, W).plan.fwd:
            out[op[0].__name__] = out.get(op[0].__name__, 0) + 1
        return out
