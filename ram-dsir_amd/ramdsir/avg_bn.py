"""BatchNorm re-estimation of the averaged model (train.py --avg_bn_recal K; rd_bn_recal, csrc/bn_recal.hip): at the end of an epoch
the running statistics of the averaged encoder and seg decoder are re-estimated from the last K training batches of that epoch, with
the semantics of torch.optim.swa_utils.update_bn and momentum=None -- every batch is normalised by its own batch statistics,
running_mean is the running mean of the batch means, running_var the running mean of the unbiased batch variances,
num_batches_tracked = K.  The mean of running statistics collected under many weight vectors (what rd_avg_step leaves in the averaged
bank) is not the statistics of the activations the averaged weights produce; this pass measures those.  No reference counterpart.

    BatchRing        K device copies of the clean half (img, not img_freq) of the step's input, taken behind the last K steps of an epoch
    RecalBank        a third set of buffers: the averaged bank's parameter arena, clones of its encoder / seg-decoder BatchNorm buffers
    RecalForward     encoder + seg decoder as one forward launch list with batch statistics (engine.Plan recal_bn) over the averaged
                     weights, and ONE rd_bn_recal launch per batch behind it -- the counterpart of infer.EvalForward
    BnRecal          the three of them on a FusedTrainer (FusedTrainer.enable_avg_bn_recal): capture(), run_pass(), eval_forward(),
                     state_dicts()
    model(...)       the numpy model of the kernel: bit for bit

The training is bit-identical with and without it: the capture is a device-to-device copy behind the step that only reads the step's
input, and the pass writes the RecalBank's own buffers.  rd_avg_step keeps averaging the averaged bank's buffers undisturbed, and they
are what a training-state snapshot holds; nothing of the ring is snapshotted (every epoch's pass uses that epoch's own batches).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import engine as E
from . import range_table as R


# ------------------------------------------------------------------------------------------------ the numpy model of the kernel
def slot_sums_model(slots, nslots=L.STAT_SLOTS):
    """csrc/bn_fin.h slot_sums on one statistics group: slots [RD_STAT_SLOTS][C][2] float64 -> (s1, s2) [C] float64, the first
    `nslots` copies added one after the other in slot order."""
    slots = np.asarray(slots, np.float64)
    s1, s2 = np.zeros(slots.shape[1], np.float64), np.zeros(slots.shape[1], np.float64)
    with np.errstate(all='ignore'):
        for k in range(int(nslots)):
            s1 = s1 + slots[k, :, 0]
            s2 = s2 + slots[k, :, 1]
    return s1, s2


def fwd_stat_model(s1, s2, count, conv_bias=None, with_var=False):
    """csrc/bn_fin.h fwd_stat, operation by operation (contraction off): (mean, unb) float32 [C].
    m0 = s1 / count; var = max(s2 / count - m0 * m0, 0) in float64; mean = float32(m0 + conv_bias);
    unb = float32(var * count / (count - 1)) for count > 1, float32(var) otherwise.  count is the float32 the kernel receives.
    with_var: (mean, unb, float32(var)) -- the biased variance that invstd is taken from (tests/bn_fin_model.py)."""
    f32, f64 = np.float32, np.float64
    s1, s2 = np.asarray(s1, f64), np.asarray(s2, f64)
    cnt = f64(f32(count))
    cb = np.zeros(s1.shape, f32) if conv_bias is None else np.asarray(conv_bias, f32)
    with np.errstate(all='ignore'):
        m0 = s1 / cnt
        sq = m0 * m0
        vard = s2 / cnt - sq
        vard = np.where(vard < 0.0, 0.0, vard)
        mean = (m0 + cb.astype(f64)).astype(f32)
        unb = ((vard * cnt) / (cnt - 1.0)).astype(f32) if cnt > 1.0 else vard.astype(f32)
        var = vard.astype(f32)
    return (mean, unb, var) if with_var else (mean, unb)


def update_model(run, x, k):
    """The cumulative average of rd_bn_recal on one vector: k == 0 the batch value (the old content is not read); k > 0:
    d = x - run; t = w * d; run + t with w = float32(1) / float32(k + 1) -- three float32 operations, each rounded on its own."""
    f32 = np.float32
    x = np.asarray(x, f32)
    if int(k) == 0:
        return x.copy()
    run = np.asarray(run, f32)
    w = f32(1) / f32(int(k) + 1)
    with np.errstate(all='ignore'):
        d = (x - run).astype(f32)
        t = (w * d).astype(f32)
        return (run + t).astype(f32)


def model(running_mean, running_var, slots, count, conv_bias, k, nslots=L.STAT_SLOTS):
    """rd_bn_recal on one site, in numpy: (running_mean, running_var, num_batches_tracked) behind batch k.  slots: the site's
    statistic slots [RD_STAT_SLOTS][C][2] float64 as the forward list left them; conv_bias: [C] or None."""
    s1, s2 = slot_sums_model(slots, nslots)
    mean, unb = fwd_stat_model(s1, s2, count, conv_bias)
    return update_model(running_mean, mean, k), update_model(running_var, unb, k), np.int64(int(k) + 1)


# ------------------------------------------------------------------------------------------------ the kernel's table
def site_table(sites):
    """The rd_bn_recal_site_t rows of Plan.recal_sites as a ctypes array."""
    arr = (L.RdBnRecalSite * max(len(sites), 1))()
    for r, (stats, cbias, rm, rv, nbt, count, Cc, nslots, _) in zip(arr, sites):
        r.stats, r.conv_bias = stats, cbias
        r.running_mean, r.running_var, r.num_batches_tracked = rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()
        r.count, r.C, r.nslots = float(count), int(Cc), int(nslots)
    return arr


upload_table = R.upload


def run(arr, table_dev, n, max_c, k, eps=E.EPS, stream=None):
    """One rd_bn_recal call; returns its code (0, or the negative validation code: nothing was launched)."""
    return L.lib().rd_bn_recal(arr, table_dev.data_ptr() if table_dev is not None else None, n, max_c, int(k), float(eps), R.stream_handle(stream))


# ------------------------------------------------------------------------------------------------ the plan
def build_plan(bank, wpack, dtype, N, H, W, in_channels=3, n=16, num_classes=2, slope=0.0):
    """The re-estimation plan of (N, H, W) over modules 'enc' and 'dec' of `bank`.  Launches nothing (works on CPU tensors: the plan
    tests).  Returns the plan with .x_in (the input Act) and .out (the logits Act).  The input's channel stride is in_channels, as in
    the Encoder module's plan and in infer.build_plan: every conv takes the route it takes when the drop-in modules run in training
    mode."""
    if H % 16 or W % 16:
        raise ValueError('RecalForward: H and W must be multiples of 16 (four 2x2 max-pools), got %dx%d' % (H, W))
    pl = E.Plan(bank, dtype, N, [0, N], slope=slope, training=True, fused_step=False, recal_bn=True)
    pl.x_in = E.Act(pl, N, H, W, in_channels, name='input')
    feats = E.build_encoder(pl, pl.x_in, n=n, mname='enc')
    pl.out = E.build_decoder(pl, feats, n=n, num_classes=num_classes, mname='dec')
    pl.build(wpack)
    return pl


class RecalBank(E.ParamBank):
    """The third set of buffers: the averaged bank's layout and PARAMETER ARENA (shared, never written here) with clones of the
    BatchNorm buffers of `modules` (encoder and seg decoder) that the re-estimation pass writes; the buffers of every other module
    (the restoration decoder's DSBN, which takes no part in inference) are the averaged bank's own tensors."""

    def __init__(self, avg_bank, modules=('enc', 'dec')):
        self.device, self.index, self.module_range, self.n = avg_bank.device, avg_bank.index, avg_bank.module_range, avg_bank.n
        self.params = avg_bank.params
        self.grads = self.exp_avg = self.exp_avg_sq = None
        self.recal_modules = tuple(modules)
        self.buffers = {k: (t.detach().clone() if k[0] in self.recal_modules else t) for k, t in avg_bank.buffers.items()}


class RecalForward:
    """Encoder + seg decoder forward with batch statistics over `bank` as one launch list, and one rd_bn_recal launch per batch that
    folds the statistic slots of all BatchNorm sites into the cumulative average held in the bank's running statistics."""

    def __init__(self, bank, wpack, dtype, N, H, W, in_channels=3, n=16, num_classes=2, slope=0.0):
        if torch.device(bank.device).type != 'cuda':
            raise ValueError('RecalForward runs HIP kernels: the parameters must be on the GPU (there is no CPU fallback)')
        self.bank, self.wpack, self.dtype = bank, wpack, dtype
        self.plan = build_plan(bank, wpack, dtype, N, H, W, in_channels, n, num_classes, slope)
        self.list = E.LaunchList(tuple(self.plan.fwd), ())
        self.sites = self.plan.recal_sites
        self.n_sites, self.max_c = len(self.sites), max(s[6] for s in self.sites)
        self.arr = site_table(self.sites)
        self.table_dev = upload_table(self.arr, self.n_sites, bank.device)       # once: the pointers never move

    def input(self):
        """The NHWC storage-dtype input [N][H][W][in_channels] of the plan, to be filled in place."""
        return self.plan.x_in.buf

    def run(self, k):
        """Batch k of a pass on the current stream: the statistic slots zeroed, ONE rd_run_list call, ONE rd_bn_recal launch."""
        self.plan.stat_arena.zero_()
        self.list.run(torch.cuda.current_stream(), {})
        L.check(run(self.arr, self.table_dev, self.n_sites, self.max_c, k), 'rd_bn_recal')

    def slots(self, i):
        """Site i's statistic slots [RD_STAT_SLOTS][C][2] float64 as the last forward left them (a view of the plan's arena)."""
        o = self.sites[i][8]
        off = self.plan._stat_off[o.stats[1]]
        return self.plan.stat_arena[off:off + L.STAT_SLOTS * o.C * 2].view(L.STAT_SLOTS, o.C, 2)

    def launches(self):
        """Launch counts of one batch by entry point."""
        out = {'rd_bn_recal': 1}
        for op in self.plan.fwd:
            out[op[0].__name__] = out.get(op[0].__name__, 0) + 1
        return out


def ring_bytes(K, B, H, W, cstride, elemsize):
    return int(K) * int(B) * int(H) * int(W) * int(cstride) * int(elemsize)


def _check_memory(nbytes, K, device):
    """As gpu_data._check_memory: the ring against free device memory, with a message."""
    free, total = torch.cuda.mem_get_info(device)
    if nbytes > free:
        raise RuntimeError('--avg_bn_recal %d: the ring of %d captured batches needs %.2f GB of device memory, %.2f GB of %.2f GB are free '
                           '(use a smaller K)' % (K, K, nbytes / 1e9, free / 1e9, total / 1e9))


class BatchRing:
    """K entries [B][H][W][cstride] in the step's storage dtype: the clean half (the first B images: img, not img_freq) of
    TrainStep.xbufs[slot] as it lies there, padded channel slot included.  One contiguous device-to-device copy per captured step."""

    def __init__(self, ts, K):
        x = ts.xbufs[0]
        self.K, self.B = int(K), ts.B
        _check_memory(ring_bytes(K, ts.B, x.shape[1], x.shape[2], x.shape[3], x.element_size()), self.K, x.device)
        self.buf = torch.zeros((self.K, ts.B) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        self.count = 0

    def begin_epoch(self):
        self.count = 0

    def capture(self, ts, slot):
        """Behind the step that trained on `slot`, on the current stream: the next entry."""
        if self.count >= self.K:
            raise RuntimeError('BatchRing: %d batches captured in one epoch, the ring holds %d' % (self.count + 1, self.K))
        self.buf[self.count].copy_(ts.xbufs[slot][:self.B])
        self.count += 1


class BnRecal:
    """--avg_bn_recal on a FusedTrainer with an averaged model: the ring, the RecalBank, the pass."""

    def __init__(self, trainer, avg, K):
        K = check_k(K)
        if K < 1:
            raise ValueError('avg_bn_recal: K = %d (0 switches the pass off: construct nothing)' % K)
        enc, dec = trainer.modules['enc'], trainer.modules['dec']
        from . import infer
        infer.EvalForward._check_modules(enc, dec)
        self.trainer, self.avg, self.K = trainer, avg, K
        ts = trainer.ts
        self.ring = BatchRing(ts, K)
        self.bank = RecalBank(avg.bank)
        self._mods = [('enc', enc._specs), ('dec', dec._specs)]
        self._geom = (enc._c, enc._n, dec._k, enc._slope)
        self._packs, self._forward = {}, {}
        self.forward = RecalForward(self.bank, self.pack(ts.dtype), ts.dtype, ts.B, ts.H, ts.W, *self._geom)

    def pack(self, dtype):
        """The weight pack of the averaged encoder / seg decoder in `dtype`: one per dtype, shared by the pass and the fused
        validation forward where their dtypes agree."""
        if dtype not in self._packs:
            self._packs[dtype] = E.WeightPack(self.bank, self._mods, dtype)
        return self._packs[dtype]

    def settings(self):
        return self.K

    # ---- the capture
    def begin_epoch(self):
        self.ring.begin_epoch()

    def capture(self, slot):
        """The after-step hook's part (FusedTrainer._arm_after_step): one copy on the step's stream behind the step."""
        self.ring.capture(self.trainer.ts, slot)

    # ---- the pass
    def run_pass(self):
        """Re-estimate from the batches captured in this epoch, on the current stream: one repack of the averaged weights, then per
        batch one copy into the plan's input, the forward list and rd_bn_recal.  Returns the number of batches (0: nothing captured,
        nothing done)."""
        fwd, n = self.forward, self.ring.count
        if n == 0:
            return 0
        with torch.no_grad():
            fwd.wpack.refresh(L._stream())
            x, c = fwd.input(), self._geom[0]
            for k in range(n):
                x.copy_(self.ring.buf[k][..., :c])
                fwd.run(k)
        return n

    # ---- what reads the result
    def eval_forward(self, dtype=None):
        """infer.EvalForward over the RecalBank (avg.WeightAverage.eval_forward's counterpart): the averaged weights, the re-estimated
        statistics.  Its refresh() repacks and recomputes the frozen coefficients once per pass."""
        from . import infer, modules as M
        dtype = M.storage_dtype() if dtype is None else dtype
        f = self._forward.get(dtype)
        if f is None:
            f = self._forward[dtype] = infer.EvalForward(self.bank, self.pack(dtype), True, dtype, *self._geom)
        return f

    def state_dicts(self):
        """avg.WeightAverage.state_dicts() with the encoder / seg-decoder BatchNorm buffers of the RecalBank: the same keys and order."""
        from .ckpt import MODULE_KEYS
        from .step import state_dict_of
        return OrderedDict((key, state_dict_of(self.bank, m, self.trainer.modules[m]._specs)) for m, key in MODULE_KEYS)


def check_k(K):
    if isinstance(K, bool) or int(K) != K or int(K) < 0:
        raise ValueError('avg_bn_recal takes a number of batches (0 = off), got %r' % (K,))
    return int(K)
