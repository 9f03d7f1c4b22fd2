"""Glue between the drop-in nn.Modules and the fused HIP training step: puts the three modules into ONE
parameter arena (encoder first: Adam's lr/2 group, code/train.py:573), builds the TrainStep for the batch
geometry and (multi-GPU) wraps it with the bucketed RCCL gradient exchange.  The step is launched eagerly over three
HIP streams (step.TrainStep.lanes; the host enqueues a step in ~1.4 ms against ~7 ms of GPU time); use_graph=True
replays one captured hipGraph per step instead (no host work per step, but slower on ROCm 7: DESIGN.md section 3)."""
import torch
import torch.distributed as dist

from . import engine as E
from . import step as S
from . import ddp as D


class FusedTrainer:
    def __init__(self, encoder, seg_decoder, rec_decoder, batch_sizes, H, W, dataset='fundus', consistency='kd', lambda_rec=0.1,
                 lr=2e-3, total_iters=1, dtype=torch.bfloat16, use_graph=False, device=None):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        self.modules = dict(enc=encoder, dec=seg_decoder, rec=rec_decoder)
        mods = [('enc', encoder._specs), ('dec', seg_decoder._specs), ('rec', rec_decoder._specs)]
        self.bank = E.ParamBank(mods, dev)
        for name, m in self.modules.items():
            m.bind(self.bank, name, None)
        slope = encoder._slope
        self.ts = S.TrainStep(self.bank, mods, dtype, batch_sizes, H, W, dataset=dataset, consistency=consistency,
                              lambda_rec=lambda_rec, lr=lr, total_iters=total_iters, in_channels=encoder._c, n=encoder._n,
                              num_classes=seg_decoder._k, slope=slope, ram='u8' if dataset == 'fundus' else True,
                              # a captured graph replays one chain: no lane to leave compute units to (tuning.py)
                              options=dict(side_cus=0, rec_cus=0) if use_graph else None)
        self.ts.wpack.refresh()
        self._primed, self._graphs, self._announced = False, bool(use_graph), None
        self._tb, self._tb_pending, self._tb_hook, self._log, self._avg, self._guard = None, None, None, None, None, None
        self._optim = None
        self._accum = None
        self._bn_recal, self._bn_capture = None, False
        self._hist, self._hist_armed, self._hist_pending = None, None, None
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        if self.world > 1:
            # identical initial weights on every rank (DataParallel broadcasts replica 0's, train.py:205-208)
            dist.broadcast(self.bank.params, src=0)
            for b in self.bank.buffers.values():
                dist.broadcast(b, src=0)
            self.ts.wpack.refresh()
            self.runner = D.DataParallelStep(self.ts)
            if use_graph:
                self.runner.capture()
            self._step = self.runner.step
        else:
            if use_graph:
                self.ts.capture()
            self._step = self.ts.step

    def step(self, src_nhwc, trg_nhwc, lam, target, next_batch=None):
        """src/trg: NHWC images as the dataset holds them before RAM -- fundus: uint8 pixels 0..255 (the step is built with
        uint8 RAM buffers; float images are refused by TrainStep.load_raw), prostate: float32 in [-1,1];
        lam: [B]; target: fundus (B,2,H,W) float multilabel mask / prostate (B,H,W) int64.
        next_batch = (src, trg, lam, target) of the FOLLOWING step, if the caller has it: its images go into the other input slot now
        and are mixed (RAM) in this step's tail, beside Adam and the weight repack, instead of opening the next step alone
        (step.TrainStep.load_raw_next); the next call's first four arguments are then ignored -- that batch is already on the
        device.  Not with captured graphs (they replay the classical step)."""
        if not self._primed:
            self.ts.load_raw(src_nhwc, trg_nhwc, lam)
            self.ts.load_target(target)
        elif not all(a is b for a, b in zip((src_nhwc, trg_nhwc, lam, target), self._announced)):
            # the previous call uploaded `next_batch` and this step trains on THAT: a caller that now passes other tensors would
            # silently train on the wrong data
            raise ValueError('FusedTrainer.step: the previous call announced next_batch; this call must pass the same tensors '
                             '(src, trg, lam, target) as its current batch')
        pipelined = next_batch is not None and not self._graphs
        if pipelined:
            self.ts.load_raw_next(*next_batch[:3])
        self._arm_after_step()
        self._step()
        if pipelined:
            self.ts.load_target(next_batch[3])            # after the step has been enqueued: its loss still reads the current mask
        self._primed = pipelined
        self._announced = tuple(next_batch[:4]) if pipelined else None

    def _refuse_graphs(self, what):
        if self._graphs:
            raise RuntimeError('%s: a captured hipGraph replays a fixed launch list (use_graph=True)' % what)

    def stages(self):
        """(avg, guard, optim, accum): what enable_avg_weights, enable_grad_guard, enable_optim and enable_grad_accum have returned,
        None where one is off -- in the order their records and ranges go into a training-state snapshot (train.py open_state)."""
        return self._avg, self._guard, self._optim, self._accum

    def arm_tb_images(self):
        """The next step() also composes the TensorBoard image grids of ITS batch (ramdsir/tb_images.py; code/train.py:306-329,
        475-496) and starts their copy to pinned host memory; take_tb_images() then returns the pending result.  The compose is
        enqueued behind the step's last launch and in front of the upload of the next mask (TrainStep.arm_after_step), reads the
        input slot the step trained on, and only reads: training is bit-identical with and without it.  Not with use_graph=True."""
        self._refuse_graphs('arm_tb_images')
        from . import tb_images
        ts = self.ts
        if self._tb is None:
            self._tb = tb_images.GridComposer(ts.dataset, ts.B, ts.H, ts.W, ts.K, self.bank.device)

        def hook(slot):
            self._tb_pending = self._tb.enqueue(tb_images.train_step_sources(ts, slot))
        self._tb_hook = hook

    def _arm_after_step(self):
        """TrainStep.arm_after_step holds ONE one-shot hook; the image grids (armed for single steps), the step log and the weight
        average (every step, once enabled) share it: one closure per step runs whichever of the three apply, in the order step log,
        averaging, image compose -- the two per-step launches of a few microseconds first, the compose and the start of its copy to
        the host last.  All three only read the step's buffers, so the order changes no result.  Nothing is armed when none applies.
        A step armed with arm_bn_capture() (--avg_bn_recal) joins them with one copy of its input, behind the averaging; a step armed
        with arm_tb_hist() (--tb_hist) ends the hook with the rd_hist call over the arenas and the start of its copy."""
        tb, self._tb_hook = self._tb_hook, None
        hist, self._hist_armed = self._hist_armed, None
        log, avg = self._log, self._avg
        cap, self._bn_capture = (self._bn_recal if self._bn_capture else None), False
        if avg is not None and self._accum is not None and not self._accum.next_is_boundary():
            avg = None                                      # rd_avg_step reads the counter, which moves at a window's last step only
        if tb is None and log is None and avg is None and cap is None and hist is None:
            return

        def hook(slot):
            if log is not None:
                log.append(torch.cuda.current_stream().cuda_stream)
            if avg is not None:
                avg.enqueue(torch.cuda.current_stream().cuda_stream)
            if cap is not None:
                cap.capture(slot)                           # --avg_bn_recal: the clean half of the step's input into the ring
            if tb is not None:
                tb(slot)
            if hist is not None:
                self._hist_pending = self._hist.enqueue(torch.cuda.current_stream().cuda_stream, copy=hist == 'copy')
        self.ts.arm_after_step(hook)

    def enable_tb_hist(self, what=('weights', 'grads')):
        """Builds the histogram state of train.py --tb_hist (ramdsir/tb_hist.py): the range table over every parameter tensor of the
        arenas named in `what` (weights, grads, adam_m, adam_v), the uploaded bucket limits, the device output, the workspace.  Nothing
        runs until a step is armed with arm_tb_hist().  Only reads the arenas: training is bit-identical with and without it.  Returns
        the tb_hist.TbHist.  Not with use_graph=True."""
        if self._graphs:
            self.ts.refuse_fixed_list('enable_tb_hist', ['the per-tensor histograms behind the step (rd_hist)'])
        from . import tb_hist
        self._hist = tb_hist.TbHist(self.bank, what)
        return self._hist

    def arm_tb_hist(self, copy=True):
        """The next step() is followed by ONE rd_hist call on the main stream -- behind the whole tail (Adam, repack, guard sync, the
        weight average), in front of the upload of the next mask: `grads` still holds this step's gradient (the one the step log's
        health pass reads), `params` and the moments are the updated ones -- and, with copy, by the copy of its result to pinned host
        memory; take_tb_hist() then returns the pending result.  A data-parallel rank that does not write passes copy=False: the
        launch runs (every rank enqueues the same step), nothing is copied.  A step that is not armed runs no launch and no call."""
        self._refuse_graphs('arm_tb_hist')
        if self._hist is None:
            raise RuntimeError('arm_tb_hist: enable_tb_hist() first')
        self._hist_armed = 'copy' if copy else 'launch'

    def take_tb_hist(self):
        """The tb_hist.Pending of the last armed step (its fetch() waits for the copy), once."""
        pending, self._hist_pending = self._hist_pending, None
        if pending is None:
            raise RuntimeError('take_tb_hist: no armed step (with copy) has run')
        return pending

    def enable_avg_bn_recal(self, K):
        """BatchNorm re-estimation of the averaged model (ramdsir/avg_bn.py; needs enable_avg_weights first): a device ring of K
        batches, a third set of encoder / seg-decoder BatchNorm buffers and a forward-only plan with batch statistics over the averaged
        weights.  arm_bn_capture() makes the next step() copy the clean half of its input into the ring -- one device-to-device copy
        behind the step through the one after-step hook, beside the step log, the averaging and the image grids; the returned
        avg_bn.BnRecal's run_pass() re-estimates from what an epoch captured.  Only reads the trainer's buffers: training and the
        averaged bank are bit-identical with and without it.  K == 0 constructs nothing and returns None.  Not with use_graph=True."""
        from . import avg_bn
        K = avg_bn.check_k(K)
        self._refuse_graphs('enable_avg_bn_recal')
        if K == 0:
            return None
        if self._avg is None:
            raise RuntimeError('enable_avg_bn_recal: the pass re-estimates the averaged model (enable_avg_weights first)')
        self._bn_recal = avg_bn.BnRecal(self, self._avg, K)
        self._avg.bn_recal = self._bn_recal
        return self._bn_recal

    def arm_bn_capture(self):
        """The next step() also copies the first B images of its input slot into the ring of enable_avg_bn_recal."""
        self._refuse_graphs('arm_bn_capture')
        if self._bn_recal is None:
            raise RuntimeError('arm_bn_capture: enable_avg_bn_recal() first')
        self._bn_capture = True

    def enable_avg_weights(self, mode='ema', decay=0.999, start=0):
        """From now on every step() is followed by one rd_avg_step launch (ramdsir/avg.py) that moves a second copy of the model -- the
        parameter arena and every BatchNorm buffer, initialised HERE as a copy of the live ones -- towards the live model: an exponential
        moving average (mode 'ema', `decay`) or the uniform average of the iterates behind iteration `start` ('uniform').  The launch
        sits on the main stream behind the step's last launch (TrainStep.arm_after_step), reads the device-side iteration counter
        itself and only reads the trainer's buffers: training is bit-identical with and without it.  Data parallel: rank-local, no
        collective.  Returns the avg.WeightAverage.  Not with use_graph=True."""
        self._refuse_graphs('enable_avg_weights')
        from . import avg
        self._avg = avg.WeightAverage(self, mode, decay, start)
        return self._avg

    def enable_grad_guard(self, max_norm=0.0):
        """From now on every step() runs the guarded tail (ramdsir/guard.py) in place of Adam + repack: the global gradient norm of the
        whole arena, Adam on the gradient scaled by min(1, max_norm / (norm + 1e-6)) (max_norm 0: no clipping), and a step whose
        gradient is not finite leaves parameters, moments and every BatchNorm buffer as they were (the shadow copies are initialised
        HERE from the live buffers).  Decided on the device, no read-back.  The after-step launches (step log, averaging, image grids)
        run behind the guarded tail as behind Adam; the gradient arena is never modified.  Returns the guard.GradGuard.  Not with
        use_graph=True."""
        self._refuse_graphs('enable_grad_guard')
        from . import guard
        self._guard = guard.GradGuard(self, max_norm)
        self.ts.enable_grad_guard(self._guard)
        return self._guard

    def enable_optim(self, weight_decay=0.0, wd_mode='decoupled', lr_schedule='poly', warmup_iters=0, enc_lr_mult=0.5):
        """From now on every step() runs the grouped Adam (ramdsir/optim.py, rd_optim_step) in place of rd_adam_step: the arena as a
        device table of ranges, each with its learning-rate multiplier (enc_lr_mult inside the encoder, 1 elsewhere) and its weight
        decay (weight_decay on tensors with more than one dimension -- the conv kernels; biases and BatchNorm weight / bias are
        exempt), decoupled (AdamW) or L2 (Adam(weight_decay)); the schedule (poly with the reference's lag, cosine, constant) and a
        linear warm-up are evaluated on the device from the counter.  The default values give the reference's optimizer, bit for
        bit.  Counter, schedule words and lr() are rd_adam_step's; with enable_grad_guard (in either order) the step's tail
        (TrainStep.enqueue_tail) calls it under the guard's state word.  Returns the optim.GroupedAdam.  Not with use_graph=True."""
        self._refuse_graphs('enable_optim')
        from . import optim
        self._optim = optim.GroupedAdam(self, weight_decay, wd_mode, lr_schedule, warmup_iters, enc_lr_mult)
        self.ts.enable_optim(self._optim)
        return self._optim

    def enable_grad_accum(self, steps):
        """From now on every step() runs forward, losses and backward as ever and is followed by one rd_grad_accum launch
        (ramdsir/accum.py); the optimizer tail -- rd_adam_step + repack, the guarded tail or the grouped Adam, whichever is enabled,
        in either order with this call -- runs behind every `steps`-th step only, on the mean of the window's gradients.  The device
        iteration counter, the schedule (`total_iters` is a number of UPDATES), the bias corrections and the start of
        enable_avg_weights count updates; the weight average moves at a window's last step only; BatchNorm moves its running
        statistics at every step, and a window the guard skips rolls them back over all of its forward passes.  losses() and lr()
        report the current micro-batch's losses and the last update's rate.  steps == 1 constructs nothing and returns None.  Not
        with use_graph=True, not data parallel."""
        from . import accum
        steps = accum.check_steps(steps)
        self._refuse_graphs('enable_grad_accum')
        if self.world > 1:
            raise RuntimeError('enable_grad_accum: gradient accumulation runs in one process (the bucketed gradient exchange of %d ranks '
                               'is tied to the segments of the step)' % self.world)
        if steps == 1:
            return None
        acc = accum.GradAccum(self, steps)
        self.ts.enable_grad_accum(acc)                      # (refuses a captured step: nothing is left half-enabled)
        self._accum = acc
        return acc

    def enable_step_log(self, health=False, rows=256):
        """From now on every step() appends one row to a device-resident ring (ramdsir/step_log.py, rd_step_log): the losses, the lr and
        the iteration number of the step and, with health=True, the gradient norm of each of the three Adam groups (code/train.py:573-576)
        and the number of non-finite gradient elements.  The row is written on the main stream behind the step's last launch -- behind
        the join of all lanes, Adam and the repack, in front of the upload of the next mask (TrainStep.arm_after_step) -- and only
        reads the step's buffers: training is bit-identical with and without it.  drain_step_log() returns the records.  Not with
        use_graph=True."""
        self._refuse_graphs('enable_step_log')
        from . import step_log
        ts, b = self.ts, self.bank
        r = [b.module_range['enc'][0], b.module_range['enc'][1], b.module_range['dec'][1], b.module_range['rec'][1]]
        assert b.module_range['dec'][0] == r[1] and b.module_range['rec'][0] == r[2]
        self._log = step_log.StepLog(ts.losses, ts.rec_mse, ts.hyper, b.grads if health else None, r if health else None, rows=rows)
        return self._log

    def step_log_full(self):
        return self._log is not None and self._log.full()

    def drain_step_log(self):
        """The records of the steps since the last drain, oldest first: {iteration, losses (the dict of losses()), lr, norms, nonfinite}.
        Synchronises.  Data parallel: collective, the loss columns are the mean over the ranks (what losses() returns for one step)."""
        if self._log is None:
            raise RuntimeError('drain_step_log: enable_step_log() first')
        return self._log.drain(self.ts.dataset, self.ts.lambda_rec, world=self.world)

    def take_tb_images(self):
        """The tb_images.Pending of the last armed step (its images() waits for the copy), once."""
        pending, self._tb_pending = self._tb_pending, None
        if pending is None:
            raise RuntimeError('take_tb_images: no armed step has run')
        return pending

    def losses(self):
        """The five loss terms + per-domain rec losses (names of the tensorboard scalars, train.py:298-304).  Data parallel:
        the MEAN over the ranks (every rank must call this; one small all-reduce at logging time)."""
        if self.world > 1:
            buf = torch.cat([self.ts.losses, self.ts.rec_mse])
            dist.all_reduce(buf)
            buf /= self.world
            keep = self.ts.losses.clone(), self.ts.rec_mse.clone()
            self.ts.losses.copy_(buf[:self.ts.losses.numel()])
            self.ts.rec_mse.copy_(buf[self.ts.losses.numel():])
            out = self.ts.loss_dict()
            self.ts.losses.copy_(keep[0])
            self.ts.rec_mse.copy_(keep[1])
            return out
        return self.ts.loss_dict()

    def lr(self):
        return float(self.ts.hyper[0])


class ModuleTrainer:
    """The reference's own training step (code/train.py:246-296 fundus, 412-465 prostate) over the drop-in modules of networks/unet.py
    -- torch autograd between the modules, torch's losses and torch.optim.Adam, the poly schedule of train.py:289-293 -- with the
    FusedTrainer interface.  train.py takes this path for --norm gn / in: the fused step keeps the statistics groups of the shared
    BatchNorms and of the restoration decoder's DSBN in one launch list and implements `bn` only, the modules implement all of
    normalization().  The convolutions / normalisations are the HIP launch lists of the modules, RAM is rd_ram_mix; single process."""

    def __init__(self, encoder, seg_decoder, rec_decoder, batch_sizes, H, W, dataset='fundus', consistency='kd', lambda_rec=0.1,
                 lr=2e-3, total_iters=1, dtype=torch.bfloat16, **_):
        if dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError('norm gn / in: the module-level training loop runs in one process (no gradient exchange)')
        from torch.optim import Adam
        self.enc, self.dec, self.rec = encoder, seg_decoder, rec_decoder
        self.bs, self.dataset, self.cons, self.lambda_rec = list(batch_sizes), dataset, consistency, lambda_rec
        self.base_lr, self.total_iters, self.iter_num = lr, total_iters, 0
        self.num_classes = seg_decoder._k
        self.opt = Adam([{'params': encoder.parameters(), 'lr': lr / 2}, {'params': seg_decoder.parameters(), 'lr': lr},
                         {'params': rec_decoder.parameters(), 'lr': lr}], lr=lr, betas=(0.9, 0.999))                 # train.py:573-576
        self._last = None
        # the modules' activation storage follows `dtype` (the default of train.py --dtype is bf16; the RAMDSIR_DTYPE environment default
        # of the module path is fp32: without this the flag was silently ignored here)
        from . import modules as M
        M.set_storage_dtype(dtype)
        self.dtype = dtype
        # ONE RAM plan (twiddles, workspace, the two output tensors), bound per step: the geometry is fixed
        from .ram import RamMixer
        B = sum(self.bs)
        dev = next(encoder.parameters()).device
        self._ram = RamMixer(B, H, W, torch.float32, dev, dataset)
        self._ram_out = (torch.empty(B, H, W, 3, dtype=torch.float32, device=dev), torch.empty(B, H, W, 3, dtype=torch.float32, device=dev))
        self._geom, self._tb, self._tb_armed, self._tb_pending = (B, H, W, dev), None, False, None

    def arm_tb_images(self):
        """As FusedTrainer.arm_tb_images: the next step() hands the tensors it holds -- img, img_freq, the soft prediction of the first
        pass, the concatenated restored images, the target -- to rd_tb_grids (NCHW fp32, already transformed)."""
        from . import tb_images
        if self._tb is None:
            B, H, W, dev = self._geom
            self._tb = tb_images.GridComposer(self.dataset, B, H, W, self.num_classes, dev)
        self._tb_armed = True

    take_tb_images = FusedTrainer.take_tb_images

    def _mix(self, src_nhwc, trg_nhwc, lam):
        """(img, img_freq) NCHW fp32 in [-1, 1] (ram.source_to_target_freq_batch with the plan built once)."""
        if not (src_nhwc.dtype == torch.uint8 and trg_nhwc.dtype == torch.uint8):
            src_nhwc, trg_nhwc = src_nhwc.float(), trg_nhwc.float()
        oi, of = self._ram_out
        self._ram.bind(src_nhwc.contiguous(), trg_nhwc.contiguous(), lam.float().contiguous(), oi, of)
        self._ram.run()
        return oi.permute(0, 3, 1, 2).contiguous(), of.permute(0, 3, 1, 2).contiguous()

    def step(self, src_nhwc, trg_nhwc, lam, target, next_batch=None):
        import torch.nn.functional as F
        from utils.losses import dice_loss, dice_loss_multi
        img, img_freq = self._mix(src_nhwc, trg_nhwc, lam)
        fundus = self.dataset == 'fundus'

        def seg(feats):
            logits = self.dec(feats)
            if fundus:
                soft = torch.sigmoid(logits)
                return soft, F.binary_cross_entropy(soft, target), dice_loss(soft, target)
            soft = torch.softmax(logits, dim=1)
            return soft, F.cross_entropy(logits, target), dice_loss_multi(soft, target, num_classes=self.num_classes, ignore_index=0)

        soft1, seg1, dice1 = seg(self.enc(img))
        feats2 = self.enc(img_freq)
        soft2, seg2, dice2 = seg(feats2)
        zero = torch.zeros((), device=img.device)
        if self.cons == 'kd':                                                                   # train.py:85-88 KD(pred_soft_2, pred_soft_1)
            consistency = F.kl_div(soft2.log(), soft1, reduction='mean') + F.kl_div(soft1.log(), soft2, reduction='mean')
        elif self.cons == 'mse':
            consistency = F.mse_loss(soft2, soft1)
        else:
            consistency = zero
        loss, left, rec_l, rec_imgs = 0, 0, [], []
        for d, b in enumerate(self.bs):                                                         # train.py:265-276
            rec_soft = torch.tanh(self.rec(feats2[-1][left:left + b], domain_label=d * torch.ones(b, dtype=torch.long)))
            l = F.mse_loss(rec_soft, img[left:left + b])
            loss = loss + self.lambda_rec * l
            rec_l.append(l)
            rec_imgs.append(rec_soft.detach())
            left += b
        loss = loss + seg1 + seg2 + dice1 + dice2 + 0.5 * consistency
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        lr = self.base_lr * (1 - self.iter_num / self.total_iters) ** 0.9                       # train.py:289-293
        self.opt.param_groups[0]['lr'], self.opt.param_groups[1]['lr'], self.opt.param_groups[2]['lr'] = lr / 2, lr, lr
        self.iter_num += 1
        self._last = (seg1, dice1, seg2, dice2, consistency, loss, rec_l)
        if self._tb_armed:
            from . import tb_images
            self._tb_armed = False
            self._tb_pending = self._tb.enqueue(tb_images.module_sources(img, img_freq, soft1.detach(), torch.cat(rec_imgs, 0), target))

    def losses(self):
        seg1, dice1, seg2, dice2, cons, loss, rec_l = self._last
        s = 'bce' if self.dataset == 'fundus' else 'ce'
        return {'loss_%s_1' % s: float(seg1), 'loss_dice_1': float(dice1), 'loss_%s_2' % s: float(seg2), 'loss_dice_2': float(dice2),
                'loss_consistency': float(cons), 'rec': [float(r) for r in rec_l], 'loss': float(loss)}

    def lr(self):
        return float(self.opt.param_groups[1]['lr'])
