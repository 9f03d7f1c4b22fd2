#!/usr/bin/env python3
"""Drop-in for the reference's code/train.py: same flags, same data layout, same checkpoint files, same
training semantics (code/train.py:195-361, 363-528, 530-601) -- on the fused HIP training step.

    python train.py --data_root ../dataset --dataset fundus --domain_idxs 1,2,3 --test_domain_idx 0 \\
                    --ram --rec --is_out_domain --consistency --consistency_type kd --save_path outdir/fundus/target0
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...      # data parallel (RCCL)

Differences, all deliberate: (i) RAM runs on the GPU per batch (the DataLoader workers only pick the partner
image and lambda); (ii) the step is a static launch list enqueued ahead of the GPU, so the five loss scalars are read every
--log_every iterations instead of forcing a device sync every iteration (train.py:298-304) -- and written, under the
reference's tags, to a TensorBoard event file in <save_path>/log (utils/tfevents.py: tensorboardX is not a dependency);
--tb_every_iter writes them at every iteration all the same, from a device-resident ring that is read at those iterations
(ramdsir/step_log.py), and --tb_health adds per-iteration gradient norms and a non-finite count through the same ring;
(iii) multi-GPU is one process per GPU with an RCCL gradient all-reduce instead of nn.DataParallel; (iv) the tensorboard image
grids (train.py:306-329, 475-496) are opt-in (--tb_images: composed on the GPU, ramdsir/tb_images.py) and the source-tree snapshot
(train.py:534-536) is not reproduced; (v) --ckpt_every N snapshots the whole training state (model, Adam moments, BatchNorm buffers,
schedule counter, host generators, the cycled loaders' replay lists) every N epochs through one HIP gather and a writer thread, --resume
continues from such a file -- bit-identically with --gpu_data or --num_workers 0 -- and --stop_after_epochs slices a run into jobs
(ramdsir/ckpt.py); the reference can only start from a fresh initialisation; (vi) --avg_weights ema | uniform keeps a second copy of
the model, averaged along the trajectory by one HIP launch behind every step (ramdsir/avg.py, rd_avg_step), validates it beside the live
one where --fused_val is in use (<target>_val_log_avg.csv, model_avg_%.2f.pth) and writes final_model_avg.pth, with
--avg_bn_recal K after re-estimating its BatchNorm statistics from the epoch's last K batches (ramdsir/avg_bn.py, rd_bn_recal); the
reference keeps the last iterate only; (vii) --clip_grad_norm X clips the gradient of the whole model by its global norm in front of Adam and
--skip_nonfinite makes a step with a non-finite gradient leave no trace in the model state (parameters, moments, BatchNorm buffers),
both decided on the device (ramdsir/guard.py: rd_grad_guard, rd_adam_step_guarded, rd_guard_sync); the reference steps on whatever
gradient it gets (code/train.py:285-287); (viii) --weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult replace the
reference's one hard-coded optimizer line (Adam without decay, lr / 2 on the encoder, poly; code/train.py:573-576, 289-293) by a grouped
Adam whose ranges, decay and schedule live on the device (ramdsir/optim.py, rd_optim_step); their defaults ARE that line; (ix)
--accum_steps N applies the optimizer at every N-th iteration, on the mean of the N micro-batch gradients (ramdsir/accum.py,
rd_grad_accum: one HIP launch per iteration into a second gradient arena) -- the effective batch is N times the reference's per-domain
tables (code/train.py:35-45), which stay as they are; the schedule counts updates, the loop counts iterations; (x) --tb_hist N writes
one TensorBoard histogram per parameter tensor of the weights and gradients (--tb_hist_what: also the two Adam moments) every N
iterations, counted by one HIP call over the arenas behind the step and written by the writer thread (ramdsir/tb_hist.py, rd_hist); the
reference writes scalars and images only (code/train.py:298-329).
"""
import argparse
import os
import os.path as osp
import random
import time
import sys
from itertools import cycle

HERE = osp.dirname(osp.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

import dataset.transform as trans
from dataset.fundus import Fundus_Multi, Fundus
from dataset.prostate import Prostate_Multi
from networks.unet import Encoder, Decoder, Rec_Decoder, count_params
from utils.metrics import postprocessing, dice_coeff_2label, post_and_dice
from utils.tfevents import SummaryWriter, QueuedWriter

fundus_batch_list = [[3, 6, 7], [2, 7, 7], [2, 4, 10], [2, 4, 10]]              # train.py:35-38
prostate_batch_list = [[2, 2, 2, 2, 2]] * 6                                       # train.py:40-45
AVG_DECAY = 0.999                                                                 # --avg_decay where it is not given


class Compose(object):
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, s):
        for t in self.ts:
            s = t(s)
        return s


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='DG Medical Segmentation Train')
    p.add_argument('--data_root', type=str, default='../dataset')
    p.add_argument('--dataset', type=str, default='fundus', choices=['fundus', 'prostate'])
    p.add_argument('--batch_size', type=int, default=8, help='parsed but unused, as in the reference (train.py:35-45)')
    p.add_argument('--test_batch_size', type=int, default=8)
    p.add_argument('--lr', type=float, default=None)
    p.add_argument('--epochs', type=int, default=None)
    p.add_argument('--domain_idxs', type=str, default='0,1,2')
    p.add_argument('--test_domain_idx', type=int, default=3)
    p.add_argument('--in_channels', type=int, default=3)
    p.add_argument('--num_classes', type=int, default=None)
    p.add_argument('--seed', type=int, default=1337)
    p.add_argument('--lambda_rec', type=float, default=0.1)
    p.add_argument('--deterministic', action='store_true')
    p.add_argument('--ram', action='store_true')
    p.add_argument('--rec', action='store_true')
    p.add_argument('--is_out_domain', action='store_true')
    p.add_argument('--consistency', action='store_true')
    p.add_argument('--consistency_type', type=str, default='mse')
    p.add_argument('--save_path', type=str, default=None, required=True)
    p.add_argument('--norm', type=str, default='bn')
    p.add_argument('--activation', type=str, default='relu')
    p.add_argument('--gpu', type=str, default='0')
    # additions
    p.add_argument('--dtype', type=str, default=None, choices=['bf16', 'f32'],
                   help='activation storage type; default: bf16 for the fused step (--norm bn), f32 for the module-level loop of --norm gn / in '
                        '(its modules are process-wide objects that validation shares: fp32 is their parity-grade mode)')
    p.add_argument('--log_every', type=int, default=20)
    p.add_argument('--num_workers', type=int, default=8)
    p.add_argument('--max_iters', type=int, default=None, help='stop early (smoke runs)')
    p.add_argument('--gpu_data', action='store_true',
                   help='decode the training images once and keep them in device memory; the augmentation runs as one HIP launch per '
                        'step (bit-identical to the host path with --num_workers 0, which then only sizes the preload thread pool)')
    p.add_argument('--gpu_val', action='store_true',
                   help='fundus: keep the held-out test set in device memory and run everything after the validation forward pass '
                        '(resize, threshold, largest component + hole filling, Dice counts) as HIP kernels; the reported numbers are '
                        'those of the host path')
    p.add_argument('--gpu_val_volumes', action='store_true',
                   help='prostate: keep the held-out site\'s volumes in device memory and build the 2.5-D batches, take the argmax, keep '
                        'the largest 3-D component and count for the Dice as HIP kernels; the reported numbers are those of the host path')
    p.add_argument('--fused_val', action='store_true',
                   help='with --gpu_val / --gpu_val_volumes (--norm bn): the validation forward pass as one HIP launch list per batch '
                        '(ramdsir/infer.py EvalForward) instead of the drop-in modules; the same masks, counts and CSV lines')
    p.add_argument('--tb_images', type=int, nargs='?', const=100, default=0, metavar='N',
                   help='also write the reference\'s TensorBoard image grids (input, RAM-mixed input, restored image, predictions, ground '
                        'truth) of rank 0\'s batch every N iterations (100 as in the reference when N is omitted), composed by one HIP '
                        'call from the step\'s buffers and encoded by a writer thread; off by default')
    p.add_argument('--tb_hist', type=int, nargs='?', const=100, default=0, metavar='N',
                   help='also write one TensorBoard histogram per parameter tensor (tags <kind>/<module>.<key>, TensorFlow\'s default '
                        'buckets) every N iterations (100 when N is omitted): one HIP call over the arenas behind the step (ramdsir/'
                        'tb_hist.py, rd_hist), one copy, trimmed and encoded by a writer thread; non-finite elements are left out and '
                        'reported as hist_nonfinite/<kind>; --norm bn only, not with --accum_steps; off by default')
    p.add_argument('--tb_hist_what', type=str, default=None, metavar='LIST',
                   help='with --tb_hist: a comma list over weights,grads,adam_m,adam_v (default weights,grads)')
    p.add_argument('--tb_every_iter', action='store_true',
                   help='write the seven TensorBoard scalars at EVERY iteration, as the reference does (train.py:298-304, 467-473), without a '
                        'host synchronisation per step: one small HIP launch behind each step appends them to a device-resident ring '
                        '(ramdsir/step_log.py) that is read at the --log_every iterations; --norm bn only; off by default')
    p.add_argument('--tb_health', action='store_true',
                   help='per iteration, through the same ring: the gradient norm of each Adam group (health/grad_norm_encoder, _seg_decoder, '
                        '_rec_decoder) and the number of non-finite gradient elements (health/nonfinite_grads); one console line names the '
                        'first iteration with non-finite losses or gradients; --norm bn only; off by default')
    p.add_argument('--ckpt_every', type=int, default=0, metavar='N',
                   help='every N epochs, after the validation and the keep-best rotation, snapshot the WHOLE training state (parameters, Adam '
                        'moments, BatchNorm buffers, the schedule counter, the host generators, the replay lists of the cycled loaders) to '
                        '<save_path>/last_state.pth: one HIP gather (ramdsir/ckpt.py, rd_snapshot), a copy beside the next epoch, a writer '
                        'thread; --norm bn, one process; 0 = off (the default)')
    p.add_argument('--resume', type=str, default=None, metavar='PATH',
                   help='continue from a --ckpt_every snapshot: with --gpu_data or --num_workers 0 the continuation is bit-identical to the '
                        'uninterrupted run; the arguments that shape the run must be those of the snapshot')
    p.add_argument('--stop_after_epochs', type=int, default=0, metavar='K',
                   help='leave after K epochs of THIS process, once the last snapshot is on disk, without writing final_model.pth -- as a '
                        'preempted job would; needs --ckpt_every (slices a run into jobs)')
    p.add_argument('--avg_weights', type=str, default=None, choices=['ema', 'uniform'],
                   help='keep a second copy of the model averaged along the training trajectory -- an exponential moving average, or the '
                        'uniform average of every iterate from --avg_start on -- by one HIP launch behind every step (ramdsir/avg.py, '
                        'rd_avg_step); with --fused_val it is validated per epoch beside the live model (<target>_val_log_avg.csv, '
                        'model_avg_%%.2f.pth); final_model_avg.pth at the end; BatchNorm running statistics are averaged like parameters '
                        '(see --avg_bn_recal); --norm bn only; off by default')
    p.add_argument('--avg_bn_recal', type=int, default=0, metavar='K',
                   help='--avg_weights: at the end of every epoch, before the averaged model is validated, and once more before '
                        'final_model_avg.pth is written, re-estimate the BatchNorm running statistics of the averaged encoder and seg '
                        'decoder from the last K training batches of the epoch (no new draws: the clean half of the step\'s input is '
                        'copied into a device ring), as torch.optim.swa_utils.update_bn does with momentum=None: a forward-only HIP launch '
                        'list with batch statistics and one rd_bn_recal launch per batch (ramdsir/avg_bn.py); num_batches_tracked = K; the '
                        'restoration decoder takes no part in inference and keeps its averaged DSBN buffers; K at most the iterations of an '
                        'epoch; --norm bn only; default 0 (off)')
    p.add_argument('--avg_decay', type=float, default=None, metavar='D', help='--avg_weights ema: the decay, in (0, 1); default %g' % AVG_DECAY)
    p.add_argument('--avg_start', type=int, default=None, metavar='ITER',
                   help='--avg_weights: the iteration from which on iterates are averaged; until then the averaged model is a copy of the '
                        'live one; default 0')
    p.add_argument('--clip_grad_norm', type=float, default=None, metavar='X',
                   help='before Adam, scale the gradient of the whole model (all three parameter groups jointly, as '
                        'torch.nn.utils.clip_grad_norm_ over the one optimizer) by min(1, X / (norm + 1e-6)); X > 0 and finite; decided on '
                        'the device in HIP (ramdsir/guard.py), no read-back; implies --skip_nonfinite; --norm bn only; off by default')
    p.add_argument('--skip_nonfinite', action='store_true',
                   help='a step whose gradient holds a NaN or an infinity, or whose norm is not finite, leaves no trace in the model: '
                        'parameters and Adam moments stay, every BatchNorm buffer is rolled back, the bias corrections count the updates '
                        'applied; the iteration counter (and with it the lr schedule) still advances; --norm bn only; off by default')
    p.add_argument('--weight_decay', type=float, default=0.0, metavar='W',
                   help='weight decay of the fused step\'s Adam (ramdsir/optim.py, rd_optim_step), applied to tensors with more than one '
                        'dimension -- the convolution kernels; 1-D tensors (biases, BatchNorm weight and bias) are exempt; W >= 0 and '
                        'finite; --norm bn only; default 0')
    p.add_argument('--wd_mode', choices=['decoupled', 'l2'], default='decoupled',
                   help='--weight_decay: decoupled multiplies the parameter by 1 - lr * W in front of the update (torch.optim.AdamW, with '
                        'the lr of the parameter\'s group); l2 adds W * parameter to the gradient (torch.optim.Adam(weight_decay), behind '
                        '--clip_grad_norm\'s scale); l2 needs --weight_decay; default decoupled')
    p.add_argument('--lr_schedule', choices=['poly', 'cosine', 'constant'], default='poly',
                   help='poly: the reference\'s lr * (1 - iter / total) ^ 0.9, one iteration behind as there (code/train.py:289-293); cosine: '
                        '0.5 * lr * (1 + cos(pi * iter / total)); constant: lr; evaluated on the device; --norm bn only; default poly')
    p.add_argument('--warmup_iters', type=int, default=0, metavar='N',
                   help='multiply the scheduled lr of iteration i by min(1, (i + 1) / N); fewer than the run\'s iterations; --norm bn '
                        'only; default 0 (none)')
    p.add_argument('--enc_lr_mult', type=float, default=0.5, metavar='M',
                   help='the encoder\'s learning rate as a multiple of --lr; M > 0 and finite; --norm bn only; default 0.5, the '
                        'reference\'s lr / 2 (code/train.py:573)')
    p.add_argument('--accum_steps', type=int, default=1, metavar='N',
                   help='gradient accumulation: forward, losses and backward run at every iteration as ever, the optimizer (with '
                        '--clip_grad_norm / --skip_nonfinite, the optimizer flags and --avg_weights where they are on) at every N-th '
                        'iteration only, on the mean of the N micro-batch gradients, summed in a second arena by one HIP launch per '
                        'iteration (ramdsir/accum.py, rd_grad_accum); the lr schedule, --warmup_iters and --avg_start count updates '
                        '(iterations // N), epochs, --max_iters and --tb_images count iterations, trailing iterations that complete no '
                        'window are never applied; BatchNorm moves its running statistics at every iteration; the --log_every console and '
                        'scalar lines and --tb_images report the current micro-batch\'s losses and the last update\'s lr, not window '
                        'means; --norm bn, one process, not with --tb_every_iter / --tb_health; default 1 (off)')
    return p.parse_args(argv)


def worker_cap(requested, world, n_domains, cpus=None):
    """DataLoader workers per domain loader of one rank: min(requested, cores // (domains x ranks)), at least 1 unless 0 was
    asked for (single-process loading)."""
    if requested <= 0:
        return 0
    cpus = cpus or os.cpu_count() or 8
    return max(1, min(requested, cpus // max(1, n_domains * world)))


def seed_worker(worker_id):
    worker_seed = torch.initial_seed() % 2 ** 32
    np.random.seed(worker_seed)
    random.seed(worker_seed)


def fundus_testset(data_dir, datasetTest):
    return Fundus(base_dir=data_dir, split='test', domain_idx=datasetTest, transform=Compose([trans.Resize((256, 256)), trans.Normalize()]))


def start_host_val(data_dir, datasetTest, batch_size):
    """The test loader and the post-processing pool of the Fundus host path, made to live across epochs: the reference rebuilds an
    8-worker loader and post-processes every 800x800 prediction serially at every epoch (~0.2 s per image: connected components +
    hole filling) -- seconds per epoch, invisible next to its training time, most of the wall clock next to this one's.
    Call it BEFORE the process's first GPU call.  Returns (loader, pool, the loader's started iterator) for close_host_val."""
    import multiprocessing as mp
    testset = fundus_testset(data_dir, datasetTest)
    nw = min(8, max(1, len(testset) // 2))
    loader = DataLoader(testset, batch_size=batch_size, num_workers=nw, shuffle=False, drop_last=False, pin_memory=True,
                        persistent_workers=True)
    pool = mp.get_context('fork').Pool(min(16, max(2, (os.cpu_count() or 4) // 4)))     # children never touch the GPU
    # a DataLoader forks its workers at the first iter(), not at construction: start them NOW, from an address space that has never
    # initialised HIP.  With persistent_workers it keeps this iterator (and its workers) and resets it at every `for ... in loader`.
    return loader, pool, iter(loader)


def close_host_val(host):
    """Ends the pool; the loader's persistent workers shut down with its iterator, when the caller drops `host`."""
    host[1].terminate()
    host[1].join()


def report_fundus(dices, epoch, datasetTest, output_path, batch_size, suffix=''):
    """The end of train.py:91-132: the mean cup / disc Dice of [(cup, disc)] per image, the console line, the reference's CSV line
    (in <target>_val_log<suffix>.csv: '_avg' for the averaged model of --avg_weights)."""
    cup = disc = 0.0
    for c, d in dices:
        cup, disc = cup + c, disc + d
    cup, disc = cup / max(len(dices), 1), disc / max(len(dices), 1)
    print('val_cup_dice : {}, val_disc_dice : {}'.format(cup, disc))
    with open(osp.join(output_path, str(datasetTest) + '_val_log%s.csv' % suffix), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['cup dice coefficence: '] + [cup] +
                                   ['disc dice coefficence: '] + [disc]])) + '\n')
    return (cup + disc) * 100.0 / 2


def report_prostate(val_dice, epoch, datasetTest, output_path, batch_size, suffix=''):
    """The end of train.py:134-192: the console line and the reference's CSV line of the mean volume Dice (in
    <target>_val_log<suffix>.csv)."""
    print('val_dice : {}'.format(val_dice))
    with open(osp.join(output_path, str(datasetTest) + '_val_log%s.csv' % suffix), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['dice coefficence: '] + [val_dice]])) + '\n')
    return val_dice * 100.0


def test_fundus(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='fundus', host=None):
    """train.py:91-132 (BN in eval mode here, as in the reference's in-training evaluation): sigmoid, bilinear resize to the
    native mask size, threshold 0.75, largest component + hole filling, Dice with +1 smoothing, one CSV line.  host: what
    start_host_val returned before the first GPU call; without it a loader and a pool live for this call, as in the reference."""
    encoder.eval()
    seg_decoder.eval()
    loader, pool, _ = own = host or start_host_val(data_dir, datasetTest, batch_size)
    pending = []
    with torch.no_grad():
        for data, target, target_orig, ids in loader:
            pred = torch.sigmoid(seg_decoder(encoder(data.cuda(non_blocking=True))))
            pred = torch.nn.functional.interpolate(pred, size=(target_orig.size(2), target_orig.size(3)), mode='bilinear')
            masks = (pred > 0.75).to(torch.uint8).cpu().numpy()                  # the threshold of postprocessing(), on the GPU
            tg = target_orig.to(torch.uint8).numpy()
            pending.append(pool.map_async(post_and_dice, [(masks[i], tg[i]) for i in range(masks.shape[0])]))
    dices = [cd for r in pending for cd in r.get()]
    if host is None:
        close_host_val(own)
    return report_fundus(dices, epoch, datasetTest, output_path, batch_size)


def test_fundus_gpu(encoder, seg_decoder, epoch, resident, datasetTest, output_path, batch_size=8, forward=None, suffix=''):
    """test_fundus with everything after the forward pass on the GPU (--gpu_val; ramdsir/gpu_val.py, csrc/val_post.hip): the same
    batches in list order through the same modules, the same CSV line, the same return value; Dice from integer counts, read back once.
    resident: gpu_val.preload's set.  forward (--fused_val): the infer.EvalForward that runs the forward pass instead of the modules
    (its parameters are the model that is validated); suffix: of the CSV's name."""
    from ramdsir import gpu_val
    return report_fundus(gpu_val.validate(encoder, seg_decoder, resident, batch_size, forward=forward), epoch, datasetTest, output_path,
                         batch_size, suffix)


def test_prostate(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='prostate'):
    """train.py:134-192: Dice over the NIfTI volumes of the held-out site (BN in eval mode), one line in
    <target>_val_log.csv.  `data_dir` is the dataset directory (<data_root>/prostate)."""
    from utils.prostate_eval import DOMAIN_LIST, evaluate_domain
    encoder.eval()
    seg_decoder.eval()
    with torch.no_grad():
        val_dice, _, _ = evaluate_domain(lambda v: seg_decoder(encoder(v.cuda())), data_dir, DOMAIN_LIST[datasetTest], batch_size)
    return report_prostate(val_dice, epoch, datasetTest, output_path, batch_size)


def test_prostate_gpu(encoder, seg_decoder, epoch, resident, datasetTest, output_path, batch_size=8, forward=None, suffix=''):
    """test_prostate on the resident volumes (--gpu_val_volumes; ramdsir/gpu_val_volumes.py, csrc/val_volume.hip): the same batches
    through the same modules, the same CSV line, the same return value; Dice from integer counts, read back once.  resident:
    gpu_val_volumes.preload's volumes.  forward (--fused_val): the infer.EvalForward that runs the forward pass instead of the modules;
    suffix: of the CSV's name."""
    from ramdsir import gpu_val_volumes
    val_dice = 0.0
    for d in gpu_val_volumes.validate(encoder, seg_decoder, resident, batch_size, forward=forward):
        val_dice += d
    return report_prostate(val_dice / max(len(resident), 1), epoch, datasetTest, output_path, batch_size, suffix)


def val_mode(args, on_disk, fits=True):
    """How this run validates, as data: (mode, console line at the resident preload or None, console line where the fused forward is
    bound or None).  mode: 'none' (no data on disk), 'host', 'resident' (--gpu_val / --gpu_val_volumes) or 'fused' (resident with
    --fused_val's forward).  on_disk: the held-out data exists; fits: the resident preload fitted (True before it has been tried)."""
    wants_resident = args.gpu_val if args.dataset == 'fundus' else args.gpu_val_volumes and args.num_classes == 2
    mode = 'none' if not on_disk else 'host' if not (wants_resident and fits) else 'fused' if args.fused_val else 'resident'
    preload_line = bind_line = None
    if args.dataset == 'prostate' and args.gpu_val_volumes and args.num_classes != 2:
        # the host path sums the class indices of a component (ndi.sum(mask, ...)); the kernels count voxels: two classes only
        preload_line = 'gpu_val_volumes: --num_classes %d is not 2: validating on the host' % args.num_classes
    if args.fused_val and mode != 'fused':
        bind_line = 'fused_val: the resident validation is not in use: validating through the modules'
    return mode, preload_line, bind_line


class Validation:
    """The in-training validation of one run, on rank 0: the held-out domain, whether its data is on disk, and what the mode keeps
    across epochs (the host path's loader and pool, or the resident data and --fused_val's forward).  Its three steps sit at fixed
    places in main(): the constructor before the first GPU call, preload() on the device, bind() on the trainer."""

    def __init__(self, args, data_root):
        """INVARIANT: runs before the process's first HIP call.  Fundus host path: the pool and the test loader's workers are forked
        here, and the loader's iterator takes one 64-bit draw (its base seed) from torch's global generator, which the training
        samplers shuffle from.  --gpu_val creates neither and takes that one draw itself, so that the trained model does not depend
        on the flag.  Prostate forks nothing and draws nothing."""
        self.args, self.data_root, self.domain, self.batch_size = args, data_root, args.test_domain_idx, args.test_batch_size
        self.fundus = args.dataset == 'fundus'
        self.host = self.resident = self.forward = self.bind_line = None
        if self.fundus:
            self.on_disk = os.path.exists(os.path.join(data_root, 'Domain%d_test.list' % (self.domain + 1)))
        else:
            from utils.prostate_eval import DOMAIN_LIST
            self.site = DOMAIN_LIST[self.domain]
            self.on_disk = os.path.isdir(os.path.join(data_root, self.site))
        self.mode = val_mode(args, self.on_disk)[0]         # 'resident' / 'fused' stand until preload() has tried
        if self.fundus and self.mode == 'host':
            self.host = start_host_val(data_root, self.domain, self.batch_size)
        elif self.fundus and self.mode != 'none':
            torch.empty((), dtype=torch.int64).random_()

    def preload(self, workers):
        """After torch.cuda.set_device: the held-out data, decoded once and kept on this GPU (ramdsir/gpu_val.py, gpu_val_volumes.py);
        the host path if it does not fit.  INVARIANT: Fundus then starts the host resources late and leaves torch's generator where
        it was (the constructor took the loader's draw); the Prostate host path has no loader and no pool, so nothing to reproduce."""
        args, wants, t0 = self.args, self.mode in ('resident', 'fused'), time.time()
        if wants and self.fundus:
            from ramdsir import gpu_val, modules
            nhwc = modules.storage_dtype() if args.fused_val else None      # the inputs also as the fused forward reads them
            self.resident = val_set = gpu_val.preload(fundus_testset(self.data_root, self.domain), workers=workers,
                                                      batch_size=self.batch_size, nhwc_dtype=nhwc)
            if val_set is not None:
                print('gpu_val: %d test images, %.3f GB resident%s, preloaded in %.1f s'
                      % (len(val_set), val_set.nbytes / 1e9, '' if nhwc is None else ' (%.3f GB of it the NHWC %s inputs of --fused_val)'
                         % (val_set.inputs_nhwc.numel() * val_set.inputs_nhwc.element_size() / 1e9, 'bf16' if nhwc == torch.bfloat16 else 'fp32'),
                         time.time() - t0))
            else:
                rng_state = torch.get_rng_state()
                self.host = start_host_val(self.data_root, self.domain, self.batch_size)
                torch.set_rng_state(rng_state)
        elif wants:
            from ramdsir import gpu_val_volumes
            self.resident = vols = gpu_val_volumes.preload(self.data_root, self.site, batch_size=self.batch_size, workers=workers)
            if vols is not None:
                print('gpu_val_volumes: %d volumes, %.3f GB resident + %.3f GB scratch, preloaded in %.1f s'
                      % (len(vols), vols.nbytes / 1e9, vols.scratch_bytes / 1e9, time.time() - t0))
        self.mode, line, self.bind_line = val_mode(args, self.on_disk, not wants or self.resident is not None)
        if line:
            print(line)

    def bind(self, trainer):
        """Once the trainer exists: --fused_val's forward pass as one launch list over the trainer's own parameter arena
        (ramdsir/infer.py), only where the resident validation is in use (what did not fit validates through the modules)."""
        if self.mode == 'fused':
            from ramdsir.infer import EvalForward
            self.forward = EvalForward.from_trainer(trainer)
            print('fused_val: validation forward as one launch list per batch, %s storage, %s' % (
                'bf16' if self.forward.dtype == torch.bfloat16 else 'fp32',
                'its own weight pack (one repack per pass)' if self.forward.owns_pack else "the step's weight pack (no repack)"))
        elif self.bind_line:
            print(self.bind_line)

    def __call__(self, encoder, seg_decoder, epoch):
        """One pass (train.py:331-341): the average Dice in percent; None when the data is not on disk (synthetic / smoke runs)."""
        if self.mode == 'none':
            return None
        print('Test on target domain {}'.format(self.domain))
        models, tail = (encoder, seg_decoder, epoch), (self.domain, self.args.save_path, self.batch_size)
        if self.mode == 'host' and self.fundus:
            return test_fundus(*models, self.data_root, *tail, host=self.host)
        if self.mode == 'host':
            return test_prostate(*models, self.data_root, *tail)
        return (test_fundus_gpu if self.fundus else test_prostate_gpu)(*models, self.resident, *tail, forward=self.forward)

    def averaged(self, avg, encoder, seg_decoder, epoch):
        """--avg_weights: a second pass of the resident validation, through the fused forward over the AVERAGED bank
        (avg.WeightAverage.eval_forward(); the pass begins with its refresh(): the averaged weights repacked, the frozen BatchNorm
        coefficients from the averaged running statistics), into <target>_val_log_avg.csv.  The average Dice in percent; None where
        the fused forward is not in use -- the modules' forward reads the live parameters."""
        if self.mode != 'fused':
            return None
        print('Test the averaged model on target domain {}'.format(self.domain))
        test = test_fundus_gpu if self.fundus else test_prostate_gpu
        return test(encoder, seg_decoder, epoch, self.resident, self.domain, self.args.save_path, self.batch_size,
                    forward=avg.eval_forward(), suffix='_avg')

    def close(self):
        if self.host is not None:
            close_host_val(self.host)
        self.host = self.resident = self.forward = None


def save_checkpoint(path, encoder, seg_decoder, rec_decoder):
    """train.py:342-360: unwrapped state_dicts under the reference's three keys."""
    torch.save({'encoder_state_dict': encoder.state_dict(), 'seg_decoder_state_dict': seg_decoder.state_dict(),
                'rec_decoder_state_dict': rec_decoder.state_dict()}, path)


def make_loaders(args, data_root, world, rank, bsl, domain_idx_list, replay=False):
    """train.py:554-560: one loader per training domain, cycled except the longest.  --gpu_data: the same construction over the
    parameter datasets of ramdsir/gpu_data.py, loaded in this process.  replay (--ckpt_every / --resume): the cycles are ckpt.ReplayCycle,
    itertools.cycle with a state that can be saved.  Returns (raw loaders, samplers, iterables, longest length)."""
    zoo = {'fundus': Fundus_Multi, 'prostate': Prostate_Multi}
    if args.gpu_data:
        from ramdsir import gpu_data
        zoo = gpu_data.PARAMS
    transform = {'fundus': Compose([trans.Resize((256, 256)), trans.RandomScaleCrop((256, 256))]), 'prostate': None}
    loaders, max_len, max_id = [], -1, 0
    raw, samplers = [], []
    for idx, i in enumerate(domain_idx_list):
        ds = zoo[args.dataset](base_dir=data_root, split='train', domain_idx_list=[i], transform=transform[args.dataset],
                               is_out_domain=args.is_out_domain, test_domain_idx=args.test_domain_idx)
        # Data parallel (one process per GPU): every domain's list is SHARDED over the ranks (DistributedSampler, reshuffled
        # per epoch with seed + epoch), each rank draws the reference's per-domain batch sizes from its shard, so one step
        # consumes world x the reference's batch and an epoch is 1/world as many iterations; RAM partners / lambda / crops
        # are drawn rank-locally (workers are seeded from seed + rank).  Single process: exactly the reference's loaders.
        sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed, drop_last=True) if world > 1 else None
        # the reference's loader settings (train.py:558-559) + persistent workers with a deeper queue: the reference respawns its
        # 3 x 8 worker processes at every epoch, which costs seconds per 53-iteration epoch -- invisible next to its step time,
        # 20x the step time here (profiles/README.md, end-to-end throughput)
        extra = dict(persistent_workers=True, prefetch_factor=4) if args.num_workers > 0 else {}
        if args.gpu_data:               # the parameter datasets (--gpu_data): draws in this process, records as they are
            extra = dict(num_workers=0, pin_memory=False, collate_fn=gpu_data.collate)
        else:
            extra.update(num_workers=args.num_workers, pin_memory=True)
        dl = DataLoader(ds, batch_size=bsl[idx], shuffle=sampler is None, sampler=sampler, drop_last=True,
                        worker_init_fn=seed_worker, **extra)
        raw.append(dl)
        samplers.append(sampler)
        if replay:
            from ramdsir.ckpt import ReplayCycle
            loaders.append(ReplayCycle(dl))
        else:
            loaders.append(cycle(dl))                   # train.py:560: replays the first pass of the shorter loaders
        if max_len < len(dl):
            max_len, max_id = len(dl), idx
    loaders[max_id] = raw[max_id]
    return raw, samplers, loaders, max_len


def uses_step_log(args):
    """Either flag turns the per-step ring on (ramdsir/step_log.py); without both, the run never touches it."""
    return bool(args.tb_every_iter or args.tb_health)


def uses_ckpt(args):
    """Any of the three flags turns the resumable-state machinery on (ramdsir/ckpt.py); without them the run never touches it."""
    return bool(args.ckpt_every or args.resume or args.stop_after_epochs)


def uses_avg(args):
    """--avg_weights turns the averaged model on (ramdsir/avg.py); without it the run allocates and launches nothing for it."""
    return args.avg_weights is not None


def avg_settings(args):
    """(mode, decay, start) of --avg_weights with the defaults of the two flags that were not given."""
    return args.avg_weights, AVG_DECAY if args.avg_decay is None else args.avg_decay, 0 if args.avg_start is None else args.avg_start


def uses_bn_recal(args):
    """--avg_bn_recal K > 0 turns the BatchNorm re-estimation of the averaged model on (ramdsir/avg_bn.py); at 0 nothing is constructed."""
    return args.avg_bn_recal != 0


def check_bn_recal(args, max_len):
    """The one refusal of --avg_bn_recal that needs the length of an epoch: where it becomes known, in front of the preload, the
    trainer and any launch."""
    if uses_bn_recal(args) and args.avg_bn_recal > max_len:
        raise ValueError('--avg_bn_recal %d is more than the %d iterations of an epoch of this run' % (args.avg_bn_recal, max_len))


def uses_guard(args):
    """Either flag turns the guarded optimizer step on (ramdsir/guard.py); without both the step is the unguarded one, launch for
    launch."""
    return bool(args.clip_grad_norm is not None or args.skip_nonfinite)


def guard_max_norm(args):
    """The guard's max_norm: --clip_grad_norm, or 0 (no clipping) for --skip_nonfinite alone."""
    return 0.0 if args.clip_grad_norm is None else float(args.clip_grad_norm)


GUARD_TAGS = ('guard/grad_norm', 'guard/scale', 'guard/clipped', 'guard/skipped')


def guard_pairs(g):
    """The four scalars of a logging iteration from the guard's state word: norm and scale of that iteration's step, the counts so far."""
    return list(zip(GUARD_TAGS, (g['norm'], g['scale'], float(g['clipped']), float(g['skipped']))))


def guard_suffix(g):
    return ' grad_norm %.4g scale %.4g clipped %d skipped %d' % (g['norm'], g['scale'], g['clipped'], g['skipped'])


OPTIM_DEFAULTS = dict(weight_decay=0.0, wd_mode='decoupled', lr_schedule='poly', warmup_iters=0, enc_lr_mult=0.5)


def optim_settings(args):
    """The five optimizer flags as FusedTrainer.enable_optim takes them."""
    return {k: getattr(args, k) for k in OPTIM_DEFAULTS}


def uses_optim(args):
    """Any of the five flags away from its default turns the grouped Adam on (ramdsir/optim.py); with all five at their defaults
    nothing is constructed and the step is the reference's rd_adam_step, launch for launch."""
    return any(getattr(args, k) != v for k, v in OPTIM_DEFAULTS.items())


def uses_accum(args):
    """--accum_steps above 1 turns gradient accumulation on (ramdsir/accum.py); at 1 nothing is constructed and the step is the
    unflagged one, launch for launch."""
    return args.accum_steps != 1


def accum_totals(args, max_len):
    """(updates, iterations, trailing iterations that complete no window) of the run: the schedule, --warmup_iters and the fingerprint
    count updates, the loop counts iterations.  A run with no complete window is refused."""
    iterations = max_len * args.epochs
    updates, trailing = iterations // args.accum_steps, iterations % args.accum_steps
    if updates < 1 and uses_accum(args):
        raise ValueError('--accum_steps %d: the %d iterations of this run complete no window (no optimizer update would be applied)'
                         % (args.accum_steps, iterations))
    return updates, iterations, trailing


def accum_line(steps, updates, iterations, trailing):
    return ('accum: %d micro-batches per update: %d updates over %d iterations, %d trailing iteration%s applied'
            % (steps, updates, iterations, trailing, ' is not' if trailing == 1 else 's are not'))


def val_log_path(args, suffix=''):
    return osp.join(args.save_path, str(args.test_domain_idx) + '_val_log%s.csv' % suffix)


def console_line(iter_num, lr_now, l):
    return ('iter %d lr %.6f ' % (iter_num, lr_now) + ' '.join('%s %.4f' % (k, v) for k, v in l.items() if k != 'rec')
            + ' loss_rec %.4f' % (sum(l['rec']) / 4))                 # train.py:304 logs avg/4


def scalar_pairs(lr_now, l):
    """The reference's seven scalars of one iteration (train.py:298-304 / 467-473), in its order."""
    return [('lr', lr_now)] + [('loss/' + k, v) for k, v in l.items() if k not in ('rec', 'loss')] + [('loss/loss_rec', sum(l['rec']) / 4)]


def step_log_pairs(rec, every_iter, health, log_every):
    """What one drained record (ramdsir/step_log.py) contributes to the event file: the seven scalars at every iteration with
    --tb_every_iter, otherwise at the --log_every iterations as always; behind them the four health tags with --tb_health."""
    from ramdsir.step_log import HEALTH_TAGS
    pairs = scalar_pairs(rec['lr'], rec['losses']) if every_iter or rec['iteration'] % log_every == 0 else []
    if health:
        pairs += list(zip(HEALTH_TAGS, rec['norms'] + (float(rec['nonfinite']),)))
    return pairs


def record_is_finite(rec):
    l = rec['losses']
    return rec['nonfinite'] == 0 and all(np.isfinite(v) for k, v in l.items() if k != 'rec') and all(np.isfinite(v) for v in l['rec']) \
        and all(np.isfinite(v) for v in rec['norms'])


def uses_tb_hist(args):
    return args.tb_hist > 0


def tb_hist_what(args):
    """--tb_hist_what as a tuple of kinds; ValueError for an unknown, repeated or empty one (no GPU call: the module only parses)."""
    from ramdsir import tb_hist
    return tb_hist.DEFAULT_WHAT if args.tb_hist_what is None else tb_hist.parse_what(args.tb_hist_what)


def check_args(args, world):
    """Every flag combination this script refuses, and nothing else: no GPU call, no file, no process."""
    if not (args.ram and args.rec):
        # the reference only runs end-to-end with --ram --rec (train.py:591 / :315 raise otherwise)
        raise ValueError('only the --ram --rec flag combination exists in the reference; got ram=%s rec=%s' % (args.ram, args.rec))
    if args.gpu_val and args.dataset != 'fundus':
        raise ValueError('--gpu_val covers the in-training Fundus validation only; --dataset %s validates on the host' % args.dataset)
    if args.tb_images < 0:
        raise ValueError('--tb_images takes a positive interval, got %d' % args.tb_images)
    if args.gpu_val_volumes and args.dataset != 'prostate':
        raise ValueError('--gpu_val_volumes covers the in-training Prostate validation only; --dataset %s has --gpu_val' % args.dataset)
    if args.fused_val and not (args.gpu_val or args.gpu_val_volumes):
        raise ValueError('--fused_val is the forward pass of the resident validation: it needs --gpu_val (fundus) or --gpu_val_volumes (prostate)')
    if uses_step_log(args) and args.norm != 'bn':
        raise ValueError('--tb_every_iter / --tb_health read the fused step\'s device buffers: --norm %s trains through the modules, whose '
                         'losses are host-visible tensors (use --log_every 1 there)' % args.norm)
    if args.fused_val and args.norm != 'bn':
        raise ValueError('--fused_val freezes BatchNorm on its running statistics: --norm %s has none (validate through the modules)' % args.norm)
    if args.ckpt_every < 0 or args.stop_after_epochs < 0:
        raise ValueError('--ckpt_every / --stop_after_epochs take a number of epochs, got %d / %d' % (args.ckpt_every, args.stop_after_epochs))
    if args.stop_after_epochs and not args.ckpt_every:
        raise ValueError('--stop_after_epochs leaves the run to be resumed: it needs --ckpt_every')
    if uses_ckpt(args) and args.norm != 'bn':
        raise ValueError('--ckpt_every / --resume / --stop_after_epochs snapshot the fused step\'s arenas: --norm %s trains through the modules, '
                         'whose Adam is torch\'s' % args.norm)
    if uses_ckpt(args) and world > 1:
        raise ValueError('--ckpt_every / --resume / --stop_after_epochs run in one process: BatchNorm buffers, generators and replay lists '
                         'are rank-local (WORLD_SIZE=%d)' % world)
    if not uses_avg(args) and (args.avg_decay is not None or args.avg_start is not None):
        raise ValueError('--avg_decay / --avg_start shape the averaged model: they need --avg_weights')
    if uses_avg(args) and args.norm != 'bn':
        raise ValueError('--avg_weights averages the fused step\'s parameter arena behind its Adam launch: --norm %s trains through the '
                         'modules, whose Adam is torch\'s' % args.norm)
    if args.avg_weights == 'uniform' and args.avg_decay is not None:
        raise ValueError('--avg_decay is the decay of --avg_weights ema; uniform weighs every iterate alike')
    # (the kernel's weight is 1 - decay formed in float32: a decay that rounds to 1 there is refused with the ones outside the interval)
    if args.avg_decay is not None and not (0.0 < args.avg_decay < 1.0 and 0.0 < float(np.float32(1) - np.float32(args.avg_decay)) < 1.0):
        raise ValueError('--avg_decay takes a decay in (0, 1), got %r' % args.avg_decay)
    if args.avg_start is not None and args.avg_start < 0:
        raise ValueError('--avg_start takes an iteration number, got %d' % args.avg_start)
    if args.avg_bn_recal < 0:
        raise ValueError('--avg_bn_recal takes a number of batches (0 = off), got %d' % args.avg_bn_recal)
    if uses_bn_recal(args) and not uses_avg(args):
        raise ValueError('--avg_bn_recal re-estimates the BatchNorm statistics of the averaged model: it needs --avg_weights')
    if uses_bn_recal(args) and args.norm != 'bn':
        raise ValueError('--avg_bn_recal re-estimates BatchNorm running statistics: --norm %s has none' % args.norm)
    # (the kernel receives the norm as float32: a value that is infinite there is refused with the ones that are infinite as given)
    if args.clip_grad_norm is not None and not 0.0 < args.clip_grad_norm <= float(np.finfo(np.float32).max):      # NaN fails both
        raise ValueError('--clip_grad_norm takes a positive finite norm, got %r' % args.clip_grad_norm)
    if uses_guard(args) and args.norm != 'bn':
        raise ValueError('--clip_grad_norm / --skip_nonfinite guard the fused step\'s Adam launch: --norm %s trains through the modules, '
                         'whose Adam is torch\'s' % args.norm)
    # (the kernel receives both factors as float32: values that are infinite there are refused with the ones infinite as given)
    if not 0.0 <= args.weight_decay <= float(np.finfo(np.float32).max):                                           # NaN fails both
        raise ValueError('--weight_decay takes a decay that is 0 or positive and finite, got %r' % args.weight_decay)
    if args.wd_mode != 'decoupled' and not args.weight_decay > 0:
        raise ValueError('--wd_mode shapes the weight decay: it needs --weight_decay')
    if args.warmup_iters < 0:
        raise ValueError('--warmup_iters takes a number of iterations, got %d' % args.warmup_iters)
    if not 0.0 < args.enc_lr_mult <= float(np.finfo(np.float32).max) or float(np.float32(args.enc_lr_mult)) == 0.0:
        raise ValueError('--enc_lr_mult takes a positive finite multiplier, got %r' % args.enc_lr_mult)
    if uses_optim(args) and args.norm != 'bn':
        raise ValueError('--weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult shape the fused step\'s Adam launch: '
                         '--norm %s trains through the modules, whose Adam is torch\'s' % args.norm)
    if args.accum_steps < 1:
        raise ValueError('--accum_steps takes a number of micro-batches per update, got %d' % args.accum_steps)
    if args.accum_steps > 65536:
        raise ValueError('--accum_steps takes at most 65536 micro-batches per update, got %d' % args.accum_steps)
    if uses_accum(args) and args.norm != 'bn':
        raise ValueError('--accum_steps accumulates the fused step\'s gradient arena in front of its Adam launch: --norm %s trains through '
                         'the modules, whose Adam is torch\'s' % args.norm)
    if uses_accum(args) and world > 1:
        raise ValueError('--accum_steps runs in one process: the bucketed gradient exchange is tied to the segments of the step '
                         '(WORLD_SIZE=%d)' % world)
    if uses_accum(args) and uses_step_log(args):
        raise ValueError('--accum_steps does not go with --tb_every_iter / --tb_health: the rows of the per-step ring are keyed by the '
                         'optimizer\'s counter, which moves once per window')
    if args.tb_hist < 0:
        raise ValueError('--tb_hist takes a positive interval, got %d' % args.tb_hist)
    if args.tb_hist_what is not None and not uses_tb_hist(args):
        raise ValueError('--tb_hist_what chooses the arenas of the histograms: it needs --tb_hist')
    if uses_tb_hist(args):
        tb_hist_what(args)
        if args.norm != 'bn':
            raise ValueError('--tb_hist reads the fused step\'s parameter, gradient and moment arenas: --norm %s trains through the modules, '
                             'which have no arenas behind a fused step' % args.norm)
        if uses_accum(args):
            raise ValueError('--tb_hist does not go with --accum_steps: inside a window the gradient arena holds a micro-batch gradient '
                             'that belongs to the accumulator, not the gradient of an update')


class TrainLog:
    """The logging side of the loop: the event file in <save_path>/log (train.py:538) and the console lines of rank 0, and --
    on every rank, because the drain is collective -- the reads of the per-step device ring (--tb_every_iter / --tb_health)."""

    def __init__(self, args, trainer, rank, imgs_per_iter, guard=None):
        self.args, self.trainer, self.rank0, self.imgs_per_iter = args, trainer, rank == 0, imgs_per_iter
        # --clip_grad_norm / --skip_nonfinite: the guard's state word is read at the logging iterations, behind the read of the losses
        self.guard = guard
        self.guard_mark = guard.read() if guard is not None else None      # (behind a --resume restore: the counts continue)
        # --tb_images: one writer thread owns the event file (scalars go through its queue too, so the records keep the order of the
        # calls); without the flag the direct writer, record for record what it always wrote
        Writer = QueuedWriter if (args.tb_images or uses_tb_hist(args)) else SummaryWriter
        self.writer = Writer(os.path.join(args.save_path, 'log')) if self.rank0 else None
        self.first_bad = None                               # --tb_health: the first iteration with non-finite values, named once
        self.t_mark, self.it_mark = None, 0                 # the throughput clock starts at iteration 5
        self.step_log = uses_step_log(args)
        if self.step_log:                                   # every step appends one row to a device-resident ring
            trainer.enable_step_log(health=args.tb_health)

    def drain(self):
        """Drain the ring (collective; synchronises) and write its records in iteration order, with the drain's wall time."""
        args, records = self.args, self.trainer.drain_step_log()
        now = time.time()
        for rec in records if self.rank0 else ():
            pairs = step_log_pairs(rec, args.tb_every_iter, args.tb_health, args.log_every)
            if pairs:
                self.writer.add_scalars_at(rec['iteration'], pairs, walltime=now)
            if args.tb_health and self.first_bad is None and not record_is_finite(rec):
                self.first_bad = rec['iteration']
                print('tb_health: iteration %d is the first with non-finite values (%d non-finite gradient elements, loss %r); the run '
                      'continues' % (rec['iteration'], rec['nonfinite'], rec['losses']['loss']))
        return records

    def guard_report(self, iter_num):
        """A logging iteration with the guard on: (the console line's suffix, the four guard/* scalars) from the state word -- read
        behind the read of the losses, which has synchronised already.  Warns when every step since the previous logging iteration
        was skipped.  Without the guard: ('', [])."""
        if self.guard is None:
            return '', []
        g, mark = self.guard.read(), self.guard_mark
        self.guard_mark = g
        steps, skipped = g['steps'] - mark['steps'], g['skipped'] - mark['skipped']
        if steps > 0 and skipped == steps:
            print('grad_guard: warning: every one of the %d steps up to iteration %d was skipped (non-finite gradients); the model has '
                  'not moved since iteration %d' % (steps, iter_num, iter_num - steps))
        return guard_suffix(g), guard_pairs(g)

    def after_step(self, iter_num, log_images, log_hist=False):
        """Behind the step of iteration iter_num.  With the ring, it is read where the loop synchronises anyway (the logging
        iterations), in front of image records (they follow the scalars of their own iteration) and when it is full -- all
        functions of iter_num alone, so every rank drains at the same iterations."""
        args, trainer = self.args, self.trainer
        log_now = iter_num % args.log_every == 0
        if self.step_log:
            if log_now or (args.tb_images > 0 and iter_num % args.tb_images == 0) or trainer.step_log_full():
                records = self.drain()
                if self.rank0 and log_now:                  # printed and written from the same drained row
                    suffix, pairs = self.guard_report(iter_num)
                    print(console_line(iter_num, records[-1]['lr'], records[-1]['losses']) + suffix)
                    if pairs:
                        self.writer.add_scalars_at(iter_num, pairs)
        elif log_now:
            l = trainer.losses()                            # collective when world > 1: the mean over the ranks
            if self.rank0:
                lr_now = trainer.lr()
                suffix, pairs = self.guard_report(iter_num)
                print(console_line(iter_num, lr_now, l) + suffix)
                # the reference's scalars (train.py:298-304 / 467-473), at the iterations whose losses are read back
                self.writer.add_scalars_at(iter_num, scalar_pairs(lr_now, l) + pairs)
        if log_images:                                      # behind the scalars of the iteration, in the reference's tag order
            self.writer.add_images_at(iter_num, trainer.take_tb_images())
        if log_hist:                                        # --tb_hist: the writer thread waits for the copy, trims and encodes
            self.writer.add_histograms_at(iter_num, trainer.take_tb_hist())
        if iter_num + 1 == 5:                               # end-to-end throughput (files -> DataLoader -> H2D -> step), start-up excluded
            torch.cuda.synchronize()
            self.t_mark, self.it_mark = time.time(), iter_num + 1

    def throughput(self, iter_num):
        if self.t_mark is not None and iter_num > self.it_mark:
            torch.cuda.synchronize()
            if self.rank0:
                print('train throughput: %.1f images/s end to end (%d iterations of %d images, %d DataLoader workers per domain)'
                      % ((iter_num - self.it_mark) * self.imgs_per_iter / (time.time() - self.t_mark), iter_num - self.it_mark,
                         self.imgs_per_iter, self.args.num_workers))

    def close(self):
        if self.writer is None:
            return
        self.writer.close()
        if self.args.tb_images and self.writer.seconds['calls']:
            sec, n = self.writer.seconds, self.writer.seconds['calls']
            print('tb_images: %d image records at %d iterations; writer thread per logging iteration: wait for the copy %.2f ms, PNG %.2f ms, '
                  'crc32c + framing %.2f ms, file write %.2f ms' % (sec['records'], n, 1e3 * sec['wait'] / n, 1e3 * sec['png'] / n,
                                                                    1e3 * sec['crc'] / n, 1e3 * sec['write'] / n))
        if uses_tb_hist(self.args) and self.writer.seconds['histo']['calls']:
            sec, n = self.writer.seconds['histo'], self.writer.seconds['histo']['calls']
            print('tb_hist: %d histogram records at %d iterations; writer thread per logging iteration: wait for the copy + trimming '
                  '%.2f ms, protobuf + crc32c + framing %.2f ms, file write %.2f ms' % (sec['records'], n, 1e3 * sec['wait'] / n,
                                                                                       1e3 * sec['encode'] / n, 1e3 * sec['write'] / n))


def build_trainer(args, rank, raw, resident, batch_sizes, max_len):
    """The three drop-in modules and the trainer over them.  Draws from torch's global generator: the modules' initialisation and
    next(iter(raw[0])), behind the loaders' construction and in front of the training."""
    encoder = Encoder(c=args.in_channels, norm=args.norm, activation=args.activation).cuda()
    seg_decoder = Decoder(num_classes=args.num_classes, norm=args.norm, activation=args.activation).cuda()
    rec_decoder = Rec_Decoder(num_classes=args.in_channels, norm='dsbn', activation=args.activation,
                              num_domains=len(batch_sizes)).cuda()
    print('\nEncoder Params: %.3fM' % count_params(encoder))
    print('\nSeg Decoder Params: %.3fM' % count_params(seg_decoder))
    print('\nRec Decoder Params: %.3fM' % count_params(rec_decoder))

    from ramdsir.trainer import FusedTrainer, ModuleTrainer
    sample = next(iter(raw[0]))
    H, W = resident.hw if resident is not None else sample[0].shape[1:3]
    # what the trainer's schedule, the warm-up check and the fingerprint count: optimizer updates (--accum_steps: iterations // N)
    total_iters = accum_totals(args, max_len)[0]
    cons = args.consistency_type if args.consistency else None
    assert cons in (None, 'mse', 'kd'), args.consistency_type
    # --norm bn (the reference's default): the fused HIP step.  gn / in: the reference's own loop over the drop-in modules (the fused step
    # keeps the statistics groups of the shared BatchNorms and of the restoration decoder's DSBN in one launch list: bn only)
    Trainer = FusedTrainer if args.norm == 'bn' else ModuleTrainer
    if args.norm != 'bn' and rank == 0:
        print('norm=%s: module-level training loop (torch autograd between the HIP modules)' % args.norm)
    trainer = Trainer(encoder, seg_decoder, rec_decoder, batch_sizes, H, W, dataset=args.dataset,
                      consistency=cons, lambda_rec=args.lambda_rec, lr=args.lr, total_iters=total_iters,
                      dtype=torch.bfloat16 if (args.dtype or ('bf16' if args.norm == 'bn' else 'f32')) == 'bf16' else torch.float32)
    return (encoder, seg_decoder, rec_decoder), trainer, (H, W), total_iters


def check_warmup(args, total_iters):
    """The one refusal that needs the length of the run: where total_iters becomes known, in front of any optimizer launch."""
    if args.warmup_iters >= total_iters:
        raise ValueError('--warmup_iters %d is not below the %d iterations of this run' % (args.warmup_iters, total_iters))


def enable_optim(args, trainer, total_iters, rank=0):
    """The grouped Adam of the five optimizer flags on the trainer, with its one summary line."""
    check_warmup(args, total_iters)
    optim = trainer.enable_optim(**optim_settings(args))
    if rank == 0:
        print('optim: %s schedule, warmup %d, encoder lr x %g; weight decay %g (%s) over %d ranges, %d of %d elements decay'
              % (args.lr_schedule, args.warmup_iters, args.enc_lr_mult, args.weight_decay, args.wd_mode, optim.n,
                 optim.decayed_elements(), trainer.bank.n))
    return optim


def restore_host_side(args, meta, loaders, raw):
    """The host side of a --resume snapshot, behind every start-up draw (the validation start, the loaders' construction,
    next(iter(raw[0]))): the three generators and the cycles (replaced in `loaders`) as the snapshotted process left them at the end
    of its epoch, and <domain>_val_log.csv cut back to its length at the snapshot.  Returns (first epoch, iter_num, previous_best)."""
    from ramdsir import ckpt
    ckpt.set_host_rng_state(meta['rng'])
    for idx, st in enumerate(meta['cycles']):
        if (st is None) != (loaders[idx] is raw[idx]):
            raise ValueError('--resume: the snapshot cycles other loaders than this run (domain %d)' % idx)
        if st is not None:
            loaders[idx] = ckpt.ReplayCycle.from_state(st)
    if os.path.exists(val_log_path(args)) and os.path.getsize(val_log_path(args)) > meta['val_log_bytes']:
        print('resume: %s truncated from %d to %d bytes (lines of epochs that ran after the snapshot and run again)'
              % (val_log_path(args), os.path.getsize(val_log_path(args)), meta['val_log_bytes']))
        with open(val_log_path(args), 'r+b') as f:
            f.truncate(meta['val_log_bytes'])
    print('resume: %s, continuing at epoch %d (iteration %d, best %.2f)' % (args.resume, meta['epoch'] + 1, meta['iter_num'], meta['previous_best']))
    return meta['epoch'] + 1, meta['iter_num'], meta['previous_best']


def restore_avg_host_side(args, meta):
    """--resume with --avg_weights: <domain>_val_log_avg.csv cut back to its length at the snapshot, as restore_host_side cuts the main
    one.  Returns previous_best_avg."""
    saved, path = meta['avg_weights'], val_log_path(args, '_avg')
    if os.path.exists(path) and os.path.getsize(path) > saved['val_log_bytes']:
        print('resume: %s truncated from %d to %d bytes' % (path, os.path.getsize(path), saved['val_log_bytes']))
        with open(path, 'r+b') as f:
            f.truncate(saved['val_log_bytes'])
    return saved['previous_best_avg']


def keep_best(save_path, avg_dice, previous_best, modules, averaged=None):
    """train.py:342-350: a validation at least as good as the best so far replaces model_<best>.pth.  Returns the best so far.
    averaged (--avg_weights): the avg.WeightAverage whose model was validated -- the same rotation over model_avg_<best>.pth, with the
    averaged state_dicts under the reference's three keys."""
    name = 'model_%.2f.pth' if averaged is None else 'model_avg_%.2f.pth'
    if avg_dice is None or not avg_dice >= previous_best:
        return previous_best
    if previous_best != 0:
        old = os.path.join(save_path, name % previous_best)
        if os.path.exists(old):
            os.remove(old)
    if averaged is None:
        save_checkpoint(os.path.join(save_path, name % avg_dice), *modules)
    else:
        torch.save(dict(averaged.state_dicts()), os.path.join(save_path, name % avg_dice))
    return avg_dice


def init_process(world, local):
    """This rank's device and, under torchrun, the process groups.  Returns the host-side rendezvous (gloo) for the points where
    ranks wait for rank 0 on the CPU (validation): an RCCL barrier is a GPU kernel that spins until every peer has arrived."""
    torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    return dist.new_group(backend='gloo') if world > 1 else None


def state_meta(trainer):
    """What the enabled stages of the trainer (FusedTrainer.stages()) record in a snapshot's meta, under their keys."""
    avg, guard, optim, accum = trainer.stages()
    meta = {key: obj.settings() for key, obj in (('avg_weights', avg), ('grad_guard', guard), ('optim', optim)) if obj is not None}
    if accum is not None:                               # an odd epoch length leaves a window open across the epoch boundary
        meta['grad_accum'] = dict(accum.settings(), micro=accum.position())
    return meta


def open_state(args, trainer, fingerprint_args, resume_state):
    """--ckpt_every / --resume, device side: the trainer's ranges, the staging buffers and the writer thread, once (ramdsir/ckpt.py);
    --resume: the arenas, the BatchNorm buffers and the schedule counter from the file (restore_host_side follows before the loop).
    What is enabled is read off the trainer (FusedTrainer.stages()):
    avg (--avg_weights): the averaged model's ranges go behind the trainer's; a file and a run that disagree about them are refused.
    guard (--clip_grad_norm / --skip_nonfinite): its state word goes behind those, under the same rule; behind a restore its shadow
    copies are taken from the restored BatchNorm buffers.  optim (the five optimizer flags): no range of its own -- its state is the
    arenas, the counter and the schedule words; a file taken under other settings (or, without the record, under the defaults) is
    refused.  accum (--accum_steps N > 1): the accumulator arena goes behind the other extra ranges -- a window that straddles an
    epoch boundary is open when the snapshot is taken -- and, with the guard on, so do the guard's shadow copies, which in mid-window
    hold the BatchNorm buffers of the window's START; a file taken under another N (without the record: N = 1) is refused; the restore
    sets the host-side position in the window."""
    from ramdsir import ckpt
    (avg, guard, _, accum), current, micro = trainer.stages(), state_meta(trainer), 0
    if resume_state is not None:
        ckpt.compare_avg_weights(resume_state, current.get('avg_weights'))
        ckpt.compare_grad_guard(resume_state, current.get('grad_guard'))
        ckpt.compare_optim(resume_state, current.get('optim'))
        micro = ckpt.compare_grad_accum(resume_state, current.get('grad_accum'))
    extra = (avg.named_ranges() if avg is not None else []) + (guard.named_ranges() if guard is not None else [])
    if accum is not None:
        extra += (guard.shadow_ranges() if guard is not None else []) + accum.named_ranges()
    state_io = ckpt.TrainState(trainer, ckpt.fingerprint(args, trainer, *fingerprint_args), extra=extra or None)
    if resume_state is not None:
        state_io.restore(resume_state)
        if accum is not None:
            accum.set_position(micro)
        elif guard is not None:
            guard.sync_shadow()
    if not args.gpu_data and args.num_workers > 0:
        print('ckpt: model, optimizer and schedule state are restored exactly; with DataLoader worker processes the draws come from '
              'freshly seeded workers (use --gpu_data or --num_workers 0 for a bit-identical continuation)')
    return state_io


def train_epoch(args, trainer, loaders, resident, log, iter_num, recal=None, epoch_len=0):
    """One pass over the zipped loaders; returns iter_num behind it.  One batch of look-ahead: the step of batch i also mixes batch
    i+1 (RAM) in its tail, beside Adam and the weight repack (FusedTrainer.step next_batch; the last iteration of an epoch -- or of
    --max_iters -- has no successor and runs the classical step).
    recal (--avg_bn_recal): the last K of the epoch's epoch_len iterations (fewer where --max_iters ends it early) also copy their
    input into the ring."""
    if recal is not None:
        recal.begin_epoch()
        n_epoch = min(epoch_len, args.max_iters - iter_num) if args.max_iters else epoch_len
        first_captured = iter_num + max(0, n_epoch - recal.K)
    def on_device(batches):
        if resident is not None:                        # --gpu_data: one rd_fundus_batch / rd_prostate_batch launch
            return resident.on_device(batches)
        return tuple(torch.cat([b[k] for b in batches], 0).cuda(non_blocking=True) for k in range(4))       # src, trg, lam, mask

    stream_it = iter(zip(*loaders))
    cur = next(stream_it, None)
    cur = on_device(cur) if cur is not None else None
    while cur is not None:
        nxt = next(stream_it, None)
        last = nxt is None or bool(args.max_iters and iter_num + 1 >= args.max_iters)
        nxt = None if last else on_device(nxt)
        log_images = log.rank0 and args.tb_images > 0 and iter_num % args.tb_images == 0      # train.py:306, 475
        if log_images:
            trainer.arm_tb_images()                     # this step also composes the grids of its batch and starts their copy
        if recal is not None and iter_num >= first_captured:
            trainer.arm_bn_capture()                    # ... and this one leaves the clean half of its input in the ring
        log_hist = args.tb_hist > 0 and iter_num % args.tb_hist == 0
        if log_hist:
            trainer.arm_tb_hist(copy=log.rank0)         # every rank enqueues the same step; rank 0 copies and writes
        trainer.step(*cur, next_batch=nxt)
        cur = nxt
        log.after_step(iter_num, log_images, log_hist and log.rank0)
        iter_num += 1
        if args.max_iters and iter_num >= args.max_iters:
            break
    return iter_num


def main(args):
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (('WORLD_SIZE', '1'), ('RANK', '0'), ('LOCAL_RANK', '0')))
    check_args(args, world)
    if uses_ckpt(args):
        from ramdsir import ckpt
    resume_state = ckpt.load_file(args.resume) if args.resume else None      # an unknown version or a corrupt range is refused here
    data_root = os.path.join(args.data_root, args.dataset)
    # INVARIANTS of the start-up order.  Every child process (validation pool, test-loader workers) is forked before this process's
    # first HIP call.  The draws from torch's global generator come in one order in every mode: the validation start (the test
    # loader's base seed, or --gpu_val's one substitute draw), the loaders' construction, next(iter(raw[0])), then the training.
    val = Validation(args, data_root) if rank == 0 else None        # rank 0 validates
    # DataLoader workers per domain loader: the reference's 8 (train.py:558) on one GPU; under torchrun every rank has its own
    # three loaders, so the host's cores are divided among ranks x domains (8 ranks x 3 x 8 = 192 decoder processes otherwise)
    domain_idx_list = [int(i) for i in args.domain_idxs.split(',')]
    preload_workers = max(1, worker_cap(args.num_workers, world, 1))     # threads decoding the resident data (<= 16)
    args.num_workers = worker_cap(args.num_workers, world, len(domain_idx_list))
    host_group = init_process(world, local)
    os.makedirs(args.save_path, exist_ok=True)
    bsl = (fundus_batch_list if args.dataset == 'fundus' else prostate_batch_list)[args.test_domain_idx][:len(domain_idx_list)]
    raw, samplers, loaders, max_len = make_loaders(args, data_root, world, rank, bsl, domain_idx_list, replay=uses_ckpt(args))
    if uses_accum(args):
        accum_totals(args, max_len)                                  # a run with no complete window is refused here
    check_bn_recal(args, max_len)                                    # ... and a K beyond the epoch here
    resident = None
    if args.gpu_data:
        # decode once, keep the pixels on this GPU (ramdsir/gpu_data.py); the loaders above only draw
        from ramdsir import gpu_data
        t0 = time.time()
        resident = gpu_data.preload(args.dataset, [dl.dataset for dl in raw], workers=preload_workers)
        if rank == 0:
            print('gpu_data: %.2f GB resident, preloaded in %.1f s with %d threads' % (resident.nbytes / 1e9, time.time() - t0,
                                                                                       preload_workers))
    if val is not None:
        val.preload(preload_workers)
    modules, trainer, (H, W), total_iters = build_trainer(args, rank, raw, resident, bsl, max_len)
    # --avg_weights: the second bank, a copy of the initial model (rank-local under data parallelism, as the BatchNorm buffers are)
    avg = trainer.enable_avg_weights(*avg_settings(args)) if uses_avg(args) else None
    # --avg_bn_recal: the ring, the third set of BatchNorm buffers and the forward-only plan over the averaged weights (rank-local too)
    recal = trainer.enable_avg_bn_recal(args.avg_bn_recal) if uses_bn_recal(args) else None
    if recal is not None and rank == 0:
        print('avg_bn_recal: the last %d batches of an epoch in a ring of %.1f MB; %d BatchNorm sites re-estimated per pass'
              % (recal.K, recal.ring.buf.numel() * recal.ring.buf.element_size() / 1e6, recal.forward.n_sites))
    # --clip_grad_norm / --skip_nonfinite: the guarded tail replaces Adam + repack in the step; the shadows copy the initial buffers
    guard = trainer.enable_grad_guard(guard_max_norm(args)) if uses_guard(args) else None
    # the five optimizer flags: the grouped Adam replaces rd_adam_step in the step (under the guard's state word where both are on)
    if uses_optim(args):
        enable_optim(args, trainer, total_iters, rank)
    # --accum_steps: one rd_grad_accum launch behind every backward pass, the tail above behind every N-th (total_iters counts updates)
    accum = trainer.enable_grad_accum(args.accum_steps) if uses_accum(args) else None
    if accum is not None and rank == 0:
        print(accum_line(args.accum_steps, *accum_totals(args, max_len)))
    state_io = open_state(args, trainer, (bsl, domain_idx_list, H, W, total_iters), resume_state) if uses_ckpt(args) else None
    # --tb_hist: the range table over the arenas, the bucket limits, the output and the pinned buffer; no state of its own
    if uses_tb_hist(args):
        hist = trainer.enable_tb_hist(tb_hist_what(args))
        if rank == 0:
            print('tb_hist: %d histograms (%s) of %d buckets every %d iterations, %.1f MB copied per logging iteration'
                  % (hist.n, ','.join(hist.what), hist.n_limits, args.tb_hist, hist.copy_bytes / 1e6))
    if val is not None:
        val.bind(trainer)
        if avg is not None and val.mode != 'fused':
            print('avg_weights: the averaged model is maintained and written at the end, but not validated per epoch (that pass is the '
                  'fused forward of --gpu_val / --gpu_val_volumes with --fused_val)')
    log = TrainLog(args, trainer, rank, world * sum(bsl), guard)
    previous_best, iter_num, start_epoch, previous_best_avg = 0.0, 0, 0, 0.0
    if resume_state is not None:
        start_epoch, iter_num, previous_best = restore_host_side(args, resume_state['meta'], loaders, raw)
        if avg is not None:
            previous_best_avg = restore_avg_host_side(args, resume_state['meta'])
        resume_state = None
    epochs_here, stopped = 0, False
    for epoch in range(start_epoch, args.epochs):
        it_epoch = iter_num
        if rank == 0:
            print('\n==> Epoch %i, learning rate = %.6f' % (epoch, args.lr if iter_num == 0 else trainer.lr()))
        for m in modules:
            m.train()
        t_epoch = time.time()
        for sp in samplers:
            if sp is not None:
                sp.set_epoch(epoch)
        iter_num = train_epoch(args, trainer, loaders, resident, log, iter_num, recal, max_len)
        log.throughput(iter_num)
        torch.cuda.synchronize()
        t_train = time.time() - t_epoch
        if recal is not None:
            # the statistics of the averaged weights from this epoch's last batches, in front of everything that reads them below
            # (the _avg validation, model_avg_%.2f.pth) and, behind the last epoch, final_model_avg.pth
            recal.run_pass()
        # validation on the held-out domain + keep-best checkpoint rotation (train.py:331-350)
        avg_dice = val(modules[0], modules[1], epoch) if val is not None else None
        if world > 1:
            # every rank has finished its epoch (synchronize above) and none has entered the next step's all-reduce: the
            # other ranks wait HERE, on the host (gloo), while rank 0 validates with replica 0's BatchNorm statistics (what
            # nn.DataParallel evaluates, train.py:343) -- not inside an RCCL gradient exchange with a missing peer, which
            # spins their GPUs and, past the watchdog timeout, aborts the job
            dist.barrier(group=host_group)
        previous_best = keep_best(args.save_path, avg_dice, previous_best, modules)
        if avg is not None:
            # the averaged model behind the live one: its own CSV, its own keep-best rotation; the other ranks wait on the host again
            if val is not None:
                previous_best_avg = keep_best(args.save_path, val.averaged(avg, modules[0], modules[1], epoch), previous_best_avg, modules,
                                              averaged=avg)
            if world > 1:
                dist.barrier(group=host_group)
        if state_io is not None and args.ckpt_every and (epoch + 1) % args.ckpt_every == 0:
            meta = dict(
                epoch=epoch, iter_num=iter_num, previous_best=previous_best, rng=ckpt.host_rng_state(),
                cycles=[None if it is dl else it.state() for it, dl in zip(loaders, raw)],
                val_log_bytes=os.path.getsize(val_log_path(args)) if os.path.exists(val_log_path(args)) else 0, **state_meta(trainer))
            if avg is not None:
                avg_log = val_log_path(args, '_avg')
                meta['avg_weights'].update(previous_best_avg=previous_best_avg,
                                           val_log_bytes=os.path.getsize(avg_log) if os.path.exists(avg_log) else 0)
            state_io.snapshot(osp.join(args.save_path, 'last_state.pth'), meta)
        if rank == 0:
            t_all, n_img = time.time() - t_epoch, (iter_num - it_epoch) * log.imgs_per_iter
            print('epoch %d: training %.2f s (%.0f images/s), validation + checkpoint %.2f s (%.0f images/s over the whole epoch)'
                  % (epoch, t_train, n_img / max(t_train, 1e-9), t_all - t_train, n_img / max(t_all, 1e-9)))
        if args.max_iters and iter_num >= args.max_iters:
            break
        epochs_here += 1
        if args.stop_after_epochs and epochs_here >= args.stop_after_epochs and epoch + 1 < args.epochs:
            stopped = True                              # --stop_after_epochs: as a preempted job, no final_model.pth
            break
    if log.step_log:
        log.drain()                                         # the rows behind the last logging iteration
    if guard is not None and rank == 0:
        g = guard.read()
        print('grad_guard: %d of %d steps clipped, %d skipped' % (g['clipped'], g['steps'], g['skipped']))
    if state_io is not None:
        state_io.close()                                    # the last snapshot is durable
        if state_io.seconds['calls']:
            print(state_io.report())
    if stopped:
        print('\nStopped after %d epochs of this process (epoch %d of %d); resume from %s'
              % (epochs_here, epoch, args.epochs, osp.join(args.save_path, 'last_state.pth')))
    elif rank == 0:
        save_checkpoint(os.path.join(args.save_path, 'final_model.pth'), *modules)
        if avg is not None:
            if recal is not None:
                recal.run_pass()                            # once more, over the last epoch's batches: the same bits
            torch.save(dict(avg.state_dicts()), os.path.join(args.save_path, 'final_model_avg.pth'))
        print('\nSave Final Model to {}'.format(args.save_path))
    log.close()
    if val is not None:
        val.close()
    if world > 1:
        dist.barrier(group=host_group)


if __name__ == '__main__':
    args = parse_args()
    if 'LOCAL_RANK' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu                  # train.py:606
    if args.deterministic:
        r = int(os.environ.get('RANK', '0'))               # rank-local RAM partners / crops; weights are broadcast from rank 0
        random.seed(args.seed + r)
        np.random.seed(args.seed + r)
        torch.manual_seed(args.seed + r)
    if args.epochs is None:
        args.epochs = {'fundus': 400, 'prostate': 200}[args.dataset]
    if args.lr is None:
        args.lr = {'fundus': 2e-3, 'prostate': 1e-3}[args.dataset]
    if args.num_classes is None:
        args.num_classes = {'fundus': 2, 'prostate': 2}[args.dataset]
    print(args)
    main(args)
