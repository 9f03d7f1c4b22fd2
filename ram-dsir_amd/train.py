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
(ramdsir/ckpt.py); the reference can only start from a fresh initialisation.
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


_VAL = {}


def _val_resources(data_dir, datasetTest, batch_size):
    """The test loader and the post-processing pool live across epochs: the reference rebuilds an 8-worker loader and
    post-processes every 800x800 prediction serially at every epoch (~0.2 s per image: connected components + hole filling) --
    seconds per epoch, invisible next to its training time, most of the wall clock next to this one's."""
    key = (data_dir, datasetTest, batch_size)
    if key not in _VAL:
        import multiprocessing as mp
        testset = Fundus(base_dir=data_dir, split='test', domain_idx=datasetTest,
                         transform=Compose([trans.Resize((256, 256)), trans.Normalize()]))
        nw = min(8, max(1, len(testset) // 2))
        loader = DataLoader(testset, batch_size=batch_size, num_workers=nw, shuffle=False, drop_last=False, pin_memory=True,
                            persistent_workers=True)
        pool = mp.get_context('fork').Pool(min(16, max(2, (os.cpu_count() or 4) // 4)))     # children never touch the GPU
        # a DataLoader forks its workers at the first iter(), not at construction: start them NOW (main() calls this before the
        # first GPU call), so that they too are forked from an address space that has never initialised HIP.  With
        # persistent_workers the DataLoader keeps this iterator (and its workers) and resets it at every later `for ... in loader`.
        it = iter(loader)
        _VAL[key] = (loader, pool, it)
    return _VAL[key][:2]


def _close_val():
    for loader, pool, it in _VAL.values():
        pool.terminate()
        pool.join()
        del it, loader                                      # persistent workers shut down with the loader's iterator
    _VAL.clear()


def test_fundus(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='fundus'):
    """train.py:91-132 (BN in eval mode here, as in the reference's in-training evaluation): sigmoid, bilinear resize to the
    native mask size, threshold 0.75, largest component + hole filling, Dice with +1 smoothing, one CSV line."""
    encoder.eval()
    seg_decoder.eval()
    loader, pool = _val_resources(data_dir, datasetTest, batch_size)
    cup = disc = 0.0
    n = 0
    pending = []
    with torch.no_grad():
        for data, target, target_orig, ids in loader:
            pred = torch.sigmoid(seg_decoder(encoder(data.cuda(non_blocking=True))))
            pred = torch.nn.functional.interpolate(pred, size=(target_orig.size(2), target_orig.size(3)), mode='bilinear')
            masks = (pred > 0.75).to(torch.uint8).cpu().numpy()                  # the threshold of postprocessing(), on the GPU
            tg = target_orig.to(torch.uint8).numpy()
            pending.append(pool.map_async(post_and_dice, [(masks[i], tg[i]) for i in range(masks.shape[0])]))
    for r in pending:
        for c, d in r.get():
            cup, disc, n = cup + c, disc + d, n + 1
    cup, disc = cup / max(n, 1), disc / max(n, 1)
    print('val_cup_dice : {}, val_disc_dice : {}'.format(cup, disc))
    with open(osp.join(output_path, str(datasetTest) + '_val_log.csv'), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['cup dice coefficence: '] + [cup] +
                                   ['disc dice coefficence: '] + [disc]])) + '\n')
    return (cup + disc) * 100.0 / 2


def _val_testset(data_dir, datasetTest):
    return Fundus(base_dir=data_dir, split='test', domain_idx=datasetTest, transform=Compose([trans.Resize((256, 256)), trans.Normalize()]))


_VAL_GPU = {}


def test_fundus_gpu(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='fundus', forward=None):
    """test_fundus with everything after the forward pass on the GPU (--gpu_val; ramdsir/gpu_val.py, csrc/val_post.hip): the same
    batches in list order through the same modules, the same CSV line, the same return value; Dice from integer counts, read back once.
    The resident test set is main()'s preload (or is made here at the first call).  forward (--fused_val): the infer.EvalForward that
    runs the forward pass instead of the modules."""
    from ramdsir import gpu_val
    key = (data_dir, datasetTest)
    if key not in _VAL_GPU:
        _VAL_GPU[key] = gpu_val.preload(_val_testset(data_dir, datasetTest), batch_size=batch_size)
        if _VAL_GPU[key] is None:
            raise RuntimeError('--gpu_val: the test set does not fit in device memory')
    dices = gpu_val.validate(encoder, seg_decoder, _VAL_GPU[key], batch_size, forward=forward)
    cup = disc = 0.0
    n = 0
    for c, d in dices:
        cup, disc, n = cup + c, disc + d, n + 1
    cup, disc = cup / max(n, 1), disc / max(n, 1)
    print('val_cup_dice : {}, val_disc_dice : {}'.format(cup, disc))
    with open(osp.join(output_path, str(datasetTest) + '_val_log.csv'), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['cup dice coefficence: '] + [cup] +
                                   ['disc dice coefficence: '] + [disc]])) + '\n')
    return (cup + disc) * 100.0 / 2


def test_prostate(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='prostate'):
    """train.py:134-192: Dice over the NIfTI volumes of the held-out site (BN in eval mode), one line in
    <target>_val_log.csv.  `data_dir` is the dataset directory (<data_root>/prostate)."""
    from utils.prostate_eval import DOMAIN_LIST, evaluate_domain
    encoder.eval()
    seg_decoder.eval()
    with torch.no_grad():
        val_dice, _, _ = evaluate_domain(lambda v: seg_decoder(encoder(v.cuda())), data_dir, DOMAIN_LIST[datasetTest], batch_size)
    print('val_dice : {}'.format(val_dice))
    with open(osp.join(output_path, str(datasetTest) + '_val_log.csv'), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['dice coefficence: '] + [val_dice]])) + '\n')
    return val_dice * 100.0


_VAL_VOL = {}


def test_prostate_gpu(encoder, seg_decoder, epoch, data_dir, datasetTest, output_path, batch_size=8, dataset='prostate', forward=None):
    """test_prostate on the resident volumes (--gpu_val_volumes; ramdsir/gpu_val_volumes.py, csrc/val_volume.hip): the same batches
    through the same modules, the same CSV line, the same return value; Dice from integer counts, read back once.  The resident
    volumes are main()'s preload (or are made here at the first call).  forward (--fused_val): the infer.EvalForward that runs the
    forward pass instead of the modules."""
    from ramdsir import gpu_val_volumes
    from utils.prostate_eval import DOMAIN_LIST
    key = (data_dir, datasetTest)
    if key not in _VAL_VOL:
        _VAL_VOL[key] = gpu_val_volumes.preload(data_dir, DOMAIN_LIST[datasetTest], batch_size=batch_size)
        if _VAL_VOL[key] is None:
            raise RuntimeError('--gpu_val_volumes: the volumes do not fit in device memory')
    val_dice = 0.0
    for d in gpu_val_volumes.validate(encoder, seg_decoder, _VAL_VOL[key], batch_size, forward=forward):
        val_dice += d
    val_dice = val_dice / max(len(_VAL_VOL[key]), 1)
    print('val_dice : {}'.format(val_dice))
    with open(osp.join(output_path, str(datasetTest) + '_val_log.csv'), 'a') as f:
        f.write(','.join(map(str, [['batch-size: '] + [batch_size] + [epoch] + ['dice coefficence: '] + [val_dice]])) + '\n')
    return val_dice * 100.0


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


def val_log_path(args):
    return osp.join(args.save_path, str(args.test_domain_idx) + '_val_log.csv')


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


def main(args):
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
    step_log = uses_step_log(args)
    if step_log and args.norm != 'bn':
        raise ValueError('--tb_every_iter / --tb_health read the fused step\'s device buffers: --norm %s trains through the modules, whose '
                         'losses are host-visible tensors (use --log_every 1 there)' % args.norm)
    if args.fused_val and args.norm != 'bn':
        raise ValueError('--fused_val freezes BatchNorm on its running statistics: --norm %s has none (validate through the modules)' % args.norm)
    ckpt_on = uses_ckpt(args)
    if args.ckpt_every < 0 or args.stop_after_epochs < 0:
        raise ValueError('--ckpt_every / --stop_after_epochs take a number of epochs, got %d / %d' % (args.ckpt_every, args.stop_after_epochs))
    if args.stop_after_epochs and not args.ckpt_every:
        raise ValueError('--stop_after_epochs leaves the run to be resumed: it needs --ckpt_every')
    if ckpt_on and args.norm != 'bn':
        raise ValueError('--ckpt_every / --resume / --stop_after_epochs snapshot the fused step\'s arenas: --norm %s trains through the modules, '
                         'whose Adam is torch\'s' % args.norm)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if ckpt_on and world > 1:
        raise ValueError('--ckpt_every / --resume / --stop_after_epochs run in one process: BatchNorm buffers, generators and replay lists '
                         'are rank-local (WORLD_SIZE=%d)' % world)
    resume_state = None
    if args.resume:
        from ramdsir import ckpt
        resume_state = ckpt.load_file(args.resume)          # an unknown format version or a corrupt range is refused here
    local = int(os.environ.get('LOCAL_RANK', '0'))
    data_root = os.path.join(args.data_root, args.dataset)
    # The validation pool (fork) and the persistent test loader -- with its worker processes started (_val_resources) -- are created
    # HERE, before the first GPU call of this process: their children are forked from an address space that has never initialised
    # HIP (rank 0 validates, below)
    has_val = args.dataset == 'fundus' and os.path.exists(os.path.join(data_root, 'Domain%d_test.list' % (args.test_domain_idx + 1)))
    if rank == 0 and has_val and args.gpu_val:
        # The host path starts its test loader's iterator at this point (_val_resources), and a DataLoader iterator takes one 64-bit
        # draw from torch's global generator for its base seed -- the generator the training samplers shuffle from.  --gpu_val creates
        # neither the loader nor the pool; it takes that one draw here, so that the trained model does not depend on the flag.
        torch.empty((), dtype=torch.int64).random_()
    elif rank == 0 and has_val:
        _val_resources(data_root, args.test_domain_idx, args.test_batch_size)
    # DataLoader workers per domain loader: the reference's 8 (train.py:558) on one GPU; under torchrun every rank has its own
    # three loaders, so the host's cores are divided among ranks x domains (8 ranks x 3 x 8 = 192 decoder processes otherwise)
    n_dom = len(args.domain_idxs.split(','))
    preload_workers = max(1, worker_cap(args.num_workers, world, 1))     # --gpu_data: threads decoding the resident data (<= 16)
    args.num_workers = worker_cap(args.num_workers, world, n_dom)
    torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    # host-side rendezvous (gloo) for the points where ranks wait for rank 0 on the CPU (validation): an RCCL barrier is a GPU
    # kernel that spins until every peer has arrived
    host_group = dist.new_group(backend='gloo') if world > 1 else None
    os.makedirs(args.save_path, exist_ok=True)

    bsl = fundus_batch_list[args.test_domain_idx] if args.dataset == 'fundus' else prostate_batch_list[args.test_domain_idx]
    domain_idx_list = [int(i) for i in args.domain_idxs.split(',')]
    raw, samplers, loaders, max_len = make_loaders(args, data_root, world, rank, bsl, domain_idx_list, replay=ckpt_on)
    resident = None
    if args.gpu_data:
        # decode once, keep the pixels on this GPU (ramdsir/gpu_data.py); the loaders above only draw
        from ramdsir import gpu_data
        t0 = time.time()
        resident = gpu_data.preload(args.dataset, [dl.dataset for dl in raw], workers=preload_workers)
        if rank == 0:
            print('gpu_data: %.2f GB resident, preloaded in %.1f s with %d threads' % (resident.nbytes / 1e9, time.time() - t0,
                                                                                       preload_workers))

    validate = test_fundus
    if rank == 0 and has_val and args.gpu_val:
        # the held-out test set, decoded once and kept on this GPU (ramdsir/gpu_val.py); the host path if it does not fit
        from ramdsir import gpu_val
        t0 = time.time()
        nhwc = None
        if args.fused_val:                                  # the inputs also in the layout and dtype the fused forward reads
            from ramdsir import modules
            nhwc = modules.storage_dtype()
        val_set = gpu_val.preload(_val_testset(data_root, args.test_domain_idx), workers=preload_workers, batch_size=args.test_batch_size,
                                  nhwc_dtype=nhwc)
        if val_set is not None:
            _VAL_GPU[(data_root, args.test_domain_idx)] = val_set
            validate = test_fundus_gpu
            print('gpu_val: %d test images, %.3f GB resident%s, preloaded in %.1f s'
                  % (len(val_set), val_set.nbytes / 1e9, '' if nhwc is None else ' (%.3f GB of it the NHWC %s inputs of --fused_val)'
                     % (val_set.inputs_nhwc.numel() * val_set.inputs_nhwc.element_size() / 1e9, 'bf16' if nhwc == torch.bfloat16 else 'fp32'),
                     time.time() - t0))
        else:
            rng_state = torch.get_rng_state()               # the loader's draw has been taken above
            _val_resources(data_root, args.test_domain_idx, args.test_batch_size)
            torch.set_rng_state(rng_state)

    validate_prostate = test_prostate
    if rank == 0 and args.gpu_val_volumes and args.num_classes != 2:
        # the host path sums the class indices of a component (ndi.sum(mask, ...)); the kernels count voxels: two classes only
        print('gpu_val_volumes: --num_classes %d is not 2: validating on the host' % args.num_classes)
    elif rank == 0 and args.gpu_val_volumes:
        # the held-out site's volumes, read once and kept on this GPU (ramdsir/gpu_val_volumes.py); the host path if they do not fit.
        # The host path creates no loader for Prostate, so there is no random draw to reproduce here.
        from ramdsir import gpu_val_volumes
        from utils.prostate_eval import DOMAIN_LIST
        if os.path.isdir(os.path.join(data_root, DOMAIN_LIST[args.test_domain_idx])):
            t0 = time.time()
            vols = gpu_val_volumes.preload(data_root, DOMAIN_LIST[args.test_domain_idx], batch_size=args.test_batch_size, workers=preload_workers)
            if vols is not None:
                _VAL_VOL[(data_root, args.test_domain_idx)] = vols
                validate_prostate = test_prostate_gpu
                print('gpu_val_volumes: %d volumes, %.3f GB resident + %.3f GB scratch, preloaded in %.1f s'
                      % (len(vols), vols.nbytes / 1e9, vols.scratch_bytes / 1e9, time.time() - t0))

    encoder = Encoder(c=args.in_channels, norm=args.norm, activation=args.activation).cuda()
    seg_decoder = Decoder(num_classes=args.num_classes, norm=args.norm, activation=args.activation).cuda()
    rec_decoder = Rec_Decoder(num_classes=args.in_channels, norm='dsbn', activation=args.activation,
                              num_domains=len(domain_idx_list)).cuda()
    print('\nEncoder Params: %.3fM' % count_params(encoder))
    print('\nSeg Decoder Params: %.3fM' % count_params(seg_decoder))
    print('\nRec Decoder Params: %.3fM' % count_params(rec_decoder))

    from ramdsir.trainer import FusedTrainer, ModuleTrainer
    sample = next(iter(raw[0]))
    H, W = resident.hw if resident is not None else sample[0].shape[1:3]
    total_iters = max_len * args.epochs
    cons = args.consistency_type if args.consistency else None
    assert cons in (None, 'mse', 'kd'), args.consistency_type
    # --norm bn (the reference's default): the fused HIP step.  gn / in: the reference's own loop over the drop-in modules (the fused step
    # keeps the statistics groups of the shared BatchNorms and of the restoration decoder's DSBN in one launch list: bn only)
    Trainer = FusedTrainer if args.norm == 'bn' else ModuleTrainer
    if args.norm != 'bn' and rank == 0:
        print('norm=%s: module-level training loop (torch autograd between the HIP modules)' % args.norm)
    trainer = Trainer(encoder, seg_decoder, rec_decoder, bsl[:len(domain_idx_list)], H, W, dataset=args.dataset,
                           consistency=cons, lambda_rec=args.lambda_rec, lr=args.lr, total_iters=total_iters,
                           dtype=torch.bfloat16 if (args.dtype or ('bf16' if args.norm == 'bn' else 'f32')) == 'bf16' else torch.float32)

    state_io = None
    if ckpt_on:
        # the trainer's ranges, the staging buffers and the writer thread, once (ramdsir/ckpt.py); --resume: the arenas, the BatchNorm
        # buffers and the schedule counter from the file (the host side follows immediately before the epoch loop)
        from ramdsir import ckpt
        state_io = ckpt.TrainState(trainer, ckpt.fingerprint(args, trainer, bsl[:len(domain_idx_list)], domain_idx_list, H, W, total_iters))
        if resume_state is not None:
            state_io.restore(resume_state)
        if not args.gpu_data and args.num_workers > 0:
            print('ckpt: model, optimizer and schedule state are restored exactly; with DataLoader worker processes the draws come from '
                  'freshly seeded workers (use --gpu_data or --num_workers 0 for a bit-identical continuation)')

    if rank == 0 and args.fused_val:
        # the validation forward pass as one launch list over the trainer's own parameter arena (ramdsir/infer.py); only where the
        # resident validation is in use (a test set that did not fit validates on the host, through the modules)
        if validate is test_fundus_gpu or validate_prostate is test_prostate_gpu:
            import functools
            from ramdsir.infer import EvalForward
            fused_forward = EvalForward.from_trainer(trainer)
            validate = functools.partial(test_fundus_gpu, forward=fused_forward) if validate is test_fundus_gpu else validate
            validate_prostate = functools.partial(test_prostate_gpu, forward=fused_forward) if validate_prostate is test_prostate_gpu \
                else validate_prostate
            print('fused_val: validation forward as one launch list per batch, %s storage, %s' % (
                'bf16' if fused_forward.dtype == torch.bfloat16 else 'fp32',
                'its own weight pack (one repack per pass)' if fused_forward.owns_pack else "the step's weight pack (no repack)"))
        else:
            print('fused_val: the resident validation is not in use: validating through the modules')

    # --tb_images: one writer thread owns the event file (scalars go through its queue too, so the records keep the order of the
    # calls); without the flag the direct writer, record for record what it always wrote
    Writer = QueuedWriter if args.tb_images else SummaryWriter
    writer = Writer(os.path.join(args.save_path, 'log')) if rank == 0 else None      # train.py:538
    first_bad = []
    if step_log:
        # --tb_every_iter / --tb_health: every step appends one row to a device-resident ring (FusedTrainer.enable_step_log)
        trainer.enable_step_log(health=args.tb_health)

    def write_step_log():
        """Drain the ring (collective; synchronises) and write its records in iteration order, with the drain's wall time."""
        records = trainer.drain_step_log()
        now = time.time()
        for rec in records if rank == 0 else ():
            pairs = step_log_pairs(rec, args.tb_every_iter, args.tb_health, args.log_every)
            if pairs:
                writer.add_scalars_at(rec['iteration'], pairs, walltime=now)
            if args.tb_health and not first_bad and not record_is_finite(rec):
                first_bad.append(rec['iteration'])
                print('tb_health: iteration %d is the first with non-finite values (%d non-finite gradient elements, loss %r); the run '
                      'continues' % (rec['iteration'], rec['nonfinite'], rec['losses']['loss']))
        return records

    previous_best, iter_num = 0.0, 0
    t_mark, it_mark, imgs_per_iter = None, 0, world * sum(bsl[:len(domain_idx_list)])
    start_epoch, epochs_here, stopped = 0, 0, False
    if resume_state is not None:
        # the host side of the snapshot, behind every start-up draw (the loaders' construction, next(iter(raw[0])), the --gpu_val draw):
        # the three generators and the cycles as the snapshotted process left them at the end of its epoch
        meta = resume_state['meta']
        ckpt.set_host_rng_state(meta['rng'])
        for idx, st in enumerate(meta['cycles']):
            if (st is None) != (loaders[idx] is raw[idx]):
                raise ValueError('--resume: the snapshot cycles other loaders than this run (domain %d)' % idx)
            if st is not None:
                loaders[idx] = ckpt.ReplayCycle.from_state(st)
        start_epoch, iter_num, previous_best = meta['epoch'] + 1, meta['iter_num'], meta['previous_best']
        if os.path.exists(val_log_path(args)) and os.path.getsize(val_log_path(args)) > meta['val_log_bytes']:
            print('resume: %s truncated from %d to %d bytes (lines of epochs that ran after the snapshot and run again)'
                  % (val_log_path(args), os.path.getsize(val_log_path(args)), meta['val_log_bytes']))
            with open(val_log_path(args), 'r+b') as f:
                f.truncate(meta['val_log_bytes'])
        print('resume: %s, continuing at epoch %d (iteration %d, best %.2f)' % (args.resume, start_epoch, iter_num, previous_best))
        resume_state = meta = None
    for epoch in range(start_epoch, args.epochs):
        it_epoch = iter_num
        if rank == 0:
            print('\n==> Epoch %i, learning rate = %.6f' % (epoch, args.lr if iter_num == 0 else trainer.lr()))
        for m in (encoder, seg_decoder, rec_decoder):
            m.train()
        t_epoch = time.time()
        for sp in samplers:
            if sp is not None:
                sp.set_epoch(epoch)
        def on_device(batches):
            if resident is not None:                    # --gpu_data: one rd_fundus_batch / rd_prostate_batch launch
                return resident.on_device(batches)
            return tuple(torch.cat([b[k] for b in batches], 0).cuda(non_blocking=True) for k in range(4))       # src, trg, lam, mask

        # one batch of look-ahead: the step of batch i also mixes batch i+1 (RAM) in its tail, beside Adam and the weight repack
        # (FusedTrainer.step next_batch; the last iteration of an epoch -- or of --max_iters -- has no successor and runs the
        # classical step)
        stream_it = iter(zip(*loaders))
        cur = next(stream_it, None)
        cur = on_device(cur) if cur is not None else None
        i = -1
        while cur is not None:
            i += 1
            nxt = next(stream_it, None)
            last = nxt is None or bool(args.max_iters and iter_num + 1 >= args.max_iters)
            nxt = None if last else on_device(nxt)
            log_images = rank == 0 and args.tb_images > 0 and iter_num % args.tb_images == 0      # train.py:306, 475
            if log_images:
                trainer.arm_tb_images()                 # this step also composes the grids of its batch and starts their copy
            trainer.step(*cur, next_batch=nxt)
            cur = nxt
            log_now = iter_num % args.log_every == 0
            if step_log:
                # the step has appended its row to the device ring; read the ring where the loop synchronises anyway (the logging
                # iterations), in front of image records (they follow the scalars of their own iteration) and when it is full --
                # all functions of iter_num alone, so every rank drains at the same iterations (the drain is collective)
                if log_now or (args.tb_images > 0 and iter_num % args.tb_images == 0) or trainer.step_log_full():
                    records = write_step_log()
                    if rank == 0 and log_now:           # printed and written from the same drained row
                        print(console_line(iter_num, records[-1]['lr'], records[-1]['losses']))
            elif log_now:
                l = trainer.losses()                    # collective when world > 1: the mean over the ranks
                if rank == 0:
                    lr_now = trainer.lr()
                    print(console_line(iter_num, lr_now, l))
                    # the reference's scalars (train.py:298-304 / 467-473), at the iterations whose losses are read back
                    writer.add_scalars_at(iter_num, scalar_pairs(lr_now, l))
            if log_images:                              # behind the scalars of the iteration, in the reference's tag order
                writer.add_images_at(iter_num, trainer.take_tb_images())
            iter_num += 1
            if iter_num == 5:                           # end-to-end throughput (files -> DataLoader -> H2D -> step), start-up excluded
                torch.cuda.synchronize()
                t_mark, it_mark = time.time(), iter_num
            if args.max_iters and iter_num >= args.max_iters:
                break
        if t_mark is not None and iter_num > it_mark:
            torch.cuda.synchronize()
            if rank == 0:
                print('train throughput: %.1f images/s end to end (%d iterations of %d images, %d DataLoader workers per domain)'
                      % ((iter_num - it_mark) * imgs_per_iter / (time.time() - t_mark), iter_num - it_mark, imgs_per_iter, args.num_workers))
        torch.cuda.synchronize()
        t_train = time.time() - t_epoch
        # validation on the held-out domain + keep-best checkpoint rotation (train.py:331-350); skipped when the
        # evaluation data is not on disk (synthetic / smoke runs)
        avg_dice = None
        if rank == 0 and args.dataset == 'fundus' and os.path.exists(os.path.join(data_root, 'Domain%d_test.list' % (args.test_domain_idx + 1))):
            print('Test on target domain {}'.format(args.test_domain_idx))
            avg_dice = validate(encoder, seg_decoder, epoch, data_root, args.test_domain_idx, args.save_path, args.test_batch_size)
        elif rank == 0 and args.dataset == 'prostate':
            from utils.prostate_eval import DOMAIN_LIST
            if os.path.isdir(os.path.join(data_root, DOMAIN_LIST[args.test_domain_idx])):
                print('Test on target domain {}'.format(args.test_domain_idx))
                avg_dice = validate_prostate(encoder, seg_decoder, epoch, data_root, args.test_domain_idx, args.save_path, args.test_batch_size)
        if world > 1:
            # every rank has finished its epoch (synchronize above) and none has entered the next step's all-reduce: the
            # other ranks wait HERE, on the host (gloo), while rank 0 validates with replica 0's BatchNorm statistics (what
            # nn.DataParallel evaluates, train.py:343) -- not inside an RCCL gradient exchange with a missing peer, which
            # spins their GPUs and, past the watchdog timeout, aborts the job
            dist.barrier(group=host_group)
        if avg_dice is not None and avg_dice >= previous_best:
            if previous_best != 0:
                old = os.path.join(args.save_path, 'model_%.2f.pth' % previous_best)
                if os.path.exists(old):
                    os.remove(old)
            save_checkpoint(os.path.join(args.save_path, 'model_%.2f.pth' % avg_dice), encoder, seg_decoder, rec_decoder)
            previous_best = avg_dice
        if state_io is not None and args.ckpt_every and (epoch + 1) % args.ckpt_every == 0:
            state_io.snapshot(osp.join(args.save_path, 'last_state.pth'), dict(
                epoch=epoch, iter_num=iter_num, previous_best=previous_best, rng=ckpt.host_rng_state(),
                cycles=[None if it is dl else it.state() for it, dl in zip(loaders, raw)],
                val_log_bytes=os.path.getsize(val_log_path(args)) if os.path.exists(val_log_path(args)) else 0))
        if rank == 0:
            t_all, n_img = time.time() - t_epoch, (iter_num - it_epoch) * imgs_per_iter
            print('epoch %d: training %.2f s (%.0f images/s), validation + checkpoint %.2f s (%.0f images/s over the whole epoch)'
                  % (epoch, t_train, n_img / max(t_train, 1e-9), t_all - t_train, n_img / max(t_all, 1e-9)))
        if args.max_iters and iter_num >= args.max_iters:
            break
        epochs_here += 1
        if args.stop_after_epochs and epochs_here >= args.stop_after_epochs and epoch + 1 < args.epochs:
            stopped = True                              # --stop_after_epochs: as a preempted job, no final_model.pth
            break
    if step_log:
        write_step_log()                                # the rows behind the last logging iteration
    if state_io is not None:
        state_io.close()                                # the last snapshot is durable
        if state_io.seconds['calls']:
            print(state_io.report())
    if stopped:
        print('\nStopped after %d epochs of this process (epoch %d of %d); resume from %s'
              % (epochs_here, epoch, args.epochs, osp.join(args.save_path, 'last_state.pth')))
    elif rank == 0:
        save_checkpoint(os.path.join(args.save_path, 'final_model.pth'), encoder, seg_decoder, rec_decoder)
        print('\nSave Final Model to {}'.format(args.save_path))
    if writer is not None:
        writer.close()
        if args.tb_images and writer.seconds['calls']:
            sec, n = writer.seconds, writer.seconds['calls']
            print('tb_images: %d image records at %d iterations; writer thread per logging iteration: wait for the copy %.2f ms, PNG %.2f ms, '
                  'crc32c + framing %.2f ms, file write %.2f ms' % (sec['records'], n, 1e3 * sec['wait'] / n, 1e3 * sec['png'] / n,
                                                                    1e3 * sec['crc'] / n, 1e3 * sec['write'] / n))
    _close_val()
    _VAL_GPU.clear()
    _VAL_VOL.clear()
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
