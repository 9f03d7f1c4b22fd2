"""In-training Prostate validation on the GPU (train.py --gpu_val_volumes).

The held-out site's NIfTI volumes are read ONCE: the min-max normalised fp32 voxels (exactly the values the host path's 2.5-D batches
hold: utils.prostate_eval.normalise_volume, then float32), the ground truths (uint8, 0 / non-0) and the per-slice "ground truth is
empty" flags stay in device memory.  Per epoch and volume the batches of utils.prostate_eval.predict_volume are built on the device
(rd_vol_stack), go through the same modules, and the argmax with its suppression lands in a resident prediction volume
(rd_vol_argmax); the largest 6-connected component and the three counts of a Dice coefficient are rd_vol_post (csrc/val_volume.hip;
code/train.py:134-192, code/utils/utils.py:30-42 of the reference), and ONE device-to-host copy of the counts ends the pass.  The
Dice doubles are then evaluated on the host from integers with metrics.dc's formula, so equal volumes give equal numbers.

`stack_model`, `argmax_model` and `largest_component_model` state the kernels' rules in plain numpy: they are what the kernels are
read against, and the CPU suite pins them to predict_volume and to scipy.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ramdsir import _lib as L
from ramdsir._lib import _stream
from ramdsir.gpu_val import _run_index, _runs

MEM_SHARE = 0.5             # as ramdsir/gpu_val.py: at most this share of the device memory free at preload
POST_GROUP_VOXELS = 1 << 25  # volumes share one rd_vol_post call (and its 8 B / voxel of scratch) up to this many voxels


# ----------------------------------------------------------------------------------------------------------------------------------
# the numpy model
def frame_batches(D, batch_size):
    """The batches predict_volume runs for a volume of D slices: D // batch_size lists of exactly batch_size frame indices taken in
    order from 1 ... D - 2, -1 where the frame list has run out."""
    frames = list(range(1, D - 1))
    out = []
    for ii in range(D // batch_size):
        f = frames[ii * batch_size:(ii + 1) * batch_size]
        out.append(f + [-1] * (batch_size - len(f)))
    return out


def stack_model(volume, frames):
    """(D, H, W) float32, frame indices (-1: empty slot) -> (B, 3, H, W) float32: channel c of slot b is slice frames[b] - 1 + c."""
    v = np.asarray(volume, dtype=np.float32)
    out = np.zeros((len(frames), 3) + v.shape[1:], np.float32)
    for b, jj in enumerate(frames):
        if jj >= 0:
            out[b] = v[jj - 1:jj + 2]
    return out


def argmax_model(logits, frames, gt_empty, pred):
    """Writes slice frames[b] of pred (D, H, W) uint8: 1 where logits[b, 1] > logits[b, 0] (argmax over the class axis, the first
    maximum winning), all zeros where gt_empty[frames[b]] is set.  Empty slots write nothing."""
    lg = np.asarray(logits, dtype=np.float32)
    for b, jj in enumerate(frames):
        if jj < 0:
            continue
        pred[jj] = 0 if gt_empty[jj] else (lg[b, 1] > lg[b, 0]).astype(np.uint8)
    return pred


def _label_runs_3d(member):
    """Union-find over the runs along x of a boolean volume; the root of a component is its first run in (z, y, x) raster order.
    Runs connect through faces only: with the runs of row y - 1 of the same slice and of row y of slice z - 1 that overlap them in x.
    Returns (start, end, root per run) with the runs in raster order."""
    D, H, W = member.shape
    rows, start, end = _runs(member.reshape(D * H, W))
    n = len(rows)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                   # the smaller root wins
    first = np.searchsorted(rows, np.arange(D * H + 1)).tolist()
    st, en = start.tolist(), end.tolist()

    def join(ra, rb):
        a, b, a_end, b_end = first[ra], first[rb], first[ra + 1], first[rb + 1]
        while a < a_end and b < b_end:
            if st[a] < en[b] and st[b] < en[a]:
                union(a, b)
            if en[a] < en[b]:
                a += 1
            else:
                b += 1
    for r in range(D * H):
        if first[r] == first[r + 1]:
            continue
        if r % H:
            join(r - 1, r)
        if r >= H:
            join(r - H, r)
    return start, end, np.array([find(r) for r in range(n)], dtype=np.int64)


def largest_component_model(pred):
    """utils.metrics.connectivity_region_analysis without scipy: keep the largest 6-connected component of a 0 / 1 volume (ties: the
    one whose first voxel in raster order comes first); an EMPTY volume becomes all ones, the reference's `keep == 0`."""
    f = np.asarray(pred) != 0
    if f.ndim != 3:
        raise ValueError('largest_component_model takes a (D, H, W) volume; got %s' % (f.shape,))
    start, end, root = _label_runs_3d(f)
    if not len(root):
        return np.ones(f.shape, np.uint8)
    area = np.bincount(root, weights=end - start, minlength=len(root))
    win = int(np.argmax(area))                              # first maximum = smallest root among the largest
    D, H, W = f.shape
    idx = _run_index(f.reshape(D * H, W)).reshape(f.shape)
    return (f & (root[idx] == win)).astype(np.uint8)


def dice_from_counts(n_post, n_gt, n_inter):
    """metrics.dc's formula on integer counts (Python floats, the same doubles); 0.0 when both volumes are empty."""
    if n_post + n_gt == 0:
        return 0.0
    return 2.0 * n_inter / float(n_post + n_gt)


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
def _frames(frames):
    return (L.i32 * len(frames))(*[int(f) for f in frames])


def stack(volume, frames):
    """volume (D, H, W) fp32 on the device -> the batch (len(frames), 3, H, W) fp32 of predict_volume."""
    D, H, W = volume.shape
    out = torch.empty((len(frames), 3, H, W), dtype=torch.float32, device=volume.device)
    L.check(L.lib().rd_vol_stack(L.ptr(volume), D, H, W, _frames(frames), len(frames), L.ptr(out), _stream()), 'rd_vol_stack')
    return out


def stack_nhwc(volume, frames, out):
    """volume (D, H, W) fp32 on the device -> the batch of predict_volume straight into `out`, the NHWC storage-dtype input
    (len(frames), H, W, cstride) of an EvalForward plan (rd_vol_stack_nhwc: the bits rd_nchw_to_nhwc makes of stack())."""
    D, H, W = volume.shape
    if out.dtype not in (torch.float32, torch.bfloat16) or tuple(out.shape[:3]) != (len(frames), H, W) or not out.is_contiguous():
        raise ValueError('--fused_val: the plan input must be contiguous NHWC %s in fp32 / bf16; got %s %s'
                         % ((len(frames), H, W, 'cstride'), out.dtype, tuple(out.shape)))
    L.check(L.lib().rd_vol_stack_nhwc(L.ptr(volume), D, H, W, _frames(frames), len(frames), L.ptr(out),
                                      L.RD_BF16 if out.dtype == torch.bfloat16 else L.RD_F32, out.shape[3], _stream()), 'rd_vol_stack_nhwc')


def argmax_nhwc(logits, frames, gt_empty, pred, shape):
    """logits (B, H, W, cstride) fp32 / bf16 NHWC on the device -> the slices `frames` of pred (rd_vol_argmax_nhwc: argmax()'s bytes)."""
    D, H, W = shape
    if logits.dtype not in (torch.float32, torch.bfloat16) or tuple(logits.shape[:3]) != (len(frames), H, W) or logits.shape[3] < 2 \
            or not logits.is_contiguous():
        raise ValueError('--fused_val: expected contiguous NHWC logits %s in fp32 / bf16; got %s %s'
                         % ((len(frames), H, W, '>= 2'), logits.dtype, tuple(logits.shape)))
    L.check(L.lib().rd_vol_argmax_nhwc(L.ptr(logits), L.RD_BF16 if logits.dtype == torch.bfloat16 else L.RD_F32, logits.shape[3], len(frames),
                                       H, W, _frames(frames), L.ptr(gt_empty), D, L.ptr(pred), _stream()), 'rd_vol_argmax_nhwc')


def argmax(logits, frames, gt_empty, pred, shape):
    """logits (B, 2, H, W) fp32 on the device -> the slices `frames` of pred (a flat uint8 view of the (D, H, W) prediction)."""
    D, H, W = shape
    if logits.dtype != torch.float32 or tuple(logits.shape) != (len(frames), 2, H, W):
        raise ValueError('--gpu_val_volumes: the decoder must return fp32 logits %s; got %s %s'
                         % ((len(frames), 2, H, W), logits.dtype, tuple(logits.shape)))
    logits = logits.contiguous()
    L.check(L.lib().rd_vol_argmax(L.ptr(logits), len(frames), H, W, _frames(frames), L.ptr(gt_empty), D, L.ptr(pred), _stream()),
            'rd_vol_argmax')


def volume_records(shapes, offs=None, gt_offs=None, slots=None):
    """rd_val_volume_t records of ((d, h, w), ...): stored back to back in list order unless offs says where; the ground truths at
    gt_offs (default: the same offsets), counts rows `slots` (default: list order) -> (ctypes array, bytes of the packed buffer)."""
    arr = (L.RdValVolume * max(len(shapes), 1))()
    off = 0
    for i, (d, h, w) in enumerate(shapes):
        arr[i].off, arr[i].d, arr[i].h, arr[i].w = off if offs is None else int(offs[i]), int(d), int(h), int(w)
        arr[i].gt_off = arr[i].off if gt_offs is None else int(gt_offs[i])
        arr[i].slot = i if slots is None else int(slots[i])
        off += int(d) * int(h) * int(w)
    return arr, off


def post(pred, out, recs, n, gt=None, counts=None, workspace=None):
    """rd_vol_post over n records: pred -> out (distinct uint8 buffers with one layout); with gt and counts (int32 (slots, 3)) the
    volumes' |post|, |gt|, |post & gt| are added to counts.  workspace: a uint8 buffer to reuse, or None."""
    lib = L.lib()
    ws_bytes = lib.rd_vol_post_workspace(recs, n)
    if ws_bytes < 0:
        raise ValueError('--gpu_val_volumes: invalid volume records')
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=pred.device)
    L.check(lib.rd_vol_post(L.ptr(pred), L.ptr(out), min(pred.numel(), out.numel()), L.ptr(gt), 0 if gt is None else gt.numel(),
                            L.ptr(counts), 0 if counts is None else counts.shape[0], L.ptr(workspace), workspace.numel(), recs, n,
                            _stream()), 'rd_vol_post')
    return out


def zero(buf):
    """buf := 0 on the current stream (rd_zero)."""
    L.check(L.lib().rd_zero((L.vp * 1)(buf.data_ptr()), (L.i64 * 1)(buf.numel() * buf.element_size()), 1, _stream()), 'rd_zero')


def post_groups(shapes, limit=None):
    """Consecutive index ranges [a, b) of at most `limit` voxels each (a single larger volume is a group of its own)."""
    limit = POST_GROUP_VOXELS if limit is None else limit
    groups, a, vox = [], 0, 0
    for i, (d, h, w) in enumerate(shapes):
        m = d * h * w
        if i > a and vox + m > limit:
            groups.append((a, i))
            a, vox = i, 0
        vox += m
    if len(shapes) > a:
        groups.append((a, len(shapes)))
    return groups


class VolResident:
    """The volumes of one Prostate site in device memory: volumes[i] (D, H, W) fp32 normalised; gt, pred and post as uint8 buffers
    with the volumes back to back (offs); gt_empty[i] (D,) uint8; the file names in list order."""

    def __init__(self, volumes, gt, gt_empty, shapes, files, scratch_bytes):
        self.volumes, self.gt, self.gt_empty, self.shapes, self.files = volumes, gt, gt_empty, shapes, files
        self.offs = [0]
        for d, h, w in shapes:
            self.offs.append(self.offs[-1] + d * h * w)
        self.pred = torch.empty(max(self.offs[-1], 1), dtype=torch.uint8, device=gt.device)
        self.post = torch.empty_like(self.pred)
        self.nbytes = sum(v.numel() * 4 for v in volumes) + 3 * gt.numel() + sum(e.numel() for e in gt_empty)
        self.scratch_bytes = scratch_bytes

    def __len__(self):
        return len(self.shapes)


def _read_case(args):
    """One volume on the host: (normalised fp32 (D, H, W), ground truth != 0 as uint8, per-slice 'ground truth sums to 0' flags)."""
    from utils.prostate_eval import load_case, merge_labels, normalise_volume
    data_dir, domain_name, file_name = args
    image, mask = load_case(data_dir, domain_name, file_name)
    mask = merge_labels(mask)
    if np.asarray(image).ndim != 3 or mask.shape != np.asarray(image).shape:
        raise ValueError('--gpu_val_volumes: %s is %s, its segmentation %s' % (file_name, np.asarray(image).shape, mask.shape))
    # what torch.from_numpy(vol).float() makes of predict_volume's float64 batch array
    vol = torch.from_numpy(np.asarray(normalise_volume(image), dtype=np.float64)).float()
    empty = np.array([np.sum(mask[jj, ...]) == 0 for jj in range(mask.shape[0])], dtype=np.uint8)
    return vol, torch.from_numpy((mask != 0).astype(np.uint8)), torch.from_numpy(empty)


def _scratch_bytes(shapes, batch_size):
    """Largest rd_vol_post workspace of a pass plus the largest batch and its logits."""
    ws = max([8 * sum(d * h * w for d, h, w in shapes[a:b]) + 64 * (b - a) for a, b in post_groups(shapes)] or [0])
    return ws + max([batch_size * 5 * h * w * 4 for _, h, w in shapes] or [0])


def preload(data_dir, domain_name, batch_size=8, workers=8, device=None):
    """Reads the volumes of <data_dir>/<domain_name> once, with at most 16 threads, in utils.prostate_eval.volume_files' order, and
    keeps what validation needs on the device.  Returns None -- after printing one line -- when that would take more than half of
    the free device memory.  Touches no random state."""
    from utils.prostate_eval import volume_files
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    files = volume_files(data_dir, domain_name)
    nw = min(16, max(1, int(workers)))
    with ThreadPoolExecutor(max_workers=nw) as ex:
        cases = list(ex.map(_read_case, [(data_dir, domain_name, f) for f in files]))
    shapes = [tuple(int(s) for s in v.shape) for v, _, _ in cases]
    vox = sum(d * h * w for d, h, w in shapes)
    scratch = _scratch_bytes(shapes, batch_size)
    need = vox * (4 + 3) + sum(d for d, _, _ in shapes) + scratch
    free = torch.cuda.mem_get_info(device)[0]
    if need > MEM_SHARE * free:
        print('gpu_val_volumes: the resident volumes need %.2f GB, more than %d %% of the %.2f GB free on %s: validating on the host'
              % (need / 1e9, int(MEM_SHARE * 100), free / 1e9, device))
        return None
    gt = torch.empty(max(vox, 1), dtype=torch.uint8, device=device)
    volumes, gt_empty, off = [], [], 0
    for vol, g, empty in cases:
        volumes.append(vol.to(device))
        gt[off:off + g.numel()].copy_(g.reshape(-1))
        gt_empty.append(empty.to(device))
        off += g.numel()
    return VolResident(volumes, gt, gt_empty, shapes, files, scratch)


def validate(encoder, seg_decoder, res, batch_size=8, keep=None, forward=None):
    """One validation pass over the resident volumes: per volume the batches of predict_volume through the modules (eval mode,
    no_grad), then the post-processing of all volumes, one device-to-host copy.  Returns the Dice of every volume in list order.
    keep: a dict that receives the prediction and the post-processed volumes as numpy arrays (tests).  forward: an
    infer.EvalForward over the same parameters (--fused_val): refresh() once, then per batch rd_vol_stack_nhwc writes the plan's
    input, ONE rd_run_list call, rd_vol_argmax_nhwc reads the plan's logits in place -- the same volumes and counts."""
    n = len(res)
    counts = torch.zeros((max(n, 1), 3), dtype=torch.int32, device=res.gt.device)
    encoder.eval()                                          # fused too: the flags the module path leaves behind
    seg_decoder.eval()
    with torch.no_grad():
        if forward is not None:
            forward.refresh()
        zero(res.pred)                                      # slices that no batch reaches, and empty slots, stay zero
        for i in range(n):
            pred, (_, H, W) = res.pred[res.offs[i]:res.offs[i + 1]], res.shapes[i]
            for frames in frame_batches(res.shapes[i][0], batch_size):
                if forward is None:                         # the batch's forward pass: all that the two modes do not share
                    argmax(seg_decoder(encoder(stack(res.volumes[i], frames))), frames, res.gt_empty[i], pred, res.shapes[i])
                else:
                    stack_nhwc(res.volumes[i], frames, forward.input(len(frames), H, W))
                    argmax_nhwc(forward.run(len(frames), H, W), frames, res.gt_empty[i], pred, res.shapes[i])
        groups = [(volume_records(res.shapes[a:b], res.offs[a:b], slots=range(a, b))[0], b - a) for a, b in post_groups(res.shapes)]
        ws_bytes = max([L.lib().rd_vol_post_workspace(recs, m) for recs, m in groups] or [0])
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=res.gt.device)
        for recs, m in groups:
            post(res.pred, res.post, recs, m, res.gt, counts, workspace)
    c = counts.cpu().tolist()                               # the pass's only synchronisation
    if keep is not None:
        keep['pred'] = [res.pred[res.offs[i]:res.offs[i + 1]].cpu().numpy().reshape(res.shapes[i]) for i in range(n)]
        keep['post'] = [res.post[res.offs[i]:res.offs[i + 1]].cpu().numpy().reshape(res.shapes[i]) for i in range(n)]
        keep['counts'] = c
    return [dice_from_counts(*c[i]) for i in range(n)]


