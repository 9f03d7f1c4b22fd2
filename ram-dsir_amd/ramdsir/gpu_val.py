"""In-training Fundus validation on the GPU (train.py --gpu_val).

The held-out domain's test set is decoded ONCE: the normalised 256 x 256 inputs (exactly the tensors the host path's test loader
feeds the encoder) and the native-size targets (uint8 planes, packed back to back) stay in device memory.  Per epoch the forward
pass runs as in train.py::test_fundus; everything after it -- sigmoid, bilinear resize to the native mask size, the 0.75 threshold,
largest 8-connected component + hole filling, the three counts of a Dice coefficient -- is csrc/val_post.hip (rd_val_threshold,
rd_val_post; code/train.py:91-132, code/utils/utils.py:19-28,45-96 of the reference), and ONE device-to-host copy of the counts
ends the pass.  The Dice doubles are then evaluated on the host from integers with dice_coefficient_numpy's formula, so equal masks
give equal numbers.

`postprocess_model` and `resize_threshold_model` state the kernels' rules in plain numpy: they are what the kernels are read
against, and the CPU suite pins them to scipy and to F.interpolate.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from ramdsir import _lib as L
from ramdsir._lib import _stream

MEM_SHARE = 0.5             # as ramdsir/gpu_data.py: at most this share of the device memory free at preload
THRESHOLD = 0.75


# ----------------------------------------------------------------------------------------------------------------------------------
# the numpy model
def resize_threshold_model(logits, H, W):
    """(F.interpolate(sigmoid(logits), (H, W), mode='bilinear', align_corners=False) > 0.75) in float32 numpy, every operation
    rounded on its own.  logits: (..., h, w) float32 -> (..., H, W) uint8."""
    f32 = np.float32
    x = np.asarray(logits, dtype=f32)
    p = (f32(1) / (f32(1) + np.exp(-x))).astype(f32)
    h, w = x.shape[-2:]

    def axis(n_in, n_out):
        scale = f32(n_in) / f32(n_out)
        src = np.maximum(scale * (np.arange(n_out, dtype=f32) + f32(0.5)) - f32(0.5), f32(0))
        i0 = src.astype(np.int32)
        return i0, np.minimum(i0 + 1, n_in - 1), (src - i0.astype(f32)).astype(f32)
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    hx, hy = f32(1) - lx, (f32(1) - ly)[:, None]
    ly = ly[:, None]
    top = hx * p[..., y0, :][..., x0] + lx * p[..., y0, :][..., x1]
    bot = hx * p[..., y1, :][..., x0] + lx * p[..., y1, :][..., x1]
    return (hy * top + ly * bot > f32(THRESHOLD)).astype(np.uint8)


def resize_probability_f64(logits, H, W):
    """The same formula in float64 on the float32 source coordinates and weights: the 'exact' probability that decides which pixels
    may differ between two float32 implementations (those within a band around 0.75)."""
    f32 = np.float32
    x = np.asarray(logits, dtype=f32).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-x))
    h, w = x.shape[-2:]

    def axis(n_in, n_out):
        scale = f32(n_in) / f32(n_out)
        src = np.maximum(scale * (np.arange(n_out, dtype=f32) + f32(0.5)) - f32(0.5), f32(0))
        i0 = src.astype(np.int32)
        return i0, np.minimum(i0 + 1, n_in - 1), (src - i0.astype(f32)).astype(np.float64)
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    ly = ly[:, None]
    top = (1.0 - lx) * p[..., y0, :][..., x0] + lx * p[..., y0, :][..., x1]
    bot = (1.0 - lx) * p[..., y1, :][..., x0] + lx * p[..., y1, :][..., x1]
    return (1.0 - ly) * top + ly * bot


def _runs(member):
    """Horizontal runs of a boolean plane in raster order: (row, first column, end column (exclusive)) arrays."""
    H, W = member.shape
    pad = np.zeros((H, W + 2), np.int8)
    pad[:, 1:-1] = member
    d = np.diff(pad, axis=1)
    rows, start = np.nonzero(d == 1)
    _, end = np.nonzero(d == -1)
    return rows, start, end


def _label_runs(member, diagonal, border):
    """Union-find over the runs of `member`; the root of a component is its first run in raster order.  diagonal: runs of adjacent
    rows also connect when they only touch at a corner (8-connectivity).  border: an extra root -1 that every run touching the
    image border joins (and so do the runs connected to those).  Returns (rows, start, end, root per run)."""
    H, W = member.shape
    rows, start, end = _runs(member)
    n = len(rows)
    parent = list(range(n + 1))                             # node 0: the border; node r + 1: run r

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)                   # the smaller root wins
    first = np.searchsorted(rows, np.arange(H + 1)).tolist()
    reach = 1 if diagonal else 0
    st, en = start.tolist(), end.tolist()
    for y in range(H):
        if border:
            for r in range(first[y], first[y + 1]):
                if y == 0 or y == H - 1 or st[r] == 0 or en[r] == W:
                    union(r + 1, 0)
        if y == 0:
            continue
        a, b, a_end, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if st[a] < en[b] + reach and st[b] < en[a] + reach:
                union(a + 1, b + 1)
            if en[a] < en[b]:
                a += 1
            else:
                b += 1
    return rows, start, end, np.array([find(r + 1) - 1 for r in range(n)], dtype=np.int64)


def _run_index(member):
    """Per pixel, the index of the run it belongs to (valid where member is set)."""
    H, W = member.shape
    pad = np.zeros((H, W + 1), np.int8)
    pad[:, 1:] = member
    return (np.cumsum((np.diff(pad, axis=1) == 1).reshape(-1)) - 1).reshape(H, W)


def largest_fillhole_model(plane):
    """One plane: keep the largest 8-connected component (ties: the one whose first pixel in raster order comes first; an empty plane
    stays empty), then turn every background pixel that is not 4-connected to the image border into foreground."""
    f = np.asarray(plane) != 0
    rows, start, end, root = _label_runs(f, diagonal=True, border=False)
    kept = np.zeros(f.shape, bool)
    if len(root):
        area = np.bincount(root, weights=end - start, minlength=len(root))
        win = int(np.argmax(area))                          # first maximum = smallest root among the largest
        kept = f & (root[_run_index(f)] == win)
    bg = ~kept
    _, _, _, broot = _label_runs(bg, diagonal=False, border=True)
    if len(broot):
        kept = kept | (bg & (broot[_run_index(bg)] != -1))
    return kept.astype(np.uint8)


def postprocess_model(mask_u8):
    """utils.metrics.postprocess_binary without scipy: (2, H, W) uint8 0/1 -> (2, H, W) uint8; the planes are independent."""
    m = np.asarray(mask_u8)
    return np.stack([largest_fillhole_model(m[0]), largest_fillhole_model(m[1])]).astype(np.uint8)


def dice_from_counts(n_post, n_gt, n_inter):
    """dice_coefficient_numpy's formula on integer counts (Python floats, the same doubles)."""
    return (2 * float(n_inter) + 1.0) / (1.0 + float(n_post) + float(n_gt))


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
def image_records(sizes, gt_offs=None, slots=None):
    """rd_val_image_t records of images stored back to back in list order: ((h, w), ...) -> (ctypes array, bytes of the buffer)."""
    arr = (L.RdValImage * max(len(sizes), 1))()
    off = 0
    for i, (h, w) in enumerate(sizes):
        arr[i].off, arr[i].h, arr[i].w = off, int(h), int(w)
        arr[i].gt_off = 0 if gt_offs is None else int(gt_offs[i])
        arr[i].slot = i if slots is None else int(slots[i])
        off += 2 * int(h) * int(w)
    return arr, off


def threshold(logits, recs, n, nbytes):
    """Stage a: logits (n, 2, S, S) fp32 on the device -> packed uint8 masks of the records' native sizes."""
    if logits.dtype != torch.float32 or logits.dim() != 4 or logits.shape[0] != n or logits.shape[1] != 2:
        raise ValueError('--gpu_val: the decoder must return fp32 logits (B, 2, H, W); got %s %s' % (logits.dtype, tuple(logits.shape)))
    logits = logits.contiguous()
    mask = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=logits.device)
    L.check(L.lib().rd_val_threshold(L.ptr(logits), n, logits.shape[2], logits.shape[3], recs, L.ptr(mask), nbytes, _stream()),
            'rd_val_threshold')
    return mask


def threshold_nhwc(logits, recs, n, nbytes):
    """Stage a on the plan's own logits: (n, S, S, cstride) fp32 / bf16 NHWC on the device, channel 0 the cup and 1 the disc -> packed
    uint8 masks of the records' native sizes (rd_val_threshold_nhwc: the bits of threshold() on the fp32 NCHW copy)."""
    if logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() != 4 or logits.shape[0] != n or logits.shape[3] < 2 \
            or not logits.is_contiguous():
        raise ValueError('--fused_val: expected contiguous NHWC logits (B, H, W, >= 2) in fp32 / bf16; got %s %s' % (logits.dtype, tuple(logits.shape)))
    mask = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=logits.device)
    dt = L.RD_BF16 if logits.dtype == torch.bfloat16 else L.RD_F32
    L.check(L.lib().rd_val_threshold_nhwc(L.ptr(logits), dt, logits.shape[3], n, logits.shape[1], logits.shape[2], recs, L.ptr(mask), nbytes,
                                          _stream()), 'rd_val_threshold_nhwc')
    return mask


def post(mask, recs, n, nbytes, gt=None, counts=None):
    """Stages b and c: packed uint8 masks -> post-processed masks (a new buffer); with gt and counts (int32 (slots, 2, 3)) the
    planes' |post|, |gt|, |post & gt| are added to counts."""
    lib = L.lib()
    out = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=mask.device)
    ws_bytes = lib.rd_val_post_workspace(recs, n)
    if ws_bytes < 0:
        raise ValueError('--gpu_val: invalid image records')
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=mask.device)
    L.check(lib.rd_val_post(L.ptr(mask), L.ptr(out), nbytes, L.ptr(gt), 0 if gt is None else gt.numel(), L.ptr(counts),
                            0 if counts is None else counts.shape[0], L.ptr(ws), ws_bytes, recs, n, _stream()), 'rd_val_post')
    return out


class ValResident:
    """The test set of one Fundus domain in device memory: inputs (N, 3, S, S) fp32, targets as uint8 planes (2, h_i, w_i) packed
    back to back (gt, gt_offs), the native sizes, the ids in list order."""

    def __init__(self, inputs, gt, gt_offs, sizes, ids):
        self.inputs, self.gt, self.gt_offs, self.sizes, self.ids = inputs, gt, gt_offs, sizes, ids
        self.nbytes = inputs.numel() * 4 + gt.numel()
        self.inputs_nhwc = None                             # keep_nhwc(): the inputs as the fused forward reads them

    def __len__(self):
        return len(self.sizes)

    def keep_nhwc(self, dtype, cstride=None):
        """Also keep the inputs as NHWC [n][S][S][cstride] in the storage dtype `dtype` (cstride: default the channel count; channels
        past it are zero): converted ONCE by rd_nchw_to_nhwc, the conversion the Encoder module applies to every batch, so EvalForward's
        first conv sees the bits the module's sees (--fused_val).  Replaces an earlier copy."""
        n, c, S, S2 = self.inputs.shape
        cs = c if cstride is None else int(cstride)
        if self.inputs_nhwc is not None:
            self.nbytes -= self.inputs_nhwc.numel() * self.inputs_nhwc.element_size()
        out = torch.zeros((n, S, S2, cs), dtype=dtype, device=self.inputs.device)
        if n:
            L.check(L.lib().rd_nchw_to_nhwc(L.ptr(self.inputs), L.ptr(out), n, c, S, S2, cs, L.RD_BF16 if dtype == torch.bfloat16 else L.RD_F32,
                                            _stream()), 'rd_nchw_to_nhwc')
        self.inputs_nhwc = out
        self.nbytes += out.numel() * out.element_size()
        return out


def _mask_size(path):
    with Image.open(path) as im:
        return im.size


def preload(testset, workers=8, device=None, batch_size=8, nhwc_dtype=None):
    """Runs `testset` (dataset.fundus.Fundus, split 'test', Resize + Normalize) once, with at most 16 threads, and keeps what
    validation needs on the device.  Returns None -- after printing one line -- when that would take more than half of the free
    device memory.  The threads touch no global random state (the transforms of the test split draw nothing).
    nhwc_dtype (torch.float32 / torch.bfloat16; --fused_val): also keep the inputs in the layout EvalForward reads
    (ValResident.keep_nhwc); None keeps nothing more."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    n = len(testset)
    nw = min(16, max(1, int(workers)))
    with ThreadPoolExecutor(max_workers=nw) as ex:
        wh = list(ex.map(_mask_size, [os.path.join(testset.base_dir, l.split(' ')[1]) for l in testset.id_path]))
    sizes = [(h, w) for w, h in wh]
    S = 256
    px = sorted((h * w for h, w in sizes), reverse=True)
    scratch = sum(px[:batch_size]) * (2 + 2 + 16) + 64 * batch_size          # masks, post, parents + counts of the largest batch
    need = n * 3 * S * S * 4 + sum(2 * p for p in px) + scratch + (n * 3 * S * S * (2 if nhwc_dtype == torch.bfloat16 else 4) if nhwc_dtype is not None else 0)
    free = torch.cuda.mem_get_info(device)[0]
    if need > MEM_SHARE * free:
        print('gpu_val: the resident test set needs %.2f GB, more than %d %% of the %.2f GB free on %s: validating on the host'
              % (need / 1e9, int(MEM_SHARE * 100), free / 1e9, device))
        return None
    gt_offs, off = [], 0
    for h, w in sizes:
        gt_offs.append(off)
        off += 2 * h * w
    gt = torch.empty(max(off, 1), dtype=torch.uint8, device=device)
    inputs = None
    with ThreadPoolExecutor(max_workers=nw) as ex:
        for i, (img, _, orig, _) in enumerate(ex.map(testset.__getitem__, range(n))):
            if inputs is None:
                inputs = torch.empty((n,) + tuple(img.shape), dtype=torch.float32, device=device)
            if tuple(orig.shape) != (2,) + sizes[i]:
                raise ValueError('--gpu_val: target %d is %s, its file says %s' % (i, tuple(orig.shape), sizes[i]))
            inputs[i].copy_(img)
            gt[gt_offs[i]:gt_offs[i] + orig.numel()].copy_(orig.to(torch.uint8).reshape(-1))
    if inputs is None:
        inputs = torch.empty((0, 3, S, S), dtype=torch.float32, device=device)
    res = ValResident(inputs, gt, gt_offs, sizes, [l for l in testset.id_path])
    if nhwc_dtype is not None:
        res.keep_nhwc(nhwc_dtype)
    return res


def validate(encoder, seg_decoder, res, batch_size=8, keep=None, forward=None):
    """One validation pass over the resident set: the forward pass of train.py::test_fundus on batches of `batch_size` in list order,
    stages a-c per batch, one device-to-host copy.  Returns [(cup dice, disc dice)] per image.  keep: a list that receives
    (thresholded masks, post-processed masks, records) of every batch (tests).  forward: an infer.EvalForward over the same
    parameters (--fused_val): refresh() once, then per batch the resident NHWC slice is copied into the plan's input, ONE rd_run_list
    call, and stage a reads the plan's logits in place (rd_val_threshold_nhwc) -- the same masks and counts as through the modules."""
    n = len(res)
    S, S2 = res.inputs.shape[2:4]
    if forward is not None:
        x0 = forward.input(min(batch_size, max(n, 1)), S, S2)
        if res.inputs_nhwc is None or res.inputs_nhwc.dtype != x0.dtype or res.inputs_nhwc.shape[3] != x0.shape[3]:
            res.keep_nhwc(x0.dtype, x0.shape[3])            # (a resident set preloaded without nhwc_dtype, or for another layout)
    counts = torch.zeros((max(n, 1), 2, 3), dtype=torch.int32, device=res.inputs.device)
    encoder.eval()                                          # fused too: the flags the module path leaves behind
    seg_decoder.eval()
    with torch.no_grad():
        if forward is not None:
            forward.refresh()
        for b0 in range(0, n, batch_size):
            b1 = min(b0 + batch_size, n)
            recs, nbytes = image_records(res.sizes[b0:b1], res.gt_offs[b0:b1], range(b0, b1))
            if forward is None:                             # the forward pass and stage a: all that the two modes do not share
                mask = threshold(seg_decoder(encoder(res.inputs[b0:b1])), recs, b1 - b0, nbytes)
            else:
                forward.input(b1 - b0, S, S2).copy_(res.inputs_nhwc[b0:b1])
                mask = threshold_nhwc(forward.run(b1 - b0, S, S2), recs, b1 - b0, nbytes)
            out = post(mask, recs, b1 - b0, nbytes, res.gt, counts)
            if keep is not None:
                keep.append((mask, out, recs))
    c = counts.cpu().tolist()                               # the pass's only synchronisation
    return [(dice_from_counts(*c[i][0]), dice_from_counts(*c[i][1])) for i in range(n)]


