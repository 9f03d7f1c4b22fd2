"""TensorBoard image summaries of the training loop (train.py --tb_images): the three-image grids the reference writes every 100
iterations (code/train.py:306-329 Fundus, :475-496 Prostate) -- input, RAM-mixed input, restored image, predictions, ground truth --
composed by ONE HIP entry point (rd_tb_grids, csrc/tb_grid.hip) straight from the buffers the training step already holds, copied to
pinned host memory behind an event, and handed to the event-file writer as finished uint8 HWC arrays.

The reference builds a grid with torchvision.utils.make_grid and hands the float CHW result to tensorboardX's add_image; neither package
is a dependency here and neither can be pinned, so their semantics are RESTATED (parity unpinned), the way utils/metrics.py restates
medpy.  What was chosen, and what `grid_model` below and the kernel both implement:

  * make_grid(t, nrow=3, padding=2, normalize, pad_value=0): a one-channel selection is replicated to three channels; ONE selected
    sample is returned as it is (H x W, no border: torchvision's single-image case); n > 1 samples give a zero-filled
    (H + 4) x (n (W + 2) + 2) grid with tile k at rows [2, 2 + H), columns [k (W + 2) + 2, k (W + 2) + 2 + W);
  * normalize=True: over the whole selection (scale_each=False), after the transform, in float32: lo / hi = min / max,
    v = (x - lo) / float32(max(float64(hi) - float64(lo), 1e-5)) -- torchvision's norm_ip: clamp_, sub_(low),
    div_(max(high - low, 1e-5)) -- a true division;
  * add_image: uint8(trunc(v * float32(255))) (tensorboardX make_np / make_image: `(x * 255).astype(uint8)`); v is in [0, 1] by
    construction; bf16 sources are widened to float32 first;
  * the label grids go through the 21 "pascal" colours of the reference's decode_segmap (code/utils/utils.py:285-336) as
    float32(float64(colour) / 255.0); a class outside the palette stays black; an argmax takes the lowest index on a tie (torch.max).
"""
import numpy as np
import torch

from . import _lib as L
from .range_table import stream_handle

PALETTE = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128],
                    [64, 0, 0], [192, 0, 0], [64, 128, 0], [192, 128, 0], [64, 0, 128], [192, 0, 128], [64, 128, 128],
                    [192, 128, 128], [0, 64, 0], [128, 64, 0], [0, 192, 0], [128, 192, 0], [0, 64, 128]], np.uint8)
assert len(PALETTE) == L.TB_PALETTE

# (tag, source, first channel, channels, normalize) in the reference's order; sources: img / img_freq = the two network inputs,
# rec = the restored image, pred = the soft prediction of the first pass, pred_class = its argmax through the palette,
# target = a plane of the multilabel mask, label = the int64 label map through the palette
TABLES = {
    'fundus': dict(samples=(0, 9, 4), grids=(                                       # train.py:306-329
        ('train/Image', 'img', 0, 3, True), ('train/Image_Freq', 'img_freq', 0, 3, True), ('train/Image_Rec', 'rec', 0, 3, True),
        ('train/Soft_Predicted_OC', 'pred', 0, 1, True), ('train/Soft_Predicted_OD', 'pred', 1, 1, True),
        ('train/GT_OC', 'target', 0, 1, False), ('train/GT_OD', 'target', 1, 1, False))),
    'prostate': dict(samples=(0, 7, 3), grids=(                                     # train.py:475-496
        ('train/Image', 'img', 1, 1, True), ('train/Image_Freq', 'img_freq', 1, 1, True), ('train/Image_Rec', 'rec', 1, 1, True),
        ('train/Predicted', 'pred_class', 0, None, False), ('train/GT', 'label', 0, 1, False))),
}


def selected_samples(dataset, B):
    """The reference's sample selection, clipped to the batch as Python slicing clips it: 0:9:4 (Fundus) / 0:7:3 (Prostate)."""
    return list(range(B))[slice(*TABLES[dataset]['samples'])]


def tags(dataset):
    return [g[0] for g in TABLES[dataset]['grids']]


def grid_shape(n, H, W):
    return (H, W) if n == 1 else (H + 4, n * (W + 2) + 2)


# ------------------------------------------------------------------------------------------------------------- the numpy model
def palette_values():
    return (PALETTE.astype(np.float64) / 255.0).astype(np.float32)


def grid_model(t, samples, c0=0, nc=3, transform=L.TB_IDENTITY, normalize=False, dtype=np.float32):
    """The uint8 (rows, columns, 3) grid rd_tb_grids writes, in numpy.  t: (N, C, H, W) float array (bf16 data already widened), or
    (N, H, W) integer labels for TB_LABEL; TB_ARGMAX takes the argmax over channels c0 .. c0 + nc.  dtype=np.float64 evaluates the
    arithmetic in double (the tests' measure of the float32 pipeline's own rounding)."""
    t = np.asarray(t)
    samples = list(samples)
    if not 1 <= len(samples) <= 3:
        raise ValueError('1 to 3 samples, got %d' % len(samples))
    if transform == L.TB_LABEL:
        sel = _palette_model(t[samples].astype(np.int64))
    elif transform == L.TB_ARGMAX:
        sel = _palette_model(np.argmax(t[samples, c0:c0 + nc], axis=1))          # numpy: the first maximum
    else:
        x = t[samples, c0:c0 + nc].astype(dtype)
        one = dtype(1)
        sel = {L.TB_IDENTITY: lambda v: v, L.TB_SIGMOID: lambda v: one / (one + np.exp(-v)), L.TB_TANH: np.tanh}[transform](x)
        sel = np.repeat(sel, 3, axis=1) if nc == 1 else sel
    sel = sel.astype(dtype)
    if normalize:
        lo, hi = sel.min(), sel.max()
        d = dtype(max(np.float64(hi) - np.float64(lo), 1e-5))
        sel = (sel - lo) / d
    n, _, H, W = sel.shape
    gh, gw = grid_shape(n, H, W)
    grid = np.zeros((3, gh, gw), dtype)
    if n == 1:
        grid[:] = sel[0]
    else:
        for k in range(n):
            grid[:, 2:2 + H, k * (W + 2) + 2:k * (W + 2) + 2 + W] = sel[k]
    return np.trunc(np.clip(grid * dtype(255), 0, 255)).astype(np.uint8).transpose(1, 2, 0).copy()


def _palette_model(cls):
    """(n, H, W) classes -> (n, 3, H, W) float32 colours / 255; a class outside the palette stays black."""
    pal = np.concatenate([palette_values(), np.zeros((1, 3), np.float32)])
    idx = np.where((cls >= 0) & (cls < len(PALETTE)), cls, len(PALETTE))
    return pal[idx].transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------- descriptors
_ETYPE = {torch.float32: L.TB_F32, torch.bfloat16: L.TB_BF16, torch.int64: L.TB_I64}


def describe(tensor, layout, samples, c0, nc, transform, normalize, dst_ptr):
    """One rd_tb_grid_t for a device tensor.  layout: 'nhwc' (N, H, W, C -- the step's buffers, channel slot padded), 'nchw', or 'nhw'
    (labels); the strides are the tensor's own, so views (a batch half, a padded slot) need no copy."""
    if tensor.dtype not in _ETYPE:
        raise TypeError('rd_tb_grids reads float32, bfloat16 or int64 tensors, got %s' % tensor.dtype)
    st = tensor.stride()
    if layout == 'nhwc':
        (N, H, W, Cc), (sn, sh, sw, sc) = tensor.shape, st
    elif layout == 'nchw':
        (N, Cc, H, W), (sn, sc, sh, sw) = tensor.shape, st
    elif layout == 'nhw':
        (N, H, W), (sn, sh, sw), Cc, sc = tensor.shape, st, 1, 0
    else:
        raise ValueError(layout)
    if transform in (L.TB_ARGMAX, L.TB_LABEL) and (nc > L.TB_PALETTE or normalize):
        raise ValueError('the palette has %d colours, got %d classes' % (L.TB_PALETTE, nc) if nc > L.TB_PALETTE
                         else 'palette grids are not normalised')
    if (transform == L.TB_LABEL) != (tensor.dtype == torch.int64) or (transform != L.TB_ARGMAX and nc not in (1, 3)):
        raise ValueError('transform %d does not fit a %s source with %d channels' % (transform, tensor.dtype, nc))
    samples = list(samples)
    if not 1 <= len(samples) <= 3 or min(samples) < 0 or max(samples) >= N or c0 < 0 or c0 + nc > Cc:
        raise ValueError('selection %s, channels %d:%d out of a tensor of %s' % (samples, c0, c0 + nc, tuple(tensor.shape)))
    g = L.RdTbGrid()
    g.src, g.dst = tensor.data_ptr(), dst_ptr
    g.stride_n, g.stride_c, g.stride_h, g.stride_w = sn, sc, sh, sw
    g.etype, g.H, g.W, g.n = _ETYPE[tensor.dtype], H, W, len(samples)
    for k, s in enumerate(samples):
        g.sample[k] = s
    g.c0, g.nc, g.transform, g.normalize = c0, nc, transform, int(bool(normalize))
    return g


def compose(specs, out, workspace, stream=None):
    """rd_tb_grids over `specs` = [(tensor, layout, samples, c0, nc, transform, normalize)], the grids packed back to back into the
    uint8 device tensor `out`.  Returns [(byte offset, rows, columns)].  Asynchronous on the current stream."""
    if not 1 <= len(specs) <= L.TB_MAX_GRIDS:
        raise ValueError('1 to %d grids per call, got %d' % (L.TB_MAX_GRIDS, len(specs)))
    arr, layout, off = (L.RdTbGrid * len(specs))(), [], 0
    for i, (t, lay, samples, c0, nc, tr, norm) in enumerate(specs):
        arr[i] = describe(t, lay, samples, c0, nc, tr, norm, out.data_ptr() + off)
        gh, gw = grid_shape(arr[i].n, arr[i].H, arr[i].W)
        layout.append((off, gh, gw))
        off += gh * gw * 3
    lib = L.lib()
    if off > out.numel() or out.dtype != torch.uint8 or workspace.numel() * workspace.element_size() < lib.rd_tb_grids_workspace(len(specs)):
        raise ValueError('output (%d bytes needed) or workspace too small' % off)
    L.check(lib.rd_tb_grids(arr, len(specs), workspace.data_ptr(), workspace.numel() * workspace.element_size(), stream_handle(stream)),
            'rd_tb_grids')
    return layout


class Pending:
    """The grids of one logging iteration on their way to the host: `images()` waits for the copy's event (in the writer thread)
    and returns [(tag, uint8 (rows, columns, 3) array)]."""

    def __init__(self, tag_list, layout, host, event):
        self.tags, self.layout, self.host, self.event = tag_list, layout, host, event

    def images(self):
        self.event.synchronize()
        a = self.host.numpy()
        return [(tag, a[off:off + gh * gw * 3].reshape(gh, gw, 3)) for tag, (off, gh, gw) in zip(self.tags, self.layout)]

    __call__ = images


class GridComposer:
    """The device output buffer, the workspace and the staging of one trainer's grids (fixed geometry: dataset, batch, H, W).
    `enqueue(sources)` composes every tag of the dataset's table from `sources` = {name: (tensor, layout, transform)} and starts the
    copy into a pinned host buffer of its own (torch's caching host allocator recycles it once the writer has dropped it)."""

    def __init__(self, dataset, B, H, W, num_classes, device):
        if num_classes > L.TB_PALETTE:
            raise ValueError('the palette of the label grids has %d colours; got %d classes' % (L.TB_PALETTE, num_classes))
        self.dataset, self.K = dataset, num_classes
        self.samples = selected_samples(dataset, B)
        self.grids = TABLES[dataset]['grids']
        gh, gw = grid_shape(len(self.samples), H, W)
        self.out = torch.zeros(len(self.grids) * gh * gw * 3, dtype=torch.uint8, device=device)
        self.ws = torch.zeros(L.lib().rd_tb_grids_workspace(len(self.grids)) // 4, dtype=torch.float32, device=device)

    def specs(self, sources):
        out = []
        for tag, name, c0, nc, norm in self.grids:
            t, lay, tr = sources[name]
            out.append((t, lay, self.samples, c0, self.K if nc is None else nc, tr, norm))
        return out

    def enqueue(self, sources):
        layout = compose(self.specs(sources), self.out, self.ws)
        n = layout[-1][0] + layout[-1][1] * layout[-1][2] * 3
        host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        host.copy_(self.out[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return Pending([g[0] for g in self.grids], layout, host, ev)


def train_step_sources(ts, slot):
    """The five sources in a step.TrainStep's own buffers: the network input of input slot `slot` ([img ; img_freq], NHWC with the
    channel vector padded to one 16-byte slot), the logits of the first pass and of the restoration decoder (the transforms the
    reference applies before it logs them happen in the kernel), the target buffer."""
    B, x = ts.B, ts.xbufs[slot]
    fundus = ts.dataset == 'fundus'
    return {'img': (x[:B], 'nhwc', L.TB_IDENTITY), 'img_freq': (x[B:], 'nhwc', L.TB_IDENTITY),
            'rec': (ts.rec_logits.buf, 'nhwc', L.TB_TANH),
            'pred': (ts.logits.buf[:B], 'nhwc', L.TB_SIGMOID), 'pred_class': (ts.logits.buf[:B], 'nhwc', L.TB_ARGMAX),
            'target': (ts.target, 'nchw' if fundus else 'nhw', L.TB_IDENTITY), 'label': (ts.target, 'nhw', L.TB_LABEL)}


def module_sources(img, img_freq, soft1, rec_soft, target):
    """The tensors the module-level trainer holds (NCHW fp32; the probabilities are already transformed)."""
    lab = target.dim() == 3
    return {'img': (img, 'nchw', L.TB_IDENTITY), 'img_freq': (img_freq, 'nchw', L.TB_IDENTITY), 'rec': (rec_soft, 'nchw', L.TB_IDENTITY),
            'pred': (soft1, 'nchw', L.TB_IDENTITY), 'pred_class': (soft1, 'nchw', L.TB_ARGMAX),
            'target': (target, 'nhw' if lab else 'nchw', L.TB_IDENTITY), 'label': (target, 'nhw', L.TB_LABEL)}
