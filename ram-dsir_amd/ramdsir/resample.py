"""Pillow's 8-bit resampling as integer tables (host side of csrc/augment.hip).

Image.resize(BILINEAR) on an 8-bit image is pure integer arithmetic once its per-axis coefficient tables exist
(Pillow src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc): a horizontal pass rounded to uint8,
then a vertical pass over that, each output value clamp((2^21 + sum px * k) >> 22, 0, 255), a pass whose size does not
change skipped (the table of an unchanged size is the identity, so applying it changes nothing either).  NEAREST
indices are taken from Pillow itself (its affine walk accumulates x += scale in double; a closed formula differs at
the edges), one table per axis.  The numpy passes here are the reference the kernel is tested against.
"""
import numpy as np
from PIL import Image

PRECISION_BITS = 22                                 # 32 - 8 - 2 (Resample.c)
HALF = 1 << (PRECISION_BITS - 1)


def bilinear_coeffs(n_in, n_out):
    """(xmin int32[n_out], cnt int32[n_out], k int32[n_out, ksize]): output i = sum_{t < cnt[i]} in[xmin[i] + t] * k[i, t]."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs * 1.0                              # bilinear filter support 1
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    i = np.arange(n_out, dtype=np.float64)
    center = (i + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    cnt = xmax - xmin
    w = np.zeros((n_out, ksize), np.float64)
    ww = np.zeros(n_out, np.float64)
    for t in range(ksize):                          # tap by tap: the C loop's summation order (numpy's sum is pairwise)
        live = t < cnt
        v = np.maximum(1.0 - np.abs((t + xmin - center + 0.5) * ss), 0.0)
        v = np.where(live, v, 0.0)
        w[:, t] = v
        ww = ww + v
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    f = w * float(1 << PRECISION_BITS)
    k = np.where(w < 0, np.trunc(-0.5 + f), np.trunc(0.5 + f)).astype(np.int32)
    return xmin.astype(np.int32), cnt.astype(np.int32), k


def nearest_index(n_in, n_out, axis):
    """Source index of every output position of Image.resize(NEAREST) along `axis` (0 = x / width, 1 = y / height)."""
    a = np.arange(n_in, dtype=np.int32)
    im = Image.fromarray(a[None, :] if axis == 0 else a[:, None])
    size = (n_out, 1) if axis == 0 else (1, n_out)
    return np.asarray(im.resize(size, Image.NEAREST), dtype=np.int32).reshape(-1)


def apply_pass(img, n_out, axis):
    """One integer pass of a uint8 (H, W[, C]) array along axis 1 (horizontal) or 0 (vertical)."""
    dim = 1 if axis == 0 else 0
    xmin, cnt, k = bilinear_coeffs(img.shape[dim], n_out)
    a = np.moveaxis(img.astype(np.int64), dim, 0)                           # resampled axis first
    acc = np.full((n_out,) + a.shape[1:], HALF, np.int64)
    for t in range(k.shape[1]):
        live = t < cnt
        idx = np.where(live, xmin + t, 0)
        kk = np.where(live, k[:, t], 0).reshape((n_out,) + (1,) * (a.ndim - 1))
        acc += a[idx] * kk
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, dim)


def resize_bilinear(img, w, h):
    """Image.fromarray(img).resize((w, h), BILINEAR) for a uint8 HWC / HW array, bit for bit."""
    out = img
    if w != img.shape[1]:
        out = apply_pass(out, w, 0)
    if h != img.shape[0]:
        out = apply_pass(out, h, 1)
    return out


def resize_nearest(img, w, h):
    """Image.fromarray(img).resize((w, h), NEAREST), through the two index tables."""
    return img[nearest_index(img.shape[0], h, 1)][:, nearest_index(img.shape[1], w, 0)]


# ------------------------------------------------------------------------------------------- device table layout
# One int32 table per (n_in, n_out, axis) at an offset of a flat buffer (csrc/augment.hip reads it):
#   [n_in, n_out, ksize, 0] xmin[n_out] cnt[n_out] k[n_out][ksize] nearest[n_out]
def axis_table(n_in, n_out, axis):
    xmin, cnt, k = bilinear_coeffs(n_in, n_out)
    head = np.array([n_in, n_out, k.shape[1], 0], np.int32)
    return np.concatenate([head, xmin, cnt, k.reshape(-1), nearest_index(n_in, n_out, axis)]).astype(np.int32)


def max_window(n_in, n_out, rows):
    """The most input positions `rows` consecutive outputs of the bilinear table (n_in -> n_out) read."""
    xmin, cnt, _ = bilinear_coeffs(n_in, n_out)
    rows = min(rows, n_out)
    end = xmin + cnt
    return int(np.max(end[rows - 1:] - xmin[:n_out - rows + 1]))


class TableSet:
    """Flat int32 buffer of axis tables, deduplicated by (n_in, n_out, axis)."""

    def __init__(self):
        self.parts, self.index, self.size = [], {}, 0

    def offset(self, n_in, n_out, axis):
        key = (int(n_in), int(n_out), int(axis))
        if key not in self.index:
            t = axis_table(*key)
            self.index[key] = self.size
            self.parts.append(t)
            self.size += t.size
        return self.index[key]

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.int32)
