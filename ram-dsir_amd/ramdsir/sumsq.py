"""The numpy model of the fixed-order sum of squares (csrc/sumsq_pass.h: rdsum::chunk, rdsum::fold), in the kernels' summation order:
what rd_grad_guard (ramdsir/guard.py) and the health pass of rd_step_log (ramdsir/step_log.py) compute, bit for bit.

    partial_sums(grad, align_words)   the {sum, count} records of the first launch over ONE group, chunks counted from its start
    fold(sums)                        the second launch's sum of those records
"""
import numpy as np

from . import _lib as L

CHUNK, THREADS, QUADS = L.LOG_CHUNK, 256, L.LOG_CHUNK // 4 // 256
_LANE = np.arange(64)


def lanes_sum(v):
    """The xor tree over the 64 lanes (last axis) as the kernels run it: offsets 32, 16, ..., 1; every lane ends with the same bits."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v[..., 0]


def chunk_sums(x, head):
    """x: float32 [C][len], C chunks of one length; head: words in front of the first 16-byte boundary.  The fp64 sum of squares of
    each chunk's finite elements in the order of the first launch: per thread the head word, its four quads, the tail word; the
    64 lanes of each wave in the xor tree; the four waves in ascending order."""
    Cn, ln = x.shape
    head = min(head, ln)
    nq = (ln - head) >> 2
    tail = head + 4 * nq
    d = np.where(np.isfinite(x), x, np.float32(0)).astype(np.float64)
    seq = np.zeros((Cn, THREADS, 2 + 4 * QUADS), np.float64)
    seq[:, :head, 0] = d[:, :head]
    quads = np.zeros((Cn, QUADS * THREADS, 4), np.float64)
    quads[:, :nq] = d[:, head:tail].reshape(Cn, nq, 4)
    seq[:, :, 1:1 + 4 * QUADS] = quads.reshape(Cn, QUADS, THREADS, 4).transpose(0, 2, 1, 3).reshape(Cn, THREADS, 4 * QUADS)
    seq[:, :ln - tail, 1 + 4 * QUADS] = d[:, tail:]
    s = np.zeros((Cn, THREADS), np.float64)
    for j in range(seq.shape[2]):
        s = seq[:, :, j] * seq[:, :, j] + s                 # the product of two converted floats is exact in fp64
    w = lanes_sum(s.reshape(Cn, THREADS // 64, 64))
    r = w[:, 0]
    for k in range(1, THREADS // 64):
        r = r + w[:, k]
    return r


def partial_sums(grad, align_words=0):
    """The {sum, count} column pair the first launch leaves in its workspace.  align_words: (address of grad / 4) % 4."""
    g = np.ascontiguousarray(grad, np.float32).reshape(-1)
    n = g.size
    head = (-int(align_words)) & 3
    full = n // CHUNK
    sums = [chunk_sums(g[:full * CHUNK].reshape(full, CHUNK), head)] if full else []
    if n % CHUNK:
        sums.append(chunk_sums(g[full * CHUNK:].reshape(1, -1), head))
    bad = ~np.isfinite(g)
    chunks = (n + CHUNK - 1) // CHUNK
    counts = np.add.reduceat(bad.astype(np.int64), np.arange(chunks) * CHUNK) if chunks else np.zeros(0, np.int64)
    return np.concatenate(sums) if sums else np.zeros(0, np.float64), counts


def fold(sums):
    """The fp64 sum of the partial sums in the order of the second launch: lane l adds partials l, l + 64, ... in ascending order,
    then the xor tree."""
    rows = -(-sums.size // 64)
    padded = np.zeros(rows * 64, np.float64)
    padded[:sums.size] = sums
    s = np.zeros(64, np.float64)
    for row in padded.reshape(rows, 64):
        s = s + row
    return lanes_sum(s)
