"""numpy float32 model of rec_loss_kernel's (pixel, channel) index split, and the launch-geometry formulas of csrc/loss.hip
(seg_blocks, rec_bx, rd_adam_step's cap) restated for the tests that have to reach their edges.  No GPU, no library."""
import numpy as np

REC_LIMIT = 1 << 24                  # rd_rec_loss: (long long)H * W * C >= (1ll << 24) -> -1
FIRST_WRONG_C3 = 12582914            # first index the uncorrected split gets wrong for C = 3 (tests/test_cpu_loss_index.py)
NS_MAX, SL_U = 24, 5                 # loss.hip: sums per block of the seg-loss kernels, pixels in flight per thread (fast path)


def raw_split(i, C):
    """The uncorrected quotient, float32 arithmetic as the kernel's: (int)((float)i * (1.f / (float)C))."""
    rC = np.float32(1.0) / np.float32(C)
    return (i.astype(np.float32) * rC).astype(np.int32)        # float -> int conversion truncates; all values are >= 0


def split(i, C):
    """The kernel's split: the raw quotient, then its two correction steps in the kernel's order."""
    pix = raw_split(i, C)
    pix = pix + (i - pix * C >= C)
    pix = pix - (i - pix * C < 0)
    return pix, i - pix * C


def seg_blocks(npix):
    return max(1, min(1024, (npix + 255) // 256))


def rec_bx(per_img):
    return max(1, min(256, (per_img + 1023) // 1024))


def adam_blocks(n):
    return min(4096, (n + 255) // 256)
