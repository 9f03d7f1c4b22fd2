"""The fixed plane set of the --gpu_val post-processing tests (TEST INFRASTRUCTURE): every rule of largest-component + hole filling
has a plane here that only passes if the rule is implemented as scipy implements it; and the logits, sizes and band rule of the
resize + threshold tests.  Shared by the CPU suite (the numpy model
against scipy) and the GPU suite (the kernels against scipy)."""
import numpy as np

BAND = 1e-4                 # pixels whose exact probability is this close to 0.75 may differ between two float32 implementations
BAND_SHARE = 1e-3           # ... and they may be at most this share of a test case's pixels
SIZES = [(800, 800), (611, 797), (1634, 1634)]


def cone_logits(seed, n=2, S=256):
    """A few cones of height 12 plus N(0, 1.5) noise, minus 3: structured masks with a few per cent of foreground."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.empty((n, 2, S, S), np.float32)
    for b in range(n):
        for c in range(2):
            z = np.zeros((S, S), np.float32)
            for _ in range(3):
                cy, cx, r = rng.uniform(0.2 * S, 0.8 * S), rng.uniform(0.2 * S, 0.8 * S), rng.uniform(0.08 * S, 0.2 * S)
                z = np.maximum(z, 12.0 * np.clip(1.0 - np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / r, 0, None))
            out[b, c] = z + rng.normal(0, 1.5, (S, S)) - 3.0
    return out


def assert_band_rule(got, ref, logits, H, W, what):
    """got == ref outside the band; the band holds at most BAND_SHARE of the pixels."""
    from ramdsir.gpu_val import resize_probability_f64
    band = np.abs(resize_probability_f64(logits, H, W) - 0.75) < BAND
    diff = np.asarray(got) != np.asarray(ref)
    print('%s %dx%d: band %.2e of the pixels, %d differ, %d of them outside the band, foreground %.3f'
          % (what, H, W, band.mean(), diff.sum(), (diff & ~band).sum(), np.asarray(ref).mean()))
    assert band.mean() <= BAND_SHARE, (what, band.mean())
    assert not (diff & ~band).any(), (what, int((diff & ~band).sum()))


def _z(h, w):
    return np.zeros((h, w), np.uint8)


def _spiral(n):
    """A one-pixel arm winding inwards with a one-pixel gap: one component, no hole (the gap is a corridor to the border)."""
    m = _z(n, n)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead_free = 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= fy < n and 0 <= fx < n and m[fy, fx])
        if ahead_free:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def named_planes():
    """[(name, (H, W) uint8 0/1)]"""
    out = []
    out.append(('empty', _z(7, 9)))
    out.append(('full', np.ones((6, 11), np.uint8)))
    m = _z(5, 8); m[3, 6] = 1
    out.append(('one pixel', m))
    # equal areas: the component whose first pixel comes first in raster order wins
    m = _z(9, 9); m[0:2, 6:8] = 1; m[6:8, 1:3] = 1
    out.append(('two equal, right one first', m))
    out.append(('two equal, left one first', m[:, ::-1].copy()))
    out.append(('two equal, transposed', m.T.copy()))
    m = _z(9, 12); m[1, 8:11] = 1; m[0:3, 1] = 1; m[6, 4:7] = 1
    out.append(('two equal, same first row: the lower start column wins', m))
    m = _z(12, 12); m[1:3, 8:10] = 1; m[5:7, 0:2] = 1; m[9:11, 5:7] = 1
    out.append(('three equal', m))
    out.append(('three equal, flipped', m[::-1].copy()))
    out.append(('three equal, transposed and flipped', m.T[:, ::-1].copy()))
    m = _z(10, 10); m[2, 7] = 1; m[0:2, 0:2] = 1; m[5:9, 5] = 1; m[8, 0:4] = 1        # 1, 4, 4, 4
    out.append(('a smaller first, then three equal', m))
    # 8- against 4-connectivity
    m = _z(8, 8); m[0:3, 0:3] = 1; m[3:5, 3:5] = 1; m[6:8, 0:3] = 1                     # 9 + 4 joined at a corner beat... 6
    out.append(('blocks joined at a corner', m))
    m = _z(8, 10); m[0:2, 0:2] = 1; m[2:4, 2:4] = 1; m[5:8, 5:8] = 1                   # 4 + 4 = 8 < 9 only if the corner joins them
    out.append(('two small blocks joined at a corner against one larger', m))
    m = _z(9, 9)
    for k in range(9):
        m[k, k] = 1
    out.append(('a diagonal line', m))
    out.append(('an anti-diagonal line', m[:, ::-1].copy()))
    # a ring closed only by diagonal steps: its inside is a hole
    m = _z(9, 9)
    for k in range(5):
        m[4 - k, k] = m[4 + k, k] = m[k, 4 + k] = m[8 - k, 4 + k] = 1
    out.append(('diamond ring', m))
    m = _z(7, 7); m[1:6, 1:6] = 1; m[2:5, 2:5] = 0; m[1, 1] = 0
    out.append(('pocket that meets the outside only at a corner', m))
    m = _z(7, 7); m[1:6, 1:6] = 1; m[2:5, 2:5] = 0; m[1, 3] = 0
    out.append(('pocket open to the outside through an edge', m))
    # holes of discarded components vanish with them
    m = _z(16, 20); m[1:9, 1:9] = 1; m[3:6, 3:6] = 0; m[10:15, 12:17] = 1; m[11:14, 13:16] = 0
    out.append(('a large ring and a small ring', m))
    m = _z(16, 20); m[1:9, 1:9] = 1; m[3, 3] = 0; m[10:15, 12:17] = 1; m[11:14, 13:16] = 0; m[12, 14] = 1
    out.append(('a large block with a hole; a small ring around an island', m))
    # the border
    m = _z(10, 10); m[0:6, 0:6] = 1; m[0:4, 2:4] = 0
    out.append(('a notch open to the border', m))
    m = _z(10, 10); m[0:6, 0:6] = 1; m[1:4, 2:4] = 0
    out.append(('a component on the border with a hole inside', m))
    m = np.ones((9, 9), np.uint8); m[0, 4] = 0; m[4, 4] = 0; m[8, 8] = 0; m[3:6, 0] = 0
    out.append(('full with border background and one hole', m))
    m = _z(9, 9); m[:, 4] = 1; m[4, :] = 1
    out.append(('a cross to all four borders', m))
    m = np.ones((9, 9), np.uint8); m[:, 4] = 0; m[4, :] = 0
    out.append(('four equal quadrants', m))
    out.append(('spiral 41', _spiral(41)))
    out.append(('spiral 20', _spiral(20)))
    out.append(('spiral 41, inverted', (1 - _spiral(41)).astype(np.uint8)))
    yy, xx = np.mgrid[0:16, 0:17]
    out.append(('checkerboard', ((yy + xx) % 2).astype(np.uint8)))
    out.append(('checkerboard, other phase', ((yy + xx + 1) % 2).astype(np.uint8)))
    out.append(('stripes', (yy % 2).astype(np.uint8)))
    rng = np.random.RandomState(20240)
    for shape in ((1, 64), (64, 1), (1, 1), (37, 53), (255, 257)):
        for dens in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9):
            out.append(('random %dx%d %.1f' % (shape[0], shape[1], dens), (rng.uniform(size=shape) < dens).astype(np.uint8)))
    for dens in (0.1, 0.5, 0.9):
        out.append(('random 800x800 %.1f' % dens, (rng.uniform(size=(800, 800)) < dens).astype(np.uint8)))
    # what validation sees: a disc with noise around its rim, some islands, some pinholes
    yy, xx = np.mgrid[0:800, 0:800]
    r = np.sqrt((yy - 390.0) ** 2 + (xx - 410.0) ** 2)
    m = ((r + rng.normal(0, 6, r.shape)) < 250).astype(np.uint8)
    m[rng.uniform(size=m.shape) < 0.002] ^= 1
    out.append(('noisy disc 800x800', m))
    return out


def stacks():
    """[(name, (2, H, W) uint8)]: every plane with its mirror image as the second structure (another raster order)."""
    return [(n, np.stack([p, p[:, ::-1]]).astype(np.uint8)) for n, p in named_planes()]
