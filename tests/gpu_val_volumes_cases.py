"""The fixed volume set of the --gpu_val_volumes tests (TEST INFRASTRUCTURE): every rule of the largest-3-D-component step has a
volume here that only passes if the rule is implemented as scipy.ndimage.label (face connectivity) + argmax implement it.  Shared by
the CPU suite (the numpy model against scipy) and the GPU suite (rd_vol_post against scipy)."""
import numpy as np


def _z(d, h, w):
    return np.zeros((d, h, w), np.uint8)


def named_volumes():
    """[(name, (D, H, W) uint8 0/1)]"""
    out = []
    out.append(('empty', _z(3, 5, 7)))
    out.append(('empty, one slice', _z(1, 4, 4)))
    out.append(('full', np.ones((4, 6, 5), np.uint8)))
    m = _z(4, 5, 6); m[2, 3, 4] = 1
    out.append(('one voxel', m))
    m = _z(1, 1, 1); m[0, 0, 0] = 1
    out.append(('one voxel, 1x1x1', m))
    # equal sizes: the component whose first voxel comes first in (z, y, x) raster order wins
    m = _z(5, 6, 6); m[3, 0:2, 0:2] = 1; m[1, 4:6, 4:6] = 1
    out.append(('two equal in different slices: the lower slice wins', m))
    out.append(('two equal in different slices, flipped in z', m[::-1].copy()))
    m = _z(3, 8, 8); m[1, 1, 5:8] = 1; m[1, 0:3, 1] = 1; m[1, 6, 2:5] = 1
    out.append(('three equal in one slice', m))
    m = _z(4, 6, 6); m[0, 5, 5] = 1; m[1, 0:2, 0] = 1; m[2, 3, 3:5] = 1; m[3, 0, 0:2] = 1
    out.append(('a smaller first, then three equal', m))
    # face connectivity: contact through an edge or a corner does not connect
    m = _z(2, 6, 6); m[0, 0:3, 0:3] = 1; m[0, 3:5, 3:5] = 1; m[1, 5, 0:5] = 1          # 9 | 4 | 5: the corner must not make 13
    out.append(('blocks that touch at an in-plane corner', m))
    m = _z(3, 4, 6); m[0, 1, 0:3] = 1; m[1, 2, 0:3] = 1; m[2, 0, 0:4] = 1               # 3 | 3 | 4: the z-y edge must not make 6
    out.append(('runs that touch at an edge across slices', m))
    m = _z(3, 4, 6); m[0, 1, 0:3] = 1; m[1, 1, 3:6] = 1; m[2, 3, 0:4] = 1               # 3 | 3 | 4: the z-x edge must not make 6
    out.append(('runs that touch at an edge across slices along x', m))
    m = _z(3, 4, 4); m[0, 0:2, 0:2] = 1; m[1, 2:4, 2:4] = 1; m[2, 0, 0:4] = 1; m[2, 1, 0] = 1   # 4 | 4 | 5: the cube corner must not make 8
    out.append(('blocks that touch at a cube corner', m))
    m = _z(4, 5, 5)
    for k in range(4):
        m[k, k, k] = 1
    out.append(('a space diagonal: four components of one voxel', m))
    # connections that exist only through the third axis
    m = _z(5, 7, 7); m[:, 3, 3] = 1; m[2, 0, 0:4] = 1
    out.append(('a column through all slices beats a run of four', m))
    m = _z(3, 5, 9); m[0, 2, 0:4] = 1; m[2, 2, 5:9] = 1; m[1, 2, 3:6] = 1; m[0, 2, 4] = 0; m[1, 2, 4] = 1
    out.append(('two runs joined by a bridge in the slice between', m))
    m = _z(6, 9, 9); m[:, 1:8, 1:8] = 1; m[1:5, 2:7, 2:7] = 0; m[3, 4, 4] = 1
    out.append(('a hollow box around an island', m))
    m = _z(4, 8, 8); m[0] = 1; m[3] = 1; m[1:3, 0, 0] = 1; m[3, 7, 7] = 0
    out.append(('two slabs joined by one column', m))
    zz, yy, xx = np.mgrid[0:5, 0:6, 0:7]
    out.append(('3-D checkerboard', ((zz + yy + xx) % 2).astype(np.uint8)))
    out.append(('alternating slices', np.broadcast_to((zz % 2).astype(np.uint8), zz.shape).copy()))
    m = _z(1, 9, 9); m[0, 0:2, 6:8] = 1; m[0, 6:8, 1:3] = 1
    out.append(('D = 1: two equal', m))
    m = _z(1, 6, 300); m[0, 2, 10:290] = 1; m[0, 4, 0:100] = 1
    out.append(('D = 1: rows longer than a workgroup', m))
    rng = np.random.RandomState(20250)
    for shape in ((1, 1, 64), (64, 1, 1), (1, 64, 1), (7, 13, 11), (5, 37, 53), (3, 20, 300)):
        for dens in (0.2, 0.4, 0.6, 0.8):
            out.append(('random %dx%dx%d %.1f' % (shape + (dens,)), (rng.uniform(size=shape) < dens).astype(np.uint8)))
    return out


def big_volumes():
    """384 x 384 slices, as the real volumes have: random noise, a noisy ball with islands, and an empty one."""
    rng = np.random.RandomState(20251)
    out = [('random 6x384x384 0.5', (rng.uniform(size=(6, 384, 384)) < 0.5).astype(np.uint8)),
           ('random 5x384x384 0.7', (rng.uniform(size=(5, 384, 384)) < 0.7).astype(np.uint8))]
    zz, yy, xx = np.mgrid[0:12, 0:384, 0:384]
    r = np.sqrt((6.0 * (zz - 5.5)) ** 2 + (yy - 190.0) ** 2 + (xx - 200.0) ** 2)
    m = ((r + rng.normal(0, 6, r.shape)) < 90).astype(np.uint8)
    m[rng.uniform(size=m.shape) < 0.002] ^= 1
    out.append(('noisy ball 12x384x384', m))
    out.append(('empty 4x384x384', np.zeros((4, 384, 384), np.uint8)))
    return out


def has_tie(m):
    """True when the largest component of m is not unique."""
    import scipy.ndimage as ndi
    lab, k = ndi.label(m)
    if k < 2:
        return False
    areas = np.bincount(lab.reshape(-1))[1:]
    return int((areas == areas.max()).sum()) > 1
