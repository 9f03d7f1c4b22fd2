"""CPU-only tests of train.py --gpu_val: the numpy model the HIP kernels are read against (ramdsir/gpu_val.py) is pinned to scipy's
post-processing bit for bit and to F.interpolate under the band rule; descriptor layout; the flag."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_val_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from gpu_val_cases import SIZES, assert_band_rule, cone_logits


def test_postprocess_model_equals_scipy_bit_for_bit():
    from ramdsir.gpu_val import postprocess_model
    from utils.metrics import postprocess_binary
    stacks = GC.stacks()
    names = ' '.join(n for n, _ in stacks)
    for must in ('empty', 'full', 'one pixel', 'two equal', 'three equal', 'corner', 'diamond ring', 'pocket', 'small ring', 'border',
                 'spiral', 'checkerboard', '1x64', '64x1', '37x53', '255x257', '800x800'):
        assert must in names, must
    for name, m in stacks:
        ref = postprocess_binary(m)
        got = postprocess_model(m)
        assert got.dtype == np.uint8 and got.shape == m.shape
        assert np.array_equal(got, ref), name


def test_postprocess_model_on_many_small_random_planes():
    """Small planes are where ties between equal areas are common."""
    from ramdsir.gpu_val import postprocess_model
    from utils.metrics import postprocess_binary
    import scipy.ndimage as ndi
    rng = np.random.RandomState(7)
    ties = 0
    for _ in range(1500):
        h, w = rng.randint(1, 13), rng.randint(1, 13)
        m = (rng.uniform(size=(2, h, w)) < rng.uniform(0.1, 0.9)).astype(np.uint8)
        lab, k = ndi.label(m[0], structure=np.ones((3, 3)))
        if k > 1:
            areas = np.bincount(lab.reshape(-1))[1:]
            ties += int((areas == areas.max()).sum() > 1)
        assert np.array_equal(postprocess_model(m), postprocess_binary(m)), m
    assert ties > 50


@pytest.mark.parametrize('size', SIZES)
def test_resize_threshold_model_against_interpolate(size):
    from ramdsir.gpu_val import resize_threshold_model
    H, W = size
    logits = cone_logits(seed=H + W)
    ref = (F.interpolate(torch.sigmoid(torch.from_numpy(logits)), size=(H, W), mode='bilinear') > 0.75).numpy().astype(np.uint8)
    got = resize_threshold_model(logits, H, W)
    assert got.shape == ref.shape and 0.01 < ref.mean() < 0.3
    assert_band_rule(got, ref, logits, H, W, 'model against CPU torch')


def test_dice_from_counts_is_the_host_formula():
    from ramdsir.gpu_val import dice_from_counts
    from utils.metrics import dice_coefficient_numpy
    rng = np.random.RandomState(1)
    for dens in (0.0, 0.3, 1.0):
        a, b = rng.uniform(size=(40, 50)) < dens, rng.uniform(size=(40, 50)) < 0.5
        assert dice_from_counts(int(a.sum()), int(b.sum()), int((a & b).sum())) == dice_coefficient_numpy(a, b)


def test_val_struct_size_matches_the_c_compiler(tmp_path):
    from ramdsir import _lib as L
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%zu %zu %zu %d\\n", sizeof(rd_val_image_t), '
           'offsetof(rd_val_image_t, h), offsetof(rd_val_image_t, slot), RD_VAL_CHUNK);return 0;}')
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, off_h, off_slot, chunk = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert ctypes.sizeof(L.RdValImage) == size == 32
    assert L.RdValImage.h.offset == off_h and L.RdValImage.slot.offset == off_slot and L.VAL_CHUNK == chunk


def test_image_records_pack_back_to_back():
    from ramdsir.gpu_val import image_records
    recs, nbytes = image_records([(3, 5), (7, 2)], gt_offs=[100, 0], slots=[4, 9])
    assert nbytes == 2 * 15 + 2 * 14
    assert [(r.off, r.gt_off, r.h, r.w, r.slot) for r in recs] == [(0, 100, 3, 5, 4), (30, 0, 7, 2, 9)]


def test_gpu_val_flag(tmp_path):
    import train
    base = ['--save_path', str(tmp_path), '--ram', '--rec']
    assert train.parse_args(base).gpu_val is False
    assert train.parse_args(base + ['--gpu_val']).gpu_val is True
    assert callable(train.test_fundus_gpu)
    a = train.parse_args(base + ['--gpu_val', '--dataset', 'prostate'])
    with pytest.raises(ValueError, match='--gpu_val covers the in-training Fundus validation only'):
        train.main(a)
