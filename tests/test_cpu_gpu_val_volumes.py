"""CPU-only tests of train.py --gpu_val_volumes: the numpy model the HIP kernels are read against (ramdsir/gpu_val_volumes.py) is
pinned to scipy's largest component bit for bit and to utils.prostate_eval.predict_volume's batches and predictions; the Dice formula;
descriptor layout; the flag."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import gpu_val_volumes_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(m):
    """connectivity_region_analysis as predict_volume calls it: on a float64 volume."""
    from utils.metrics import connectivity_region_analysis
    return connectivity_region_analysis(np.asarray(m, dtype=np.float64))


def test_largest_component_model_equals_scipy_bit_for_bit():
    from ramdsir.gpu_val_volumes import largest_component_model
    cases = VC.named_volumes()
    names = ' '.join(n for n, _ in cases)
    for must in ('empty', 'full', 'one voxel', 'two equal in different slices', 'in-plane corner', 'edge across slices', 'cube corner',
                 'through all slices', 'D = 1'):
        assert must in names, must
    assert any(VC.has_tie(m) for _, m in cases)
    for name, m in cases:
        ref = _reference(m)
        got = largest_component_model(m)
        assert got.dtype == np.uint8 and got.shape == m.shape
        assert np.array_equal(got, ref), name
    assert largest_component_model(VC.named_volumes()[0][1]).all()               # the empty prediction becomes all ones


def test_largest_component_model_on_many_small_random_volumes():
    """Small volumes are where ties between equal sizes are common."""
    from ramdsir.gpu_val_volumes import largest_component_model
    rng = np.random.RandomState(11)
    ties = n = 0
    for dens in (0.2, 0.4, 0.6):
        for _ in range(600):
            d, h, w = rng.randint(1, 9, 3)
            m = (rng.uniform(size=(d, h, w)) < dens).astype(np.uint8)
            ties += int(VC.has_tie(m))
            n += 1
            assert np.array_equal(largest_component_model(m), _reference(m)), m
    assert n >= 1500 and ties >= 100, (n, ties)


class _Recorder:
    """A stub `forward`: records the batches predict_volume feeds and returns fixed logits for them."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.batches, self.logits = [], []

    def __call__(self, v):
        assert v.dtype == torch.float32
        self.batches.append(v.numpy().copy())
        lg = self.rng.normal(0, 1, (v.shape[0], 2) + tuple(v.shape[2:])).astype(np.float32)
        tie = self.rng.uniform(size=lg[:, 1].shape) < 0.1                         # some exact ties between the two classes
        lg[:, 1][tie] = lg[:, 0][tie]
        lg[0, 1, 0, :] = lg[0, 0, 0, :]
        self.logits.append(lg)
        return torch.from_numpy(lg)


@pytest.mark.parametrize('D,bs,dtype', [(10, 4, np.float32), (13, 4, np.int16), (5, 4, np.float64), (3, 4, np.float32), (8, 2, np.uint8),
                                        (2, 1, np.float32)])
def test_stack_and_argmax_models_reproduce_predict_volume(D, bs, dtype):
    """The batches (`vol`), the prediction before post-processing (`pred_y`) and the result, with D % batch_size != 0, D < batch_size
    (no batch at all -> all ones) and empty ground-truth slices."""
    from ramdsir import gpu_val_volumes as V
    from utils import prostate_eval as PE
    rng = np.random.RandomState(D * 7 + bs)
    image = rng.uniform(0, 900, (D, 12, 10)).astype(dtype)
    mask = (rng.uniform(size=(D, 12, 10)) < 0.3).astype(np.uint8) * rng.randint(1, 3, (D, 12, 10)).astype(np.uint8)
    mask[1::3] = 0                                                                # empty ground-truth slices
    rec = _Recorder(D)
    post_ref, mask_ref = PE.predict_volume(rec, image, mask, bs)
    # the model, fed as the resident path feeds it
    vol = torch.from_numpy(np.asarray(PE.normalise_volume(image), dtype=np.float64)).float().numpy()
    merged = PE.merge_labels(mask)
    assert np.array_equal(merged, mask_ref)
    gt_empty = np.array([np.sum(merged[jj]) == 0 for jj in range(D)], dtype=np.uint8)
    assert gt_empty[1] == 1 or D < 2
    batches = V.frame_batches(D, bs)
    assert len(batches) == len(rec.batches) == D // bs
    pred = np.zeros((D, 12, 10), np.uint8)
    for frames, fed, lg in zip(batches, rec.batches, rec.logits):
        assert len(frames) == bs
        got = V.stack_model(vol, frames)
        assert got.dtype == np.float32 and np.array_equal(got, fed)
        V.argmax_model(lg, frames, gt_empty, pred)
    # pred_y itself: recomputed the host way from the recorded logits
    pred_y = np.zeros(mask.shape)
    frame_list = list(range(1, D - 1))
    for ii, lg in enumerate(rec.logits):
        p = torch.max(torch.softmax(torch.from_numpy(lg), dim=1), dim=1)[1].numpy()
        sm = torch.softmax(torch.from_numpy(lg), dim=1).numpy()
        assert np.array_equal(p[sm[:, 0] != sm[:, 1]], (lg[:, 1] > lg[:, 0])[sm[:, 0] != sm[:, 1]].astype(p.dtype))
        for idx, jj in enumerate(frame_list[ii * bs:(ii + 1) * bs]):
            if np.sum(merged[jj]) != 0:
                pred_y[jj] = p[idx]
    assert np.array_equal(pred, pred_y.astype(np.uint8))
    assert np.array_equal(V.largest_component_model(pred), post_ref)
    if D < bs:
        assert post_ref.all()                                                     # no batch ran: the empty prediction becomes all ones
    post = V.largest_component_model(pred).astype(bool)
    gt = merged != 0
    assert V.dice_from_counts(int(post.sum()), int(gt.sum()), int((post & gt).sum())) == PE.dc(post_ref.astype(bool), mask_ref.astype(bool))


def test_normalise_volume_is_predict_volumes_expression():
    from utils.prostate_eval import normalise_volume
    rng = np.random.RandomState(2)
    for dtype in (np.float32, np.float64, np.int16, np.uint8):
        image = rng.uniform(0, 200, (4, 5, 6)).astype(dtype)
        mx, mn = np.max(image), np.min(image)
        want = 2 * (image - mn) / (mx - mn) - 1
        got = normalise_volume(image)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    with np.errstate(all='ignore'):
        flat = normalise_volume(np.full((2, 3, 3), 7, np.int16))                  # mx == mn: whatever the expression gives
    assert np.isnan(flat).all()


def test_dice_from_counts_is_the_host_formula():
    from ramdsir.gpu_val_volumes import dice_from_counts
    from utils.metrics import dc
    rng = np.random.RandomState(1)
    for da in (0.0, 0.3, 1.0):
        for db in (0.0, 0.5):
            a, b = rng.uniform(size=(4, 40, 50)) < da, rng.uniform(size=(4, 40, 50)) < db
            got = dice_from_counts(int(a.sum()), int(b.sum()), int((a & b).sum()))
            assert isinstance(got, float) and got == dc(a, b), (da, db)
    assert dice_from_counts(0, 0, 0) == 0.0


def test_post_groups_and_records():
    from ramdsir.gpu_val_volumes import post_groups, volume_records
    shapes = [(2, 2, 2)] * 5 + [(9, 3, 3)]
    assert post_groups(shapes, limit=16) == [(0, 2), (2, 4), (4, 5), (5, 6)]
    assert post_groups([], limit=16) == [] and post_groups([(9, 3, 3)], limit=16) == [(0, 1)]
    recs, nbytes = volume_records([(3, 5, 2), (7, 2, 4)], gt_offs=[100, 0], slots=[4, 9])
    assert nbytes == 30 + 56
    assert [(r.off, r.gt_off, r.d, r.h, r.w, r.slot) for r in recs] == [(0, 100, 3, 5, 2, 4), (30, 0, 7, 2, 4, 9)]


def test_volume_struct_size_matches_the_c_compiler(tmp_path):
    from ramdsir import _lib as L
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
           'sizeof(rd_val_volume_t), offsetof(rd_val_volume_t, gt_off), offsetof(rd_val_volume_t, d), offsetof(rd_val_volume_t, w), '
           'offsetof(rd_val_volume_t, slot));return 0;}')
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, off_gt, off_d, off_w, off_slot = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert ctypes.sizeof(L.RdValVolume) == size == 32
    assert (L.RdValVolume.gt_off.offset, L.RdValVolume.d.offset, L.RdValVolume.w.offset, L.RdValVolume.slot.offset) == (off_gt, off_d, off_w,
                                                                                                                         off_slot)


def test_gpu_val_volumes_flag(tmp_path):
    import train
    base = ['--save_path', str(tmp_path), '--ram', '--rec']
    assert train.parse_args(base).gpu_val_volumes is False
    assert train.parse_args(base + ['--gpu_val_volumes']).gpu_val_volumes is True
    assert callable(train.test_prostate_gpu)
    a = train.parse_args(base + ['--gpu_val_volumes', '--dataset', 'fundus'])
    with pytest.raises(ValueError, match='--gpu_val_volumes covers the in-training Prostate validation only'):
        train.main(a)
