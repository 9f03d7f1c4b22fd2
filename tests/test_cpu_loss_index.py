"""CPU: the numpy float32 model of rec_loss_kernel's (pixel, channel) split (csrc/loss.hip) over its whole domain.

The kernel splits an element index i < per_img into pix = i / C, c = i - pix * C without the integer-division sequence:
    pix = trunc(float32(i) * (float32(1) / float32(C)));  pix += (i - pix * C >= C);  pix -= (i - pix * C < 0)
and rd_rec_loss refuses per_img >= 2^24, where float32(i) stops being exact.  Enumerated here for every i < 2^24:
  * with the two correction steps the split equals i // C everywhere;
  * without them it is wrong for C = 3 first at i = 12,582,914 (0.75 x 2^24 + 2) and never too LOW -- so of the two steps only
    `pix -= ...` ever fires, and only in images of more than 12.58 M elements.  That is why
    tests/test_gpu_loss_edges.py::test_rec_loss_split_correction_above_12_58M_elements has to be that large, and why it runs
    padded strides too: with dense strides pix * C + c == i whatever the split, so a missing correction addresses the same element."""
import numpy as np
import pytest

from loss_index_model import FIRST_WRONG_C3, REC_LIMIT, raw_split, split


@pytest.fixture(scope='module')
def idx():
    return np.arange(REC_LIMIT, dtype=np.int32)


@pytest.mark.parametrize('C', [1, 3, 4, 7])
def test_corrected_split_is_exact_below_2_to_24(idx, C):
    assert np.float32(REC_LIMIT - 1) == REC_LIMIT - 1          # the last accepted index is still a float32
    pix, c = split(idx, C)
    assert np.array_equal(pix, idx // C)
    assert np.array_equal(c, idx % C)


def test_uncorrected_split_for_three_channels_fails_first_at_12582914_and_never_low(idx):
    raw = raw_split(idx, 3)
    diff = raw - idx // 3
    wrong = np.flatnonzero(diff)
    assert wrong.size > 0 and int(wrong[0]) == FIRST_WRONG_C3
    assert int(diff.min()) == 0 and int(diff.max()) == 1       # one too high or right: only the `pix -= ...` step ever fires
    # a 2048 x 2048 x 3 image (12,582,912 elements, the size loss.hip's comment names) ends two short of the first wrong index
    assert 2048 * 2048 * 3 < FIRST_WRONG_C3 < 2048 * 2100 * 3 < REC_LIMIT


@pytest.mark.parametrize('C', [1, 4])
def test_uncorrected_split_is_already_exact_for_power_of_two_channel_counts(idx, C):
    assert np.array_equal(raw_split(idx, C), idx // C)
