"""The helpers of the bit-exact GPU tests (exact_util.py) on the CPU: the quantum, the exactness condition, the one rounding into the
storage type and the mismatch report."""
import pytest
import torch

import exact_util as X


def test_quantum_is_the_largest_power_of_two_dividing_every_value():
    assert X.quantum(torch.tensor([0.75, 3.0])) == 0.25
    assert X.quantum(torch.tensor([2.0, 4.0, 0.0])) == 2.0
    assert X.quantum(torch.tensor([5.0]), 1 / 16) == 1 / 16
    assert X.quantum(torch.zeros(3)) == 1.0
    assert X.quantum(torch.tensor([3.0 * 2 ** -10, 7.0])) == 2 ** -10


def test_generators_draw_the_documented_value_sets():
    gen = torch.Generator().manual_seed(1)
    sets = [(X.stored, {-1, 0, 1}), (X.grad, {-2, -1, 0, 1, 2}), (X.scale, {1, -1, 2}), (X.shift, {-1, 0, 1}), (X.qcoef, {0.5, -0.5, 0.25})]
    for fn, want in sets:
        t = fn((4000,), gen)
        assert t.dtype == torch.float64 and set(t.tolist()) == want
        assert torch.equal(t.to(torch.bfloat16).double(), t)                     # representable in bf16
    assert set(X.bias(4000, gen).tolist()) == {-3, -2, -1, 0, 1, 2, 3}
    assert set(X.weights((4000,), gen).tolist()) == {-1, 1}
    w = X.weights((40000,), gen, 0.25)
    assert set(w.tolist()) == {-1, 0, 1} and 0.2 < float((w != 0).double().mean()) < 0.3
    assert X.slope(0.0) == 0.0 and X.slope(0.01) == 0.25


def test_exactness_condition_is_a_condition_on_the_data():
    terms = torch.full((1000,), 3.0)
    assert X.assert_exact_in_fp32(terms.sum(), terms) == pytest.approx(3000 / 2 ** 24)
    with pytest.raises(AssertionError):
        X.assert_exact_in_fp32(torch.tensor(2.0 ** 24), torch.tensor([1.0]))     # 2^24 quanta: the next odd integer is not an fp32
    with pytest.raises(AssertionError):
        X.assert_exact_in_fp32(torch.tensor(2.0 ** 21), torch.tensor([1 / 16]))   # the same bound in units of 1/16
    # ... and what it promises: any order of fp32 partial sums gives the fp64 sum
    gen = torch.Generator().manual_seed(2)
    v = X.ints(-3000, 3000, (5000,), gen) / 16
    X.assert_exact_in_fp32(v.abs().sum(), v)
    for perm in (torch.arange(5000), torch.randperm(5000, generator=gen)):
        acc = torch.zeros((), dtype=torch.float32)
        for chunk in v[perm].float().split(7):
            acc = acc + chunk.sum()
        assert float(acc) == float(v.sum())


def test_to_storage_rounds_once_to_nearest_even():
    ref = torch.tensor([257.0, 259.0, 1.0 + 2 ** -8, -0.75], dtype=torch.float64)
    assert X.to_storage(ref, torch.bfloat16).tolist() == [256.0, 260.0, 1.0, -0.75]
    assert X.to_storage(ref, torch.float32).dtype == torch.float32


def test_bits_equal_reports_where_tensors_differ():
    ref = torch.zeros(2, 5, 6, 8, dtype=torch.bfloat16)
    X.assert_bits_equal(ref.clone(), ref, 'same', nhwc=True)
    got = ref.clone()
    got[1, 4, :, 3] = 1.0
    with pytest.raises(AssertionError) as e:
        X.assert_bits_equal(got, ref, 'seam', nhwc=True)
    msg = str(e.value)
    assert 'seam: 6 of 480 elements differ' in msg and 'rows y [4]' in msg and 'columns x [0, 1, 2, 3, 4, 5]' in msg and 'images [1]' in msg
    assert '(1, 4, 0, 3): got 1.0, want 0.0' in msg
    with pytest.raises(AssertionError):
        X.assert_bits_equal(ref.float(), ref, 'dtype')
    nan = torch.full((3,), float('nan'))
    with pytest.raises(AssertionError):
        X.assert_bits_equal(nan, torch.zeros(3), 'nan')
