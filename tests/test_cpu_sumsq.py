"""CPU-only: the one numpy model of the fixed-order sum of squares (ramdsir/sumsq.py) behind both of its users -- step_log.model_row
over one group is guard.model over the same elements, bit for bit, and over three groups each group is summed from its own start at
its own alignment.  The kernels are held to this model on the GPU (test_gpu_step_log.py, test_gpu_grad_guard.py) and to committed
digests (test_gpu_sumsq_bits.py)."""
import numpy as np
import pytest

from ramdsir import guard as G, step_log as SL, sumsq as SQ

F32 = np.float32
LOSSES, HYPER, REC = [0.5] * 8, [2e-3, 0.1, 1e-3, 41.0], [0.75, 0.5, 0.25]


def _bits(a):
    return np.asarray(a, F32).view(np.int32)


def _random(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(n) * 10.0 ** rng.uniform(-3, 2)).astype(F32)


def test_the_guard_uses_the_shared_model():
    assert G.partial_sums is SQ.partial_sums and G.fold is SQ.fold and G.CHUNK == SQ.CHUNK == 4096
    assert (SQ.THREADS, SQ.QUADS) == (256, 4)


@pytest.mark.parametrize('n', [1, 3, 4095, 4096, 4097, 64 * 4096 + 5])
def test_one_group_is_the_guards_norm_on_bits(n):
    x = _random(n, n % 1000)
    for align in range(4):
        row = SL.model_row(LOSSES, REC, HYPER, x, [0, n, n, n], align_words=align)
        want = F32(G.model(x, align_words=align)['norm'])
        assert _bits(row[28]) == _bits(want) and row[28] > 0, (n, align, row[28:], want)
        assert not row[29:].any()


def test_three_groups_off_every_boundary_and_an_empty_group():
    """Lengths (4097, 1, 8191): the second and third group start off a 16-byte boundary and off a chunk boundary."""
    lens = (4097, 1, 8191)
    x = _random(sum(lens) + 7, 77)
    x[[5, 4097 + 1 + 100]] = [np.nan, np.inf]
    for base in (0, 3):
        r = [base, base + lens[0], base + lens[0] + lens[1], base + sum(lens)]
        for align in range(4):
            row = SL.model_row(LOSSES, REC, HYPER, x, r, align_words=align)
            bad = 0
            for k in range(3):
                m = G.model(x[r[k]:r[k + 1]], align_words=(align + r[k]) & 3)
                assert _bits(row[28 + k]) == _bits(F32(m['norm'])), (base, align, k)
                bad += m['nonfinite']
            assert row[31] == bad == 2
    # an empty group in front, in the middle and at the end: norm 0, its neighbours unmoved
    n = 4097
    for r in ([0, 0, n, n + 3], [0, n, n, n + 3], [2, n, n + 3, n + 3]):
        row = SL.model_row(LOSSES, REC, HYPER, x, r, align_words=1)
        for k in range(3):
            part = x[r[k]:r[k + 1]]
            want = F32(G.model(part, align_words=(1 + r[k]) & 3)['norm']) if part.size else F32(0)
            assert _bits(row[28 + k]) == _bits(want), (r, k)
    assert SQ.fold(np.zeros(0)) == 0.0 and [v.size for v in SQ.partial_sums(np.zeros(0, F32))] == [0, 0]
