"""Helpers for the bit-exact parity tests (test_gpu_exact.py): small-integer / dyadic test data on which every product and every
accumulation of a kernel is exact in fp32, so that the result does not depend on summation order, atomics, MFMA k-order or how tiles
are dealt to workgroups -- and the fp64 torch reference has to be matched BIT FOR BIT, in bf16 as in fp32.

All generators draw from a seeded torch.Generator and return fp64 host tensors; every value is representable in bf16."""
import torch

CAP = 2 ** 24          # integers up to 2^24 are exact in fp32: a sum whose |terms| add up to less than 2^24 quanta never rounds


def _choice(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=gen)]


def ints(lo, hi, shape, gen):
    """Integers in [lo, hi] as fp64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()


def stored(shape, gen):
    """A stored activation tensor (z, t, x): integers in {-1, 0, 1} -- a third of them exact zeros, ties in every pool window."""
    return ints(-1, 1, shape, gen)


def grad(shape, gen):
    """A stored gradient tensor (g, dz, gp): integers in [-2, 2]."""
    return ints(-2, 2, shape, gen)


def scale(shape, gen):
    """BatchNorm scale / the P of a BatchNorm backward: {1, -1, 2}."""
    return _choice([1.0, -1.0, 2.0], shape, gen)


def shift(shape, gen):
    """BatchNorm shift / the R of a BatchNorm backward: {-1, 0, 1}."""
    return ints(-1, 1, shape, gen)


def qcoef(shape, gen):
    """The Q of a BatchNorm backward: {0.5, -0.5, 0.25}."""
    return _choice([0.5, -0.5, 0.25], shape, gen)


def bias(n, gen):
    return ints(-3, 3, (n,), gen)


def weights(shape, gen, density=1.0):
    """+-1 weights; with density < 1 only that share of them is non-zero (keeps the sums of squares of wide layers under the cap)."""
    w = _choice([1.0, -1.0], shape, gen)
    if density < 1.0:
        w = w * (torch.rand(tuple(shape), generator=gen, dtype=torch.float64) < density).double()
    return w


def slope(case_slope):
    """The case tables say 0 (ReLU) or 0.01 (LeakyReLU).  0.01 is not dyadic and the kernels take the slope as a plain float: 0.25."""
    return 0.0 if case_slope == 0 else 0.25


def quantum(*values):
    """The largest power of two that divides every (non-zero) value of the given tensors / numbers."""
    q = None
    for v in values:
        v = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
        v = v[v != 0].abs()
        if v.numel() == 0:
            continue
        m, e = torch.frexp(v)                                  # v = m * 2^e, 0.5 <= m < 1, m has at most 53 bits
        mi = (m * 2.0 ** 53).to(torch.int64)
        tz = torch.log2((mi & -mi).double()).to(torch.int64)   # trailing zero bits of the 53-bit mantissa
        lo = int((e.to(torch.int64) - 53 + tz).min())
        q = lo if q is None else min(q, lo)
    return 2.0 ** (q if q is not None else 0)


def exact_ratio(terms_abs_sum, values):
    """(largest sum of |terms|) / quantum / 2^24: below 1 means every fp32 partial sum of those terms, in any order, is exact."""
    q = quantum(*values) if isinstance(values, (list, tuple)) else quantum(values)
    return float(torch.as_tensor(terms_abs_sum, dtype=torch.float64).max()) / q / CAP


def assert_exact_in_fp32(terms_abs_sum, values, what=''):
    """A CONDITION on the test data (applied to the reference only), not a tolerance: the sum of the absolute terms of an accumulated
    quantity, in units of the quantum of `values` (the terms themselves, or tensors with their quantum), stays below 2^24.  Taken over
    the whole sum it holds for any split into fp32 partials.  A case that violates it fails; it does not skip."""
    r = exact_ratio(terms_abs_sum, values)
    assert r < 1.0, '%s: sum of |terms| is %.3g x the 2^24-quanta cap: this data is not exact in fp32' % (what, r)
    return r


def to_storage(ref64, dtype):
    """ONE round-to-nearest-even from the exact value to the storage dtype (the fp32 step in between is exact by the condition above)."""
    return ref64.float().to(dtype)


def group_sums(t_nchw, gstart):
    """[G][C] fp64 sums of an NCHW tensor over the images and pixels of each group."""
    return torch.stack([t_nchw[gstart[g]:gstart[g + 1]].sum((0, 2, 3)) for g in range(len(gstart) - 1)])


def pair_sums(a_nchw, b_nchw, gstart):
    """[G][C][2]: the two per-(group, channel) sums a statistics buffer holds."""
    return torch.stack([group_sums(a_nchw, gstart), group_sums(b_nchw, gstart)], -1)


def assert_bits_equal(got, ref, what, nhwc=False):
    """torch.equal (value for value; -0.0 equals +0.0), and a report that tells a seam bug from a rounding bug: how many elements differ, the first few with both values,
    and for NHWC tensors the rows (y) and columns (x) affected."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, '%s: %s %s vs %s %s' % (what, tuple(got.shape), got.dtype, tuple(ref.shape), ref.dtype)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | (torch.isnan(got) != torch.isnan(ref))
    bad &= ~(torch.isnan(got) & torch.isnan(ref))
    idx = bad.nonzero()
    msg = ['%s: %d of %d elements differ' % (what, idx.shape[0], got.numel())]
    for i in idx[:8].tolist():
        msg.append('  %s: got %r, want %r' % (tuple(i), float(got[tuple(i)]), float(ref[tuple(i)])))
    if nhwc and got.dim() == 4:
        msg.append('  images %s' % sorted(set(idx[:, 0].tolist())))
        msg.append('  rows y %s' % sorted(set(idx[:, 1].tolist())))
        msg.append('  columns x %s' % sorted(set(idx[:, 2].tolist())))
        ch = sorted(set(idx[:, 3].tolist()))
        msg.append('  channels %s' % (ch if len(ch) <= 40 else '%d of %d' % (len(ch), got.shape[3])))
    raise AssertionError('\n'.join(msg))
