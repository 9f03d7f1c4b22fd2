"""-m gpu: the split reduction of the weight gradients (wgrad_reduce_kernel, csrc/wgrad.hip) against a numpy float32 restatement of its
summation tree, bit for bit.  The tree is part of the contract (tests/golden/hip_bitwise.json pins the loss bits it feeds): per output,
split lane ql of QL adds splits ql, ql + QL, ... round-robin into a0..a3 in groups of 4 * QL, the remainder into a0, then
(a0 + a1) + (a2 + a3), then the lanes are folded in order q = 0..QL-1 starting from 0, then (beta ? beta * dW : 0) + v.  QL is 32 when
nsplit >= 128 and the filter has <= 16384 elements, else 8.  With 8 split lanes the launch uses 16-byte loads (four outputs per thread,
128 per block) when Cin % 4 == 0, and 4-byte loads otherwise (Cin = 3 below) and with 32 split lanes; all must give exactly these bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ramdsir import _lib as L                                                   # noqa: E402

NSPLITS = [1, 7, 8, 12, 33, 96, 257]            # both QL choices (257 >= 128), every remainder path of the 4 * QL groups
# (Cout, Cin); (16, 3): the scalar kernel; (3, 20) and (5, 4): 60 / 540 and 20 / 180 outputs, a ragged last block of the float4 form
# (lanes past the end store zeros, the fold skips them) -- heads with few output channels
SHAPES = [(16, 16), (24, 32), (16, 3), (3, 20), (5, 4)]
PAD = 32


def _tree(partial, d0, nsplit, beta):
    """partial [nsplit][taps][Cout][Cin] fp32 (padding already cut away), d0 [Cout][Cin][taps] -> dW, in float32 throughout."""
    f = np.float32
    total = partial[0].size
    QL = 32 if nsplit >= 128 and total <= 16384 else 8
    v = np.zeros(partial.shape[1:], f)
    for ql in range(QL):
        a = [np.zeros(partial.shape[1:], f) for _ in range(4)]
        k = ql
        while k + 3 * QL < nsplit:
            for j in range(4):
                a[j] = a[j] + partial[k + j * QL]
            k += 4 * QL
        while k < nsplit:
            a[0] = a[0] + partial[k]
            k += QL
        v = v + ((a[0] + a[1]) + (a[2] + a[3]))
    v = v.transpose(1, 2, 0)                                                    # [tap][n][c] -> [n][c][tap]
    return ((f(beta) * d0 if beta != 0 else np.zeros_like(d0)) + v).astype(f)


def _run(nsplit, Cout, Cin, pad_o, pad_i, taps_list, betas, seed):
    lib = L.lib()
    rng = np.random.RandomState(seed)
    for taps in taps_list:
        # wide-range values so that a regrouped sum rounds differently; the padding rows / columns hold garbage that must not be read into dW
        shape = (nsplit, taps, pad_o, pad_i)
        full = (rng.standard_normal(shape) * np.exp2(rng.randint(-6, 7, shape))).astype(np.float32)
        d0 = rng.standard_normal((Cout, Cin, taps)).astype(np.float32)
        pd = torch.from_numpy(full).cuda()
        assert pd.data_ptr() % 16 == 0
        for beta in betas:
            dW = torch.from_numpy(d0).cuda()
            L.check(lib.rd_wgrad_reduce(L.ptr(pd), L.ptr(dW), nsplit, taps, Cout, Cin, pad_o, pad_i, beta, None), 'rd_wgrad_reduce')
            torch.cuda.synchronize()
            ref = _tree(full[:, :, :Cout, :Cin], d0, nsplit, beta)
            got = dW.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
                'nsplit %d taps %d %dx%d beta %g: %d of %d outputs differ' % (nsplit, taps, Cout, Cin, beta, int((got != ref).sum()), ref.size)


@pytest.mark.parametrize('Cout,Cin', SHAPES)
@pytest.mark.parametrize('nsplit', NSPLITS)
def test_reduce_matches_the_tree_bit_for_bit(nsplit, Cout, Cin):
    _run(nsplit, Cout, Cin, PAD, PAD, (1, 9), (0.0, 1.0), 1000 * nsplit + 10 * Cout + Cin)


@pytest.mark.parametrize('Cin', [340, 85], ids=['float4', 'scalar'])
def test_more_blocks_than_the_grid_cap(Cin):
    """The grid is capped at 8192 blocks and a block then walks several groups of outputs: 351 x 340 x 9 = 1 074 060 outputs in blocks of
    128 (float4 form; the last block ragged) and 351 x 85 x 9 = 268 515 in blocks of 32 (scalar form), two splits."""
    _run(2, 351, Cin, 352, 352, (9,), (1.0,), Cin)
