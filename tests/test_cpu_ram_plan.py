"""CPU: the plan and index arithmetic of the RAM FFT kernels (csrc/ram_fft.hip) over their whole domain, and every refusal code of
the RAM entry points before a launch.

  * make_plan restated (tests/ram_plan_model.py): radix order 4, 2, 3, 5; the legal sides are exactly the 5-smooth numbers <= 1024.
  * fft_runtime splits a work item jj < batch * nb into (transform t, butterfly j) and j into (q, k) with float-reciprocal quotients
    `(int)(((float)a + 0.5f) * (1.0f / d))`, claimed exact "for a < 2^12, divisor <= 1024".  Enumerated here in float32 for every
    legal side, every stage and the batches the launchers use (1, 2, 3), against integer division; every twiddle index r * k * tstep
    stays inside the table.
  * the compile-time radix lists multiply to their N, are what the source text says, and their twiddle reads stay inside the table
    of the side (of twice the length for the real-input row pass).
  * rd_ram_mix / rd_ram_mutate / rd_ram_amp / rd_ram_dft_tables refuse bad arguments with their documented codes before anything is
    launched (host structs with dummy non-null pointers; no GPU), and the workspace / table sizes equal their documented formulas."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import ram_plan_model as M                      # noqa: E402
from ramdsir import _lib as L                   # noqa: E402


# ------------------------------------------------------------------------------------------------------------- make_plan
def test_legal_sides_are_the_5_smooth_numbers_up_to_1024():
    smooth = sorted({2 ** a * 3 ** b * 5 ** c for a in range(11) for b in range(7) for c in range(5) if 2 ** a * 3 ** b * 5 ** c <= 1024})
    legal = M.legal_sides()
    assert legal == smooth and len(legal) == 87
    for N in (15, 27, 45, 75, 81, 125, 243, 16, 24, 32, 250, 320, 640, 800, 1000, 1024):
        assert N in legal
    for N in (7, 14, 33, 77, 1022, 1023):
        assert not M.make_plan(N)[0]
    for N in (1030, 1080, 1125, 1250, 1280, 2048, 4096, 4 ** 13):   # beyond the documented maximum, whatever their factors
        assert not M.make_plan(N)[0]
    assert not M.make_plan(0)[0] and not M.make_plan(-16)[0]         # refused before the factor loops (0 % 4 == 0 for ever)
    assert max(len(M.make_plan(N)[1]) for N in legal) <= 6 < M.MAX_STAGES      # the stage limit never binds below 1025


def test_radix_order_is_4s_2s_3s_5s():
    assert M.make_plan(1024)[1] == [4] * 5
    assert M.make_plan(512)[1] == [4, 4, 4, 4, 2]
    assert M.make_plan(1000)[1] == [4, 2, 5, 5, 5]
    assert M.make_plan(960)[1] == [4, 4, 4, 3, 5]
    assert M.make_plan(750)[1] == [2, 3, 5, 5, 5]
    assert M.make_plan(243)[1] == [3] * 5 and M.make_plan(125)[1] == [5] * 3 and M.make_plan(1)[1] == []
    for N in M.legal_sides():
        r = M.make_plan(N)[1]
        assert int(np.prod(r, dtype=np.int64)) == N and r.count(2) <= 1
        assert r == sorted(r, key=(4, 2, 3, 5).index)


# ------------------------------------------------------------------------------------------------------------- fft_runtime
def test_runtime_plan_float_quotients_equal_integer_division_everywhere():
    checked = 0
    worst_a, worst_d = 0, 0
    for N in M.legal_sides():
        for R, nb, Ns, tstep in M.stages(N, M.make_plan(N)[1]):
            assert nb * R == N and tstep * Ns * R == N
            for batch in M.BATCHES:
                jj = np.arange(batch * nb, dtype=np.int32)
                t, j, q, k = M.runtime_split(jj, nb, Ns)
                assert np.array_equal(t, jj // nb) and np.array_equal(j, jj % nb), (N, R, batch)
                assert np.array_equal(q, j // Ns) and np.array_equal(k, j % Ns), (N, R, batch)
                # the reads a[j + r * nb] and the writes o[q * Ns * R + k + r * Ns] stay inside the transform's N points
                assert int((j + (R - 1) * nb).max()) < N and int((q * Ns * R + k + (R - 1) * Ns).max()) < N
                # tw[r * k * tstep], r < R: inside the table of N entries
                assert int(((R - 1) * k * tstep).max()) < N, (N, R)
                checked += jj.size
                worst_a, worst_d = max(worst_a, batch * nb - 1), max(worst_d, nb, Ns)
    assert worst_a < 2 ** 12 and worst_d <= 1024                     # the range the kernel's comment claims
    assert checked > 100000


def test_float_quotient_is_not_exact_without_the_half():
    """Why the kernel adds 0.5: for some divisors the plain product (float)a * (1.0f / d) falls short of an exact multiple a = m * d
    and truncates to m - 1, so the model would notice a kernel that dropped the half."""
    f = np.float32
    bad = 0
    for d in range(1, 1025):
        a = np.arange(0, 3 * d, dtype=np.int32)
        bad += int(np.count_nonzero((a.astype(f) * (f(1.0) / f(d))).astype(np.int32) != a // d))
    assert bad > 0


# ------------------------------------------------------------------------------------------------------------- compile-time plans
def test_compile_time_radix_lists_multiply_to_n_and_match_the_source():
    assert sorted(M.FIXED) == [128, 192, 200, 256, 384, 400, 512]
    for N, radix in M.FIXED.items():
        assert int(np.prod(radix)) == N and set(radix) <= {2, 3, 4, 5}
    src = open(os.path.join(ROOT, 'ram-dsir_amd', 'csrc', 'ram_fft.hip')).read()
    found = {int(n): tuple(int(v) for v in lst.split(',')) for n, lst in
             re.findall(r'N == (\d+)\) return fft_chain<N, INV, TWS, 1, 0, ([\d, ]+)>', src)}
    m = re.search(r'static_assert\(N == (\d+),[^;]*;\s*return fft_chain<N, INV, TWS, 1, 0, ([\d, ]+)>', src)
    found[int(m.group(1))] = tuple(int(v) for v in m.group(2).split(','))
    assert found == M.FIXED
    sides = tuple(int(v) for v in re.findall(r'case (\d+): CALL\(\1\); break;', src))
    assert sides == M.FIXED_SIDES and all(s in M.FIXED and s // 2 in M.FIXED for s in sides)


@pytest.mark.parametrize('N,tws', [(n, 1) for n in M.FIXED_SIDES] + [(n // 2, 2) for n in M.FIXED_SIDES])
def test_compile_time_twiddle_reads_stay_inside_the_table(N, tws):
    """stage_fixed reads tw[TWS * r * k * tstep], r < R, k < NS, from the table of TWS * N entries; the real-input post-pass reads
    s_tw[kx], kx <= b < N, and Z[N - kx]."""
    for R, nb, Ns, tstep in M.stages(N, M.FIXED[N]):
        assert tws * (R - 1) * (Ns - 1) * tstep < tws * N
    if tws == 2:
        b_max = (2 * N - 1) // 2                                     # 2 b + 1 <= W = 2 N
        assert b_max < N and N - b_max >= 1                          # side 256: b = 127 is the last bin, Z[M - 127] = Z[1]


# ------------------------------------------------------------------------------------------------------------- refusals
P0 = 0x10000                                                         # dummy device pointers: nothing below reaches a launch


def _ram(**kw):
    p = L.RdRam()
    p.src, p.trg, p.lam, p.out_img, p.out_freq, p.workspace, p.tw_w, p.tw_h = (P0 * (i + 1) for i in range(8))
    p.trg_amp, p.dft_tables = None, None
    p.B, p.H, p.W, p.C, p.b = 2, 30, 40, 3, 3
    p.clip_lo, p.clip_hi, p.scale, p.div, p.offset, p.out_cstride, p.src_u8 = 0.0, 255.0, 1.0 / 127.5, 127.5, -1.0, 3, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize('code,kw', [
    (-1, dict(C=1)), (-1, dict(C=4)), (-1, dict(C=0)), (-1, dict(out_cstride=1)), (-1, dict(out_cstride=2)),
    (-2, dict(H=14)), (-2, dict(W=14)), (-2, dict(H=1030)), (-2, dict(W=1030)), (-2, dict(H=2048)), (-2, dict(W=2048)),
    (-2, dict(H=33, W=16, b=1)), (-2, dict(H=0)), (-2, dict(W=0)), (-2, dict(W=-16)), (-2, dict(H=4 ** 13)), (-2, dict(W=2 ** 30)),     # no plan is built for these
    (-3, dict(b=-1)), (-3, dict(b=15)), (-3, dict(H=40, W=30, b=15)), (-3, dict(H=15, W=15, b=8)), (-3, dict(H=16, W=16, b=8)),
    (-4, dict(src=None)), (-4, dict(trg=None, trg_amp=None)), (-4, dict(lam=None)), (-4, dict(out_img=None)),
    (-4, dict(out_freq=None)), (-4, dict(workspace=None)),
])
@pytest.mark.parametrize('dtype', [L.RD_F32, L.RD_BF16])
def test_rd_ram_mix_refusals_before_any_launch(code, kw, dtype):
    assert L.lib().rd_ram_mix(C.byref(_ram(**kw)), dtype, None) == code


def test_rd_ram_mix_null_descriptor_and_refusal_order():
    lib = L.lib()
    assert lib.rd_ram_mix(None, L.RD_F32, None) == -1
    assert lib.rd_ram_mix(C.byref(_ram(C=1, H=14, b=-1, src=None)), L.RD_F32, None) == -1     # C, then sides, then b, then pointers
    assert lib.rd_ram_mix(C.byref(_ram(H=14, b=-1, src=None)), L.RD_F32, None) == -2
    assert lib.rd_ram_mix(C.byref(_ram(b=-1, src=None)), L.RD_F32, None) == -3
    assert lib.rd_ram_mix(C.byref(_ram(src=None, out_cstride=2)), L.RD_F32, None) == -4


@pytest.mark.parametrize('kw', [dict(a=None), dict(t=None), dict(o=None), dict(b=-1), dict(b=15), dict(H=40, W=30, b=15),
                                dict(H=15, W=15, b=8), dict(H=16, W=16, b=8)])
def test_rd_ram_mutate_refusals(kw):
    a = dict(a=P0, t=2 * P0, o=3 * P0, C=3, H=30, W=40, b=3)
    a.update(kw)
    assert L.lib().rd_ram_mutate(a['a'], a['t'], a['o'], a['C'], a['H'], a['W'], a['b'], 0.5, None) == -1


@pytest.mark.parametrize('code,kw', [
    (-1, dict(img=None)), (-1, dict(amp=None)), (-1, dict(ws=None)), (-1, dict(C=0)), (-1, dict(C=-2)),
    (-2, dict(H=14)), (-2, dict(W=14)), (-2, dict(H=1030)), (-2, dict(W=2048)), (-2, dict(H=0)), (-2, dict(W=0)), (-2, dict(W=4 ** 13)),
])
def test_rd_ram_amp_refusals(code, kw):
    a = dict(img=P0, amp=2 * P0, ws=3 * P0, C=3, H=30, W=40)
    a.update(kw)
    assert L.lib().rd_ram_amp(a['img'], a['amp'], a['C'], a['H'], a['W'], a['ws'], 4 * P0, 5 * P0, None) == code


def test_dft_tables_are_offered_only_for_widths_of_16_pixel_steps_up_to_1024():
    lib = L.lib()
    for H, W, b in ((400, 250, 25), (27, 45, 2), (15, 15, 7), (243, 125, 12), (16, 24, 1), (2048, 16, 1), (16, 2048, 1),
                    (1025, 512, 51), (512, 1040, 51), (64, 64, -1)):
        assert int(lib.rd_ram_dft_tables_bytes(H, W, b)) == 0 == M.dft_tables_bytes(H, W, b), (H, W, b)
        assert lib.rd_ram_dft_tables(P0, H, W, b, None) == -1, (H, W, b)
    assert lib.rd_ram_dft_tables(None, 400, 400, 40, None) == -1
    for H, W, b in ((400, 400, 40), (16, 16, 1), (225, 16, 1), (24, 32, 2), (40, 1024, 4), (1024, 48, 4), (1024, 1024, 102),
                    (96, 800, 9), (256, 256, 127), (250, 400, 25)):
        assert int(lib.rd_ram_dft_tables_bytes(H, W, b)) == M.dft_tables_bytes(H, W, b) > 0, (H, W, b)


def test_workspace_sizes_equal_their_documented_formulas():
    lib = L.lib()
    for B, H, W, b in ((1, 9, 25, 0), (3, 27, 45, 2), (3, 250, 400, 25), (8, 400, 400, 40), (2, 1024, 1024, 102), (3, 256, 256, 127),
                       (3, 15, 15, 7)):
        KP = (b + 1 + 3) // 4 * 4
        assert int(lib.rd_ram_workspace(B, H, W, b)) == M.ram_workspace_bytes(B, H, W, b) == 3 * B * 3 * H * KP * 8
    assert M.ram_workspace_bytes(1, 9, 25, 0) == 3 * 3 * 9 * 4 * 8                       # b = 0: nkeep 1, KP 4
    for Cc, H, W in ((1, 9, 25), (3, 27, 45), (4, 243, 125), (3, 40, 1024), (1, 1024, 48)):
        KP = (W // 2 + 1 + 3) // 4 * 4
        assert int(lib.rd_ram_amp_workspace(Cc, H, W)) == M.amp_workspace_bytes(Cc, H, W) == Cc * H * KP * 8


# ------------------------------------------------------------------------------------------------------------- routes
def test_route_model_names_the_paths_the_edge_shapes_reach():
    """The branch conditions tests/test_gpu_ram_edges.py relies on, worked out once by hand from the launchers."""
    assert M.dft_route(72, 640) == dict(nks=40, RF_NJ=8, trips=2, idle_waves=0, last_block_rows=8, ragged_last_trip=True)
    assert M.dft_route(96, 800)['trips'] == 2 and M.dft_route(96, 800)['RF_NJ'] == 8 and M.dft_route(96, 800)['ragged_last_trip']
    assert M.dft_route(40, 1024) == dict(nks=64, RF_NJ=8, trips=2, idle_waves=0, last_block_rows=8, ragged_last_trip=False)
    assert [M.dft_route(16, w)['idle_waves'] for w in (16, 32, 48, 64)] == [3, 2, 1, 0]
    assert M.dft_route(225, 16)['last_block_rows'] == 1 and M.dft_route(16, 16)['last_block_rows'] == 16
    assert [M.dft_route(64, w)['RF_NJ'] for w in (256, 320, 384, 400, 448, 512)] == [4, 6, 6, 7, 7, 8]
    assert M.mix_route(256, 320) == dict(NW=0, NH=256, KT=4, ROWS=1, row_fwd='fft', last_row_block=1)
    assert M.mix_route(250, 400) == dict(NW=400, NH=0, KT=1, ROWS=8, row_fwd='fft', last_row_block=2)
    assert M.mix_route(512, 384, True) == dict(NW=384, NH=512, KT=4, ROWS=8, row_fwd='dft', last_row_block=8)
    assert M.mix_route(243, 125, True)['row_fwd'] == 'fft'
    assert [M.window_half_width(h, w, r) for h, w, r in ((9, 25, 0.1), (15, 15, 0.5), (256, 256, 0.499), (27, 45, 0.04))] == [0, 7, 127, 1]
