"""-m gpu: the RAM kernels (csrc/ram_fft.hip, csrc/ram_dft.hip, ramdsir/ram.py) at every plan and window edge, against oracle/ram.py
in float64 with the window ratio passed as `L`.

test_gpu_ram.py holds the kernels to the reference at nine small even fixture shapes and the four square benchmark sides.  Here:
odd sides (run-time plans of radix 3 / 5 only: the fftshift centre floor(n / 2), the mirror writes of ram_col_amp_kernel, the
(H + 1) / 2 split of ram_mutate_kernel), b = 0 (nkeep 1, KP 4), the whole spectrum as the window (2 b + 1 == H; b = 127 at side 256,
the last bin of the real-input row pass), a compile-time plan on one axis with a run-time plan on the other in both orders, the
matrix-core row pass off the benchmark sides (a second, ragged trip of its k-step loop for W > 512; waves with no k-step at W = 16 /
32 / 48; H < 32 and a last 32-row block of one row; uint8 pixels at small sides), sides of 1024, `trg_amp` indexed by sample in a
batch, every output stride between sentinels, and a workspace of exactly rd_ram_workspace bytes holding NaN.  Which template values
(NW, NH, KT, ROWS, RF_NJ) a shape gets is restated in tests/ram_plan_model.py and asserted per case.

Tolerances are the project's (test_gpu_ram.py): 2e-3 on the 0..255 scale against the float64 oracle, 2e-4 between two row passes,
rtol 2e-5 / atol 2e-6 max for amplitudes.  The first is justified by the reference's own float32-vs-float64 spread, which each mix
case measures for its shape (oracle/ram.py with dtype float32 against float64) and asserts to be at most 1e-3, half the bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ramdsir import _lib as L          # noqa: E402
from ramdsir import ram as R           # noqa: E402
from oracle import ram as OR          # noqa: E402
import ram_plan_model as M             # noqa: E402

DEV = 'cuda:0'
GUARD, SENT, FILL = 4096, 0xA5, 0x5A
B = 3
LAM = (0.1, 0.5, 1.0)
TOL_ORACLE, TOL_PASSES, MAX_SPREAD = 2e-3, 2e-4, 1e-3          # on the 0..255 scale

# (H, W, ratio): which edge each shape is there for, and the reference's own spread (float32 vs float64 oracle, 0..255 scale) on
# these inputs as the test measures it on the host; every one is below MAX_SPREAD, so every shape keeps the project's 2e-3.
SHAPES = [
    (9, 25, 0.1),          # 6.1e-5  odd, b = 0: nkeep 1, KP 4, a 1 x 1 window
    (15, 15, 0.1),         # 6.1e-5  odd, radix 3 x 5 on both axes, b = 1
    (27, 45, 0.1),         # 7.6e-5  odd, H != W
    (75, 81, 0.1),         # 1.6e-4
    (243, 125, 0.1),       # 3.2e-4  3^5 x 5^3
    (15, 15, 0.5),         # 7.6e-5  b = 7: 2 b + 1 == H == W, the whole spectrum is the window
    (256, 256, 0.499),     # 4.7e-4  b = 127: 2 b + 1 == 255, the last bin of the real-input row pass (kx <= b < M = 128); KP = 128
    (256, 320, 0.1),       # 5.5e-4  compile-time column plan (NH = 256, KT = 4), run-time row plan (NW = 0, ROWS = 1); RF_NJ = 6
    (250, 400, 0.1),       # 5.9e-4  run-time column plan (NH = 0, KT = 1), compile-time row plan (NW = 400, ROWS = 8: last block of 2)
    (512, 384, 0.1),       # 8.2e-4  two different compile-time plans
    (72, 640, 0.1),        # 4.3e-4  W > 512: RF_NJ = 8, a second trip of 8 k-steps of which 2 exist per wave
    (96, 800, 0.1),        # 5.2e-4  50 k-steps: the second trip is ragged across the waves
    (40, 1024, 0.1),       # 3.9e-4  the documented maximum on the row axis: 64 k-steps, two full trips; five radix-4 stages
    (1024, 48, 0.1),       # 4.2e-4  the maximum on the column axis; three k-steps: wave 3 idle
    (16, 16, 0.1),         # 4.6e-5  one k-step: waves 1..3 idle; H < 32
    (24, 32, 0.1),         # 6.1e-5  two k-steps; H < 32
    (64, 64, 0.1),         # 1.4e-4  four k-steps, one per wave; two full 32-row blocks
    (225, 16, 0.1),        # 1.4e-4  an eighth 32-row block of one row (33 x 16, the smallest such shape, is refused: 33 = 3 x 11)
]


class Guarded:
    """`nbytes` of device memory between two GUARD-byte sentinel regions; the payload is filled with the byte `fill`."""
    def __init__(self, nbytes, fill=FILL):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.payload = self.raw[GUARD:GUARD + self.nbytes]
        self.payload.fill_(fill)

    def view(self, dtype, *shape):
        return self.payload.view(dtype).view(*shape)

    def ptr(self):
        return self.payload.data_ptr()

    def intact(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.nbytes:] == SENT).all())


def nan_workspace(nbytes):
    ws = Guarded(nbytes)
    ws.view(torch.float32, -1).fill_(float('nan'))
    return ws


MIN_SRC_AMP = 0.14                     # x sqrt(HW): the smallest in-window |F_src| a case may hold (a typical bin is 74 sqrt(HW))


def window_src_amps(src, b):
    """|F_src| of the window bins |ky| <= b, |kx| <= b, [B * 3 planes][bins], float64."""
    _, H, W, _ = src.shape
    fs = np.abs(np.fft.fft2(src.astype(np.float64).transpose(0, 3, 1, 2)))
    ky, kx = np.abs(np.fft.fftfreq(H, 1.0 / H)) <= b, np.abs(np.fft.fftfreq(W, 1.0 / W)) <= b
    return fs[:, :, ky][:, :, :, kx].reshape(B * 3, -1)


@functools.lru_cache(maxsize=None)
def inputs(H, W, ratio=0.1):
    """Integer pixels 0..255; channel 2 of source 1 is all zero (|F_src| == 0 inside a batch).  The mix divides by |F_src|, so the
    error of a bin grows as 1 / |F_src|: a case is the first draw of its generator in which no other window bin is below MIN_SRC_AMP
    sqrt(HW) (one bin in 3e5 is; only the 5e5 bins of the whole-spectrum window at 256 x 256 ever need a second draw)."""
    rng = np.random.RandomState(H * 1000 + W)
    for _ in range(64):
        src = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        trg = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        src[1, :, :, 2] = 0
        amps = window_src_amps(src, M.window_half_width(H, W, ratio))
        if amps[5].max() == 0 and np.delete(amps, 5, 0).min() >= MIN_SRC_AMP * np.sqrt(H * W):
            return src, trg
    raise AssertionError('no well-conditioned draw')


@functools.lru_cache(maxsize=None)
def fundus_oracle(H, W, ratio):
    """(img, frq64, spread): OR.ram_fundus per sample in float64, and the largest float32-vs-float64 difference of the reference
    itself on the 0..255 scale."""
    src, trg = inputs(H, W, ratio)
    f32 = [s.astype(np.float32) for s in src], [t.astype(np.float32) for t in trg]
    r64 = [OR.ram_fundus(f32[0][i], f32[1][i], LAM[i], L=ratio) for i in range(B)]
    r32 = [OR.ram_fundus(f32[0][i], f32[1][i], LAM[i], L=ratio, dtype=np.float32) for i in range(B)]
    spread = max(float(np.abs(a[1].astype(np.float64) - b[1]).max()) for a, b in zip(r32, r64)) * 127.5
    return np.stack([r[0] for r in r64]), np.stack([r[1] for r in r64]), spread


class Mix:
    """One rd_ram_mix call through RamMixer.bind with both outputs between sentinels (prefilled with FILL bytes) and a workspace of
    exactly rd_ram_workspace bytes between sentinels holding NaN."""
    def __init__(self, src, trg, lam, H, W, ratio=0.1, dtype=torch.float32, cs=3, tables=True, clip=True, trg_amp=None):
        self.m = m = R.RamMixer(B, H, W, dtype, DEV, 'fundus', ratio=ratio)
        assert m.b == M.window_half_width(H, W, ratio)
        self.has_tables = m.tables is not None
        if not tables:
            m.p.dft_tables = None
        if not clip:                                            # as source_to_target_freq_gpu: no clip, no scaling
            m.p.clip_lo, m.p.clip_hi, m.p.scale, m.p.div, m.p.offset = -3.0e38, 3.0e38, 1.0, 0.0, 0.0
        nws = int(L.lib().rd_ram_workspace(B, H, W, m.b))
        assert nws == M.ram_workspace_bytes(B, H, W, m.b)
        self.ws = nan_workspace(nws)
        m.p.workspace = self.ws.ptr()
        esz = 2 if dtype == torch.bfloat16 else 4
        self.oi, self.of = Guarded(B * H * W * cs * esz), Guarded(B * H * W * cs * esz)
        self.img, self.frq = self.oi.view(dtype, B, H, W, cs), self.of.view(dtype, B, H, W, cs)
        self.src = torch.from_numpy(src).to(DEV)
        self.trg = torch.from_numpy(trg).to(DEV) if trg is not None else None
        self.lam = torch.tensor(lam, dtype=torch.float32, device=DEV)
        m.bind(self.src, self.trg, self.lam, self.img, self.frq, trg_amp=trg_amp)
        assert m.p.out_cstride == cs
        self.run()

    def run(self):
        self.m.run()
        torch.cuda.synchronize()
        assert self.ws.intact(), 'a sentinel region around the workspace was written'
        assert self.oi.intact() and self.of.intact(), 'a sentinel region around an output was written'
        return self

    def out(self):
        return self.img.cpu(), self.frq.cpu()


def host_img(src_u8):
    x = src_u8.astype(np.float32)
    x /= 127.5
    x -= 1.0                                                     # fundus.py:217-218, float32
    return x


# ------------------------------------------------------------------------------------------------ a. mix against the oracle
@pytest.mark.parametrize('H,W,ratio', SHAPES, ids=lambda v: str(v))
def test_mix_matches_float64_oracle_over_the_shape_table(H, W, ratio):
    src, trg = inputs(H, W, ratio)
    ref_img, ref_frq, spread = fundus_oracle(H, W, ratio)
    print('reference float32-vs-float64 spread at %d x %d, ratio %g: %.3g' % (H, W, ratio, spread))
    assert spread <= MAX_SPREAD
    b = M.window_half_width(H, W, ratio)
    want_tables = W % 16 == 0
    assert (int(L.lib().rd_ram_dft_tables_bytes(H, W, b)) > 0) == want_tables
    assert np.array_equal(ref_img, host_img(src).transpose(0, 3, 1, 2))
    # the clip runs, the zero channel's window is exactly zero, and no other in-window source bin is small: no case is ill-conditioned
    assert ((ref_frq == -1) | (ref_frq == 1)).mean() > 0.004
    amps = window_src_amps(src, b)
    assert amps.shape[1] == (2 * b + 1) ** 2 and amps[5].max() == 0 and np.delete(amps, 5, 0).min() >= MIN_SRC_AMP * np.sqrt(H * W)
    kinds = [('fp32', src.astype(np.float32), trg.astype(np.float32), True), ('uint8 without tables', src, trg, False)]
    if want_tables:
        kinds.append(('uint8 with tables', src, trg, True))
    got = {}
    for name, s, t, tables in kinds:
        mx = Mix(s, t, LAM, H, W, ratio, tables=tables)
        assert mx.has_tables == want_tables, 'the mixer reports tables for exactly the widths of whole 16-pixel steps'
        img, frq = (v.numpy() for v in mx.out())
        got[name] = frq
        assert np.array_equal(img, host_img(src)), name          # bit for bit
        for i in range(B):
            err = np.abs(frq[i].transpose(2, 0, 1).astype(np.float64) - ref_frq[i]).max() * 127.5
            print('  %-22s sample %d (lam %.1f): max error %.3g' % (name, i, LAM[i], err))
            assert err <= TOL_ORACLE, (name, i, err)
        assert np.array_equal(frq[2], img[2]), name + ': lam = 1 is the identity, exactly'
        assert np.abs(frq[:2] - img[:2]).max() > 0.05, name + ': the mix did something'
    if want_tables:
        d = np.abs(got['uint8 with tables'] - got['uint8 without tables']).max() * 127.5
        print('  matrix-core row pass vs FFT row pass: %.3g' % d)
        assert d <= TOL_PASSES


def test_shape_table_reaches_the_paths_it_names():
    """The branch conditions of the launchers (restated in tests/ram_plan_model.py) at the table's shapes."""
    rt = {(H, W): (M.mix_route(H, W, True), M.dft_route(H, W)) for H, W, _ in SHAPES}
    assert all(H % 2 and W % 2 and not rt[H, W][0]['NW'] and not rt[H, W][0]['NH'] for H, W in ((9, 25), (15, 15), (27, 45), (75, 81), (243, 125)))
    assert M.window_half_width(9, 25) == 0 and M.window_half_width(15, 15, 0.5) == 7 and M.window_half_width(256, 256, 0.499) == 127
    assert (rt[256, 320][0]['NH'], rt[256, 320][0]['NW'], rt[256, 320][0]['KT'], rt[256, 320][0]['ROWS']) == (256, 0, 4, 1)
    assert (rt[250, 400][0]['NH'], rt[250, 400][0]['NW'], rt[250, 400][0]['KT'], rt[250, 400][0]['last_row_block']) == (0, 400, 1, 2)
    assert (rt[512, 384][0]['NH'], rt[512, 384][0]['NW']) == (512, 384)
    assert [rt[s][1]['RF_NJ'] for s in ((256, 320), (250, 400), (512, 384), (72, 640), (96, 800), (40, 1024), (16, 16))] == [6, 7, 6, 8, 8, 8, 4]
    assert [rt[s][1]['trips'] for s in ((72, 640), (96, 800), (40, 1024))] == [2, 2, 2]
    assert rt[72, 640][1]['ragged_last_trip'] and rt[96, 800][1]['ragged_last_trip'] and not rt[40, 1024][1]['ragged_last_trip']
    assert [rt[s][1]['idle_waves'] for s in ((16, 16), (225, 16), (24, 32), (1024, 48), (64, 64))] == [3, 3, 2, 1, 0]
    assert [rt[s][1]['last_block_rows'] for s in ((16, 16), (24, 32), (225, 16), (250, 400), (64, 64))] == [16, 24, 1, 26, 32]


# ------------------------------------------------------------------------------------------------ b. output layouts and bounds
LAYOUT_SHAPES = [(27, 45), (250, 400), (256, 256)]


@functools.lru_cache(maxsize=None)
def dense_fp32(H, W, u8):
    src, trg = inputs(H, W)
    if not u8:
        src, trg = src.astype(np.float32), trg.astype(np.float32)
    return Mix(src, trg, LAM, H, W).out()


@pytest.mark.parametrize('H,W', LAYOUT_SHAPES)
@pytest.mark.parametrize('dtype,cs', [(torch.float32, 3), (torch.float32, 4), (torch.float32, 5), (torch.bfloat16, 3), (torch.bfloat16, 8),
                                      (torch.bfloat16, 9)], ids=lambda v: str(v).replace('torch.', ''))
@pytest.mark.parametrize('u8', [False, True], ids=['fp32px', 'u8px'])
def test_output_layouts_between_sentinels(H, W, dtype, cs, u8):
    """Channels 0..2 of every layout are the dense fp32 result (bf16: that float converted once, round to nearest even), the padding
    channels of a 16-byte slot are zero, those of any other stride are untouched, nothing outside the tensors is written, the
    workspace needs no more than rd_ram_workspace bytes and nothing in it is read before it is written, and a second call gives the
    same bytes."""
    src, trg = inputs(H, W)
    if not u8:
        src, trg = src.astype(np.float32), trg.astype(np.float32)
    ref_img, ref_frq = dense_fp32(H, W, u8)
    mx = Mix(src, trg, LAM, H, W, dtype=dtype, cs=cs)
    slot = 16 // (2 if dtype == torch.bfloat16 else 4)
    first = mx.oi.payload.cpu(), mx.of.payload.cpu()
    for name, got, ref in (('img', mx.img.cpu(), ref_img), ('frq', mx.frq.cpu(), ref_frq)):
        want = ref.to(dtype)                                     # fp32: the same floats; bf16: torch converts RNE
        assert torch.equal(got[..., :3].contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), name
        assert not torch.isnan(got[..., :3].float()).any()
        if cs > 3:
            pad = got[..., 3:].contiguous().view(torch.uint8)
            assert bool((pad == (0 if cs == slot else FILL)).all()), name + ': padding channels'
    mx.ws.view(torch.float32, -1).fill_(float('nan'))
    mx.run()
    assert torch.equal(mx.oi.payload.cpu(), first[0]) and torch.equal(mx.of.payload.cpu(), first[1])


# ------------------------------------------------------------------------------------------------ c. trg_amp in a batch
@pytest.mark.parametrize('H,W,u8', [(27, 45, False), (250, 400, False), (256, 320, False), (256, 320, True)])
def test_trg_amp_is_indexed_by_sample(H, W, u8):
    """RamMixer.bind(..., trg_amp=) with B = 3 distinct partners: each sample is mixed with its OWN partner's amplitude spectrum
    (float64 oracle amplitudes cast to fp32), and agrees with the image-partner path.  No clipping, no scaling."""
    lam = (0.1, 0.5, 0.9)
    src, trg = inputs(H, W)
    amp64 = [OR.extract_amp_spectrum(trg[i].astype(np.float32).transpose(2, 0, 1)) for i in range(B)]
    # numpy keeps the HWC memory order of the transposed image through fft2, abs and stack: the kernel reads dense [B][3][H][W]
    amp = torch.from_numpy(np.ascontiguousarray(np.stack(amp64), dtype=np.float32)).to(DEV)
    assert amp.shape == (B, 3, H, W) and amp.is_contiguous()
    out = torch.empty(B, H, W, 3, device=DEV)
    strided = amp.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)       # the same values, another memory order
    for bad in (strided, amp.double(), amp[:1], amp[:, :, :, :-1].contiguous()):
        with pytest.raises(AssertionError, match='trg_amp'):                 # refused, not misread
            R.RamMixer(B, H, W, torch.float32, DEV, 'fundus').bind(torch.from_numpy(src.astype(np.float32)).to(DEV), None,
                                                                   torch.tensor(lam, device=DEV), out, out, trg_amp=bad)
    s, t = (src, trg) if u8 else (src.astype(np.float32), trg.astype(np.float32))
    by_amp = Mix(s, None, lam, H, W, clip=False, trg_amp=amp)
    assert by_amp.has_tables == (W % 16 == 0)
    img_a, frq_a = (v.numpy() for v in by_amp.out())
    img_i, frq_i = (v.numpy() for v in Mix(s, t, lam, H, W, clip=False).out())
    assert np.array_equal(img_a, src.astype(np.float32)) and np.array_equal(img_i, img_a)
    for i in range(B):
        ref = OR.source_to_target_freq(src[i].astype(np.float32), amp64[i], lam[i], L=0.1)
        err = np.abs(frq_a[i] - ref).max()
        other = min(np.abs(frq_a[i] - OR.source_to_target_freq(src[i].astype(np.float32), amp64[j], lam[i], L=0.1)).max()
                    for j in range(B) if j != i)
        print('sample %d: error vs its own partner %.3g, vs the nearest other partner %.3g' % (i, err, other))
        assert err <= TOL_ORACLE, (i, err)
        assert other > 50 * TOL_ORACLE, 'the partners are distinct enough to tell a wrong index'
        assert np.abs(frq_a[i] - frq_i[i]).max() <= TOL_PASSES, i


# ------------------------------------------------------------------------------------------------ d. rd_ram_amp / rd_ram_mutate
TRIO_SHAPES = [(9, 25), (15, 15), (27, 45), (75, 81), (24, 32), (243, 125), (40, 1024), (1024, 48)]


@pytest.mark.parametrize('H,W', TRIO_SHAPES)
@pytest.mark.parametrize('Cc', [1, 3, 4])
def test_amp_matches_float64_fft2_between_sentinels(Cc, H, W):
    """|fft2| of the full spectrum: the kernel computes columns kx <= W / 2 and writes each one's mirror (H - ky) % H, W - kx -- on an
    odd axis there is no self-mirrored Nyquist column / row."""
    lib = L.lib()
    x = np.random.RandomState(Cc * 7 + H * 1000 + W).randint(0, 256, (Cc, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    nws = int(lib.rd_ram_amp_workspace(Cc, H, W))
    assert nws == M.amp_workspace_bytes(Cc, H, W)
    ws, out = nan_workspace(nws), nan_workspace(Cc * H * W * 4)
    tw_w, tw_h = R._twiddle(W, DEV), R._twiddle(H, DEV)
    L.check(lib.rd_ram_amp(xd.data_ptr(), out.ptr(), Cc, H, W, ws.ptr(), tw_w.data_ptr(), tw_h.data_ptr(), None), 'rd_ram_amp')
    torch.cuda.synchronize()
    assert ws.intact() and out.intact(), 'a sentinel region around the workspace / the amplitudes was written'
    ref = np.abs(np.fft.fft2(x.astype(np.float64), axes=(-2, -1)))
    np.testing.assert_allclose(out.view(torch.float32, Cc, H, W).cpu().numpy(), ref, rtol=2e-5, atol=2e-6 * ref.max())


@pytest.mark.parametrize('H,W', TRIO_SHAPES)
@pytest.mark.parametrize('Cc', [1, 3, 4])
def test_mutate_window_is_the_oracles_exactly(Cc, H, W):
    """at = as + 1000: an element is changed if and only if it lies in the oracle's window; outside the result is `as` bit for bit,
    inside within 3 x 2^-24 x (|as| lam + |at| (1 - lam)) of the float64 lerp (two roundings or one fma, and the rounding of
    1 - lam).  Window half-widths: the ratios 0.1 and 0.04, b = 0, and the largest legal b."""
    lib = L.lib()
    lam = float(np.float32(0.3))
    a_s = np.random.RandomState(Cc + H * 1000 + W).uniform(1.0, 1e4, (Cc, H, W)).astype(np.float32)
    a_t = a_s + np.float32(1000.0)
    ad, td = torch.from_numpy(a_s).to(DEV), torch.from_numpy(a_t).to(DEV)
    n = min(H, W)
    for b in sorted({M.window_half_width(H, W, 0.1), M.window_half_width(H, W, 0.04), 0, (n - 1) // 2}):
        ratio = (b + 0.5) / n
        assert OR.window_half_width(H, W, ratio) == b and 2 * b + 1 <= n
        out = nan_workspace(Cc * H * W * 4)
        L.check(lib.rd_ram_mutate(ad.data_ptr(), td.data_ptr(), out.ptr(), Cc, H, W, b, lam, None), 'rd_ram_mutate')
        torch.cuda.synchronize()
        assert out.intact()
        got = out.view(torch.float32, Cc, H, W).cpu().numpy()
        ref = OR.low_freq_mutate(a_s.astype(np.float64), a_t.astype(np.float64), lam, L=ratio)
        inside = ref != a_s
        assert int(inside.sum()) == Cc * (2 * b + 1) ** 2
        assert np.array_equal(got != a_s, inside), 'b = %d: the set of changed elements is the oracle window' % b
        assert np.array_equal(got[~inside], a_s[~inside])
        bound = 3 * 2.0 ** -24 * (np.abs(a_s) * lam + np.abs(a_t) * (1 - lam))
        assert (np.abs(got.astype(np.float64) - ref) <= bound)[inside].all(), 'b = %d' % b
        if b == (n - 1) // 2 and H == W:
            assert int((~inside).sum()) == (0 if n % 2 else Cc * (2 * n - 1))     # odd square: the whole spectrum is the window


def test_free_functions_on_odd_sides_and_a_given_ratio():
    """The array-in / array-out trio of ramdsir/ram.py (what dataset/fundus.py's free functions call) at an odd shape with a ratio of
    its own: amplitude, mutate and source_to_target_freq chained, against the float64 oracle."""
    H, W, ratio, lam = 27, 45, 0.2, 0.4
    src, trg = inputs(H, W)
    s, t = src[0].astype(np.float32), trg[0].astype(np.float32)
    amp = R.extract_amp_spectrum_gpu(t.transpose(2, 0, 1))
    ref_amp = OR.extract_amp_spectrum(t.transpose(2, 0, 1))
    np.testing.assert_allclose(amp.cpu().numpy(), ref_amp, rtol=2e-5, atol=2e-6 * ref_amp.max())
    frq = R.source_to_target_freq_gpu(s, ref_amp.astype(np.float32), lam, ratio=ratio).cpu().numpy()
    assert np.abs(frq - OR.source_to_target_freq(s, ref_amp, lam, L=ratio)).max() <= TOL_ORACLE
    a_s = OR.extract_amp_spectrum(s.transpose(2, 0, 1))
    mut = R.low_freq_mutate_gpu(a_s.astype(np.float32), ref_amp.astype(np.float32), lam, ratio=ratio).cpu().numpy()
    np.testing.assert_allclose(mut, OR.low_freq_mutate(a_s, ref_amp, lam, L=ratio), rtol=1e-5, atol=1e-6 * ref_amp.max())
