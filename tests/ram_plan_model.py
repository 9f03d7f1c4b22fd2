"""numpy restatement of the host and index arithmetic of the RAM FFT kernels (csrc/ram_fft.hip, csrc/ram_dft.h): make_plan, the
float32 quotients of fft_runtime, the compile-time radix lists, which kernel a side gets, and the workspace / table sizes.  No GPU, no
library; tests/test_cpu_ram_plan.py holds it to integer arithmetic and to the library's own answers, tests/test_gpu_ram_edges.py
uses it to say which code path a shape reaches."""
import numpy as np

MAX_SIDE, MAX_STAGES = 1024, 12
# fft_fixed<N>: the radix list of every compile-time plan.  The real-input row pass of a compile-time side W runs FIXED[W / 2]
# against the twiddle table of W (TWS = 2); columns and the row inverse run FIXED[side] (TWS = 1)
FIXED = {128: (4, 4, 4, 2), 192: (4, 4, 4, 3), 200: (4, 2, 5, 5), 256: (4, 4, 4, 4), 384: (4, 4, 4, 2, 3), 400: (4, 4, 5, 5),
         512: (4, 4, 4, 4, 2)}
FIXED_SIDES = (256, 384, 400, 512)            # RD_BY_SIDE: the sides whose kernels are instantiated with a compile-time plan
BATCHES = (1, 2, 3)                           # transforms per workgroup of the run-time launchers: one plane (rd_ram_amp) or one column
#                                               with trg_amp; 2 KT columns (KT = 1) or the 2 inverse rows; the 3 channels of one image row


def make_plan(N):
    """(ok, radix list) as make_plan: 4s, then 2s, 3s, 5s; refused for another factor, N < 1, N > 1024 or more than 12 stages."""
    if N < 1 or N > MAX_SIDE:
        return False, []
    radix, n = [], N
    for r in (4, 2, 3, 5):
        while n % r == 0:
            radix.append(r)
            n //= r
    return n == 1 and len(radix) <= MAX_STAGES and N <= MAX_SIDE, radix


def legal_sides():
    return [N for N in range(1, MAX_SIDE + 1) if make_plan(N)[0]]


def stages(N, radix):
    """(R, nb, Ns, tstep) of every stage, as fft_runtime / stage_fixed compute them."""
    out, Ns = [], 1
    for R in radix:
        out.append((R, N // R, Ns, N // (Ns * R)))
        Ns *= R
    assert Ns == N
    return out


def runtime_split(jj, nb, Ns):
    """fft_runtime's float32 quotients: t = (int)(((float)jj + 0.5f) * (1.0f / (float)nb)), j = jj - t * nb, then q from j and Ns
    likewise, k = j - q * Ns.  Every operation rounded to float32 on its own (a sum followed by a product has no fused form)."""
    f = np.float32
    inv_nb, inv_Ns = f(1.0) / f(nb), f(1.0) / f(Ns)
    t = ((jj.astype(f) + f(0.5)) * inv_nb).astype(np.int32)          # all values >= 0: the conversion truncates
    j = jj - t * nb
    q = ((j.astype(f) + f(0.5)) * inv_Ns).astype(np.int32)
    return t, j, q, j - q * Ns


def window_half_width(h, w, ratio=0.1):
    return int(np.floor(min(h, w) * ratio))


def pad4(v):
    return (v + 3) // 4 * 4


def ram_workspace_bytes(B, H, W, b):
    """rd_ram_workspace: rowspec [2B][3][H][KP] + colout [B][3][H][KP] complex64, KP = b + 1 padded to 4."""
    return 3 * B * 3 * H * pad4(b + 1) * 8


def amp_workspace_bytes(C, H, W):
    """rd_ram_amp_workspace: [C][H][KP] complex64, KP = W / 2 + 1 padded to 4."""
    return C * H * pad4(W // 2 + 1) * 8


def dft_ok(H, W, b):
    return W % 16 == 0 and W <= MAX_SIDE and H <= MAX_SIDE and b >= 0


def dft_tables_bytes(H, W, b):
    """rd_ram_dft_tables_bytes: [ntile][nks][3 terms][64 lanes] uint4, or 0 when the geometry runs the FFT kernels."""
    return ((b + 1 + 15) // 16) * (W // 16) * 3 * 64 * 16 if dft_ok(H, W, b) else 0


def dft_route(H, W):
    """The matrix-core row pass of a width: (RF_NJ chosen by ram_dft_row_fwd, trips of `for (ks0 = wave; ks0 < nks; ks0 += 4 * RF_NJ)`
    that wave 0 makes, waves that have no k-step at all, rows in the last 32-row block)."""
    nks = W // 16
    nj = (nks + 3) // 4
    RF_NJ = 4 if nj <= 4 else 6 if nj <= 6 else 7 if nj == 7 else 8
    return dict(nks=nks, RF_NJ=RF_NJ, trips=-(-nks // (4 * RF_NJ)), idle_waves=max(0, 4 - nks), last_block_rows=(H - 1) % 32 + 1,
                ragged_last_trip=nks % (4 * RF_NJ) != 0)


def mix_route(H, W, u8_tables=False):
    """Template values rd_ram_mix's launchers choose in the product build: NW of the row passes, NH / KT of the column pass, ROWS of
    the row forward / inverse kernels."""
    NW, NH = (W if W in FIXED_SIDES else 0), (H if H in FIXED_SIDES else 0)
    r = dict(NW=NW, NH=NH, KT=4 if NH else 1, ROWS=8 if NW else 1, row_fwd='dft' if u8_tables and W % 16 == 0 else 'fft')
    r['last_row_block'] = (H - 1) % r['ROWS'] + 1
    return r
