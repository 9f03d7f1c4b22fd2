// tb_grid.hip -- rd_tb_grids: the TensorBoard image grids of one logging iteration (code/train.py:306-329 Fundus, :475-496 Prostate;
// train.py --tb_images, ramdsir/tb_images.py), composed from the training step's resident buffers into uint8 HWC images.
//
// Two launches: (1) per grid, RD_TB_PARTS workgroups each reduce a strided share of the selection (after the transform) to one
// (min, max) pair in the workspace -- no atomics, nothing to initialise; (2) one thread per grid pixel folds the RD_TB_PARTS pairs of
// its grid (one per lane of the first wave), normalises, scales by 255, truncates and stores three bytes.  Both passes read the
// source through the same fetch(), so the values that were measured are the values that are normalised.
#include "common.h"
#include "../../include/ramdsir.h"

namespace {

struct GridArgs {
    rd_tb_grid_t g[RD_TB_MAX_GRIDS];
    int n;
};

// the 21 "pascal" colours of the reference's decode_segmap (code/utils/utils.py:285-295), class 0 first
__constant__ unsigned char tb_palette[RD_TB_PALETTE][3] = {
    {0, 0, 0},     {128, 0, 0},   {0, 128, 0},    {128, 128, 0},  {0, 0, 128},    {128, 0, 128},   {0, 128, 128},
    {128, 128, 128}, {64, 0, 0},  {192, 0, 0},    {64, 128, 0},   {192, 128, 0},  {64, 0, 128},    {192, 0, 128},
    {64, 128, 128}, {192, 128, 128}, {0, 64, 0},  {128, 64, 0},   {0, 192, 0},    {128, 192, 0},   {0, 64, 128}};

__device__ __forceinline__ void palette_rgb(long long cls, float* v) {
    // a class outside the palette stays black, as decode_segmap leaves it (utils.py:327-330)
    const bool ok = cls >= 0 && cls < RD_TB_PALETTE;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ok ? (float)((double)tb_palette[ok ? cls : 0][c] / 255.0) : 0.f;
}

__device__ __forceinline__ float load_elem(const rd_tb_grid_t& g, long long off) {
    return g.etype == RD_TB_BF16 ? (float)((const bf16_t*)g.src)[off] : ((const float*)g.src)[off];
}

__device__ __forceinline__ float transform(int t, float x) {
    if (t == RD_TB_SIGMOID) return 1.f / (1.f + expf(-x));
    if (t == RD_TB_TANH) return tanhf(x);
    return x;
}

// the three channel values of pixel (y, x) of tile k, after the transform (a one-channel selection replicated, make_grid)
__device__ __forceinline__ void fetch(const rd_tb_grid_t& g, int k, int y, int x, float* v) {
    const long long base = (long long)g.sample[k] * g.stride_n + (long long)y * g.stride_h + (long long)x * g.stride_w;
    if (g.transform == RD_TB_LABEL) {
        palette_rgb(((const long long*)g.src)[base], v);
        return;
    }
    if (g.transform == RD_TB_ARGMAX) {
        float best = load_elem(g, base + (long long)g.c0 * g.stride_c);
        int cls = 0;
        for (int c = 1; c < g.nc; ++c) {
            const float l = load_elem(g, base + (long long)(g.c0 + c) * g.stride_c);
            if (l > best) { best = l; cls = c; }            // strict: the lowest index wins a tie (torch.max)
        }
        palette_rgb(cls, v);
        return;
    }
    if (g.slot) {
        // NHWC with the channel vector padded to one 16-byte slot (the step's input / logits buffers): one load per pixel
        float f[8];
        const uint4 u = *(const uint4*)((const char*)g.src + base * (g.etype == RD_TB_BF16 ? 2 : 4));
        if (g.etype == RD_TB_BF16) Slot<bf16_t>::unpack(u, f); else Slot<float>::unpack(u, f);
        float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {                       // (constant indices only: f stays in registers)
            if (c == g.c0) s[0] = f[c];
            if (c == g.c0 + 1) s[1] = f[c];
            if (c == g.c0 + 2) s[2] = f[c];
        }
        v[0] = transform(g.transform, s[0]);
        v[1] = g.nc == 3 ? transform(g.transform, s[1]) : v[0];
        v[2] = g.nc == 3 ? transform(g.transform, s[2]) : v[0];
        return;
    }
    v[0] = transform(g.transform, load_elem(g, base + (long long)g.c0 * g.stride_c));
    v[1] = g.nc == 3 ? transform(g.transform, load_elem(g, base + (long long)(g.c0 + 1) * g.stride_c)) : v[0];
    v[2] = g.nc == 3 ? transform(g.transform, load_elem(g, base + (long long)(g.c0 + 2) * g.stride_c)) : v[0];
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

constexpr int TB_THREADS = 256;

// grid (RD_TB_PARTS, n grids): ws[grid][part] = (min, max) of the part's share of the selection
__global__ __launch_bounds__(TB_THREADS) void tb_minmax_kernel(GridArgs a, float2* __restrict__ ws) {
    const rd_tb_grid_t& g = a.g[blockIdx.y];
    if (!g.normalize) return;
    const int hw = g.H * g.W, total = g.n * hw;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int i = blockIdx.x * TB_THREADS + threadIdx.x; i < total; i += RD_TB_PARTS * TB_THREADS) {
        const int k = i / hw, r = i - k * hw, y = r / g.W;
        float v[3];
        fetch(g, k, y, r - y * g.W, v);
        lo = fminf(lo, fminf(v[0], fminf(v[1], v[2])));
        hi = fmaxf(hi, fmaxf(v[0], fmaxf(v[1], v[2])));
    }
    __shared__ float s_lo[TB_THREADS / 64], s_hi[TB_THREADS / 64];
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TB_THREADS / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
        ws[blockIdx.y * RD_TB_PARTS + blockIdx.x] = make_float2(lo, hi);
    }
}

// grid (blocks of TB_THREADS grid pixels, n grids): one thread per pixel of the uint8 HWC grid
__global__ __launch_bounds__(TB_THREADS) void tb_compose_kernel(GridArgs a, const float2* __restrict__ ws) {
    static_assert(RD_TB_PARTS == 64, "one (min, max) pair per lane of a wave");
    const rd_tb_grid_t& g = a.g[blockIdx.y];
    const int gh = g.n == 1 ? g.H : g.H + 4, gw = g.n == 1 ? g.W : g.n * (g.W + 2) + 2;
    if ((long long)blockIdx.x * TB_THREADS >= (long long)gh * gw) return;          // (whole block: no barrier is skipped by a part of it)
    __shared__ float s_lo, s_d;
    if (g.normalize && threadIdx.x < 64) {
        const float2 p = ws[blockIdx.y * RD_TB_PARTS + threadIdx.x];
        const float lo = wave_min(p.x), hi = wave_max(p.y);
        if (threadIdx.x == 0) {
            s_lo = lo;
            s_d = (float)fmax((double)hi - (double)lo, 1e-5);                      // torchvision: div_(max(high - low, 1e-5))
        }
    }
    __syncthreads();
    const int p = blockIdx.x * TB_THREADS + threadIdx.x;
    if (p >= gh * gw) return;
    const int gy = p / gw, gx = p - gy * gw;
    int k = 0, y = gy, x = gx;
    bool inside = true;
    if (g.n > 1) {
        k = gx / (g.W + 2);
        x = gx - k * (g.W + 2) - 2;
        y = gy - 2;
        inside = k < g.n && x >= 0 && y >= 0 && y < g.H;
    }
    unsigned char out[3] = {0, 0, 0};                                              // pad_value 0
    if (inside) {
        float v[3];
        fetch(g, k, y, x, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = v[c];
            if (g.normalize) t = (t - s_lo) / s_d;                                 // IEEE division, no reciprocal
            // add_image: truncation.  t is in [0, 1] by construction; the clamp only keeps a value outside it (a NaN becomes 0)
            // from an undefined conversion
            out[c] = (unsigned char)(int)fminf(fmaxf(t * 255.f, 0.f), 255.f);
        }
    }
    unsigned char* d = g.dst + (long long)p * 3;
    d[0] = out[0]; d[1] = out[1]; d[2] = out[2];
}

bool grid_ok(const rd_tb_grid_t& g) {
    if (!g.src || !g.dst || g.H <= 0 || g.W <= 0 || g.H > 4096 || g.W > 4096 || g.n < 1 || g.n > 3) return false;
    for (int k = 0; k < g.n; ++k)
        if (g.sample[k] < 0) return false;
    if (g.c0 < 0) return false;
    switch (g.transform) {
    case RD_TB_IDENTITY: case RD_TB_SIGMOID: case RD_TB_TANH:
        return (g.etype == RD_TB_F32 || g.etype == RD_TB_BF16) && (g.nc == 1 || g.nc == 3);
    case RD_TB_ARGMAX:
        return (g.etype == RD_TB_F32 || g.etype == RD_TB_BF16) && g.nc >= 1 && g.nc <= RD_TB_PALETTE && !g.normalize;
    case RD_TB_LABEL:
        return g.etype == RD_TB_I64 && !g.normalize;
    }
    return false;
}

// whole-slot loads: channel-contiguous pixels of exactly 16 bytes, the selection inside the slot, everything 16-byte aligned
int slot_ok(const rd_tb_grid_t& g) {
    if (g.transform == RD_TB_ARGMAX || g.transform == RD_TB_LABEL) return 0;
    const int n = g.etype == RD_TB_BF16 ? 8 : 4;
    return g.stride_c == 1 && g.stride_w == n && g.c0 + g.nc <= n && g.stride_h % n == 0 && g.stride_n % n == 0 &&
           (uintptr_t)g.src % 16 == 0;
}

}  // namespace

extern "C" int64_t rd_tb_grids_workspace(int n_grids) { return (int64_t)(n_grids > 0 ? n_grids : 0) * RD_TB_PARTS * sizeof(float2); }

extern "C" int rd_tb_grids(const rd_tb_grid_t* grids_host, int n_grids, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!grids_host || n_grids < 1 || n_grids > RD_TB_MAX_GRIDS || !workspace || (uintptr_t)workspace % 8 != 0 ||
        workspace_bytes < rd_tb_grids_workspace(n_grids))
        return -1;
    GridArgs a;
    a.n = n_grids;
    bool any_norm = false;
    long long max_px = 0;
    for (int i = 0; i < n_grids; ++i) {
        a.g[i] = grids_host[i];
        rd_tb_grid_t& g = a.g[i];
        if (!grid_ok(g)) return -1;
        g.slot = slot_ok(g);
        any_norm = any_norm || g.normalize;
        const long long px = g.n == 1 ? (long long)g.H * g.W : (long long)(g.H + 4) * (g.n * (g.W + 2) + 2);
        max_px = px > max_px ? px : max_px;
    }
    for (int i = n_grids; i < RD_TB_MAX_GRIDS; ++i) a.g[i] = a.g[0];
    hipStream_t st = (hipStream_t)stream;
    if (any_norm) rd_launch(tb_minmax_kernel, dim3(RD_TB_PARTS, n_grids), dim3(TB_THREADS), 0, st, a, (float2*)workspace);
    rd_launch(tb_compose_kernel, dim3((unsigned)((max_px + TB_THREADS - 1) / TB_THREADS), n_grids), dim3(TB_THREADS), 0, st, a,
              (const float2*)workspace);
    return (int)hipGetLastError();
}
