// augment.hip -- the per-sample pixel work of the training loaders on GPU-resident data (train.py --gpu_data): Pillow's 8-bit
// bilinear / nearest resampling, RandomScaleCrop's crop and the Fundus mask thresholds (code/dataset/transform.py:163-204,
// fundus.py:197-240), and the Prostate gathers (prostate.py:167-188), one launch per step.  Integer and byte arithmetic only:
// the result is bit-identical to PIL's (include/ramdsir.h rd_fundus_batch).
#include "common.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPrecision = 22;                              // Pillow Resample.c PRECISION_BITS (8 bpc)

struct FundusChunk { rd_fundus_sample_t s[RD_AUG_CHUNK]; };
struct ProstateChunk { rd_prostate_sample_t s[RD_AUG_CHUNK]; };

// one axis table: [n_in, n_out, ksize, 0] xmin[n_out] cnt[n_out] k[n_out][ksize] nearest[n_out]
struct Axis {
    const int32_t* xmin;
    const int32_t* cnt;
    const int32_t* k;
    const int32_t* nearest;
    int ksize;
    __device__ explicit Axis(const int32_t* t) {
        const int n_out = t[1];
        ksize = t[2];
        xmin = t + 4;
        cnt = xmin + n_out;
        k = cnt + n_out;
        nearest = k + n_out * ksize;
    }
};

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> kPrecision;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// output `o` of a pass over 3-channel pixels at `base + i * stride` (i = input position), Pillow's accumulation order
__device__ __forceinline__ void tap3(const uint8_t* base, int stride, const Axis& a, int o, uint8_t* out) {
    const int x0 = a.xmin[o], n = a.cnt[o];
    const int32_t* kk = a.k + o * a.ksize;
    int s0 = 1 << (kPrecision - 1), s1 = s0, s2 = s0;
    const uint8_t* q = base + x0 * stride;
    for (int t = 0; t < n; ++t, q += stride) {
        const int w = kk[t];
        s0 += (int)q[0] * w;
        s1 += (int)q[1] * w;
        s2 += (int)q[2] * w;
    }
    out[0] = clip8(s0);
    out[1] = clip8(s1);
    out[2] = clip8(s2);
}

// grid (bands, samples of the chunk, 2): z = 0 the sample's image (+ its mask and lam), z = 1 its partner.  Stages of one band of
// output rows [r0, r1): source rows [a0, e0) -> (horizontal W0 -> S) LDS A -> stage-1 rows [a1, e1) (vertical H0 -> S) LDS B ->
// (horizontal S -> sw, crop columns only) LDS C -> output rows (vertical S -> sh at rows cy + r).
__global__ __launch_bounds__(kThreads) void fundus_batch_kernel(rd_fundus_batch_t p, FundusChunk c, int b0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int S = p.S, band = blockIdx.x, which = blockIdx.z, tid = threadIdx.x;
    const rd_fundus_sample_t& s = c.s[blockIdx.y];
    const int b = b0 + blockIdx.y;
    const int r0 = band * p.band_rows, r1 = min(r0 + p.band_rows, S);
    if (r0 >= S) return;
    const rd_aug_image_t im = p.images[which ? s.partner : s.img];
    const Axis x1(p.tables + im.tab_x), y1(p.tables + im.tab_y);
    const Axis x2(p.tables + (which ? p.id_x : s.tab_x)), y2(p.tables + (which ? p.id_y : s.tab_y));
    const int cx = which ? 0 : s.cx, cy = which ? 0 : s.cy;

    const int a1 = y2.xmin[cy + r0], e1 = y2.xmin[cy + r1 - 1] + y2.cnt[cy + r1 - 1];     // stage-1 rows this band reads
    const int a0 = y1.xmin[a1], e0 = y1.xmin[e1 - 1] + y1.cnt[e1 - 1];                   // source rows those read
    const int n1 = e1 - a1, n0 = e0 - a0;
    if (n0 > p.src_rows || n1 > p.mid_rows) return;                                       // the caller's bounds exclude this
    uint8_t* A = lds;
    uint8_t* B = A + (size_t)p.src_rows * S * 3;
    uint8_t* C = B + (size_t)p.mid_rows * S * 3;
    const uint8_t* img = p.pixels + im.off;
    const int W0 = im.w;

    for (int i = tid; i < n0 * S; i += kThreads) {                                        // horizontal W0 -> S
        const int r = i / S, o = i - r * S;
        tap3(img + (size_t)(a0 + r) * W0 * 3, 3, x1, o, A + i * 3);
    }
    __syncthreads();
    for (int i = tid; i < n1 * S; i += kThreads) {                                        // vertical H0 -> S
        const int r = i / S, o = i - r * S;
        tap3(A - (size_t)a0 * S * 3 + o * 3, S * 3, y1, a1 + r, B + i * 3);
    }
    __syncthreads();
    for (int i = tid; i < n1 * S; i += kThreads) {                                        // horizontal S -> sw, crop columns
        const int r = i / S, j = i - r * S;
        tap3(B + (size_t)r * S * 3, 3, x2, cx + j, C + i * 3);
    }
    __syncthreads();
    uint8_t* out = (which ? p.trg : p.src) + (size_t)b * S * S * 3;
    for (int i = tid; i < (r1 - r0) * S; i += kThreads) {                                 // vertical S -> sh, crop rows
        const int r = r0 + i / S, j = i - (i / S) * S;
        tap3(C - (size_t)a1 * S * 3 + j * 3, S * 3, y2, cy + r, out + ((size_t)r * S + j) * 3);
    }
    if (which || im.mask_off < 0) return;
    // the mask: nearest through both stages (composed index tables), then fundus_mask's thresholds
    const uint8_t* g = p.masks + im.mask_off;
    float* m0 = p.mask + (size_t)b * 2 * S * S;
    float* m1 = m0 + (size_t)S * S;
    for (int i = tid; i < (r1 - r0) * S; i += kThreads) {
        const int r = r0 + i / S, j = i - (i / S) * S;
        const int sy = y1.nearest[y2.nearest[cy + r]], sx = x1.nearest[x2.nearest[cx + j]];
        const int v = g[(size_t)sy * W0 + sx];
        m0[(size_t)r * S + j] = v <= 50 ? 1.f : 0.f;
        m1[(size_t)r * S + j] = v <= 200 ? 1.f : 0.f;
    }
    if (band == 0 && tid == 0) p.lam[b] = s.lam;
}

// grid (blocks, samples of the chunk, 3): z = 0 image slice, 1 partner slice, 2 mask (+ lam)
__global__ __launch_bounds__(kThreads) void prostate_batch_kernel(rd_prostate_batch_t p, ProstateChunk c, int b0) {
    const rd_prostate_sample_t& s = c.s[blockIdx.y];
    const int b = b0 + blockIdx.y, which = blockIdx.z;
    const size_t px = (size_t)p.S * p.S;
    const size_t step = (size_t)gridDim.x * kThreads;
    const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (which < 2) {
        const float* in = p.slices + (size_t)(which ? s.partner : s.img) * px * 3;
        float* out = (which ? p.trg : p.src) + (size_t)b * px * 3;
        for (size_t i = first; i < px * 3; i += step) out[i] = in[i];
    } else {
        const uint8_t* in = p.masks + (size_t)s.img * px;
        int64_t* out = p.mask + (size_t)b * px;
        for (size_t i = first; i < px; i += step) out[i] = (int64_t)in[i];
        if (first == 0) p.lam[b] = s.lam;
    }
}

}  // namespace

extern "C" int rd_fundus_batch(const rd_fundus_batch_t* p, const rd_fundus_sample_t* samples_host, int B, void* stream) {
    if (!p || !samples_host || B < 0 || p->S < 1 || p->band_rows < 1 || p->src_rows < 1 || p->mid_rows < 1 || !p->pixels || !p->masks ||
        !p->images || !p->tables || !p->src || !p->trg || !p->lam || !p->mask)
        return -1;
    for (int b = 0; b < B; ++b) {
        const rd_fundus_sample_t& s = samples_host[b];
        if (s.img < 0 || s.img >= p->n_images || s.partner < 0 || s.partner >= p->n_images || s.sw < p->S || s.sh < p->S ||
            s.cx < 0 || s.cy < 0 || s.cx > s.sw - p->S || s.cy > s.sh - p->S || s.tab_x < 0 || s.tab_y < 0)
            return -1;
    }
    const size_t lds = (size_t)(p->src_rows + 2 * p->mid_rows) * p->S * 3;
    if (lds > 160 * 1024) return -1;
    if (lds > 64 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&fundus_batch_kernel),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (attr != hipSuccess) return (int)attr;
    }
    hipStream_t st = (hipStream_t)stream;
    const int bands = (p->S + p->band_rows - 1) / p->band_rows;
    for (int b0 = 0; b0 < B; b0 += RD_AUG_CHUNK) {
        const int n = B - b0 < RD_AUG_CHUNK ? B - b0 : RD_AUG_CHUNK;
        FundusChunk c{};
        for (int i = 0; i < n; ++i) c.s[i] = samples_host[b0 + i];
        rd_launch(fundus_batch_kernel, dim3(bands, n, 2), dim3(kThreads), lds, st, *p, c, b0);
    }
    return (int)hipGetLastError();
}

extern "C" int rd_prostate_batch(const rd_prostate_batch_t* p, const rd_prostate_sample_t* samples_host, int B, void* stream) {
    if (!p || !samples_host || B < 0 || p->S < 1 || !p->slices || !p->masks || !p->src || !p->trg || !p->lam || !p->mask) return -1;
    for (int b = 0; b < B; ++b) {
        const rd_prostate_sample_t& s = samples_host[b];
        if (s.img < 0 || s.img >= p->n_slices || s.partner < 0 || s.partner >= p->n_slices) return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t px3 = (size_t)p->S * p->S * 3;
    const int blocks = (int)((px3 + 4 * kThreads - 1) / (4 * kThreads));               // four values per thread
    for (int b0 = 0; b0 < B; b0 += RD_AUG_CHUNK) {
        const int n = B - b0 < RD_AUG_CHUNK ? B - b0 : RD_AUG_CHUNK;
        ProstateChunk c{};
        for (int i = 0; i < n; ++i) c.s[i] = samples_host[b0 + i];
        rd_launch(prostate_batch_kernel, dim3(blocks, n, 3), dim3(kThreads), 0, st, *p, c, b0);
    }
    return (int)hipGetLastError();
}
