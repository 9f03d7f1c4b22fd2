// infer.hip -- what the fused validation forward (ramdsir/infer.py EvalForward, train.py --fused_val) needs around its launch list of
// rd_conv / rd_pool_fwd entries: the BatchNorm coefficients of ALL sites from the running statistics in one launch per pass, and the
// heads of the two in-training validations reading / writing the plan's NHWC storage-dtype tensors in place -- the 2.5-D Prostate
// batch written straight into the network input, the Fundus resize + threshold and the Prostate argmax read straight from the logits.
// No NCHW fp32 tensor exists between them.  Each kernel is the NHWC form of an existing one and must give its bits:
//   bn_eval_coeffs_kernel      the eval branch of bn_finalize_fwd_kernel (bn.hip), through the same rdfin::fwd_coef
//   val_threshold_nhwc_kernel  val_threshold_kernel (val_post.hip), the same expressions under the same contraction pragma
//   vol_stack_nhwc_kernel      vol_stack_kernel followed by nchw_to_nhwc_kernel (val_volume.hip, bn.hip)
//   vol_argmax_nhwc_kernel     vol_argmax_kernel (val_volume.hip)
// All are elementwise and memory-bound: grid-stride loops, one 4-byte (bf16) or 8-byte (fp32) load per logit pair, 16-byte stores of
// whole channel slots.  Host records travel as kernel arguments, RD_VAL_CHUNK per launch.
#include <mutex>
#include <vector>
#include "common.h"
#include "bn_fin.h"
#include "val_common.h"
#include "../../include/ramdsir.h"

namespace {

using rdval::VolFrames;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                            // per image / slot: the grid-stride loops take the rest
constexpr int kMaxSites = 4096;

unsigned blocks_for(int64_t n) {
    const int64_t b = (n + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// ---- BatchNorm coefficients of a frozen plan -----------------------------------------------------------------------------------------
// blockIdx.y = site; the arithmetic is bn_finalize_fwd_kernel's with p.training == 0 (mean = running_mean).
__global__ __launch_bounds__(kThreads) void bn_eval_coeffs_kernel(const rd_bn_eval_site_t* __restrict__ sites, float eps) {
    const rd_bn_eval_site_t s = sites[blockIdx.y];
    for (int c = blockIdx.x * kThreads + threadIdx.x; c < s.C; c += gridDim.x * kThreads) {
        const float gam = s.gamma[c], bet = s.beta[c], rm = s.running_mean[c], rv = s.running_var[c];
        rdfin::FwdStat r;
        r.mean = rm;
        r.invstd = 1.0f / sqrtf(rv + eps);
        r.unb = 0.f;
        float sc, sh;
        rdfin::fwd_coef(gam, bet, r, sc, sh);
        s.scale[c] = sc;
        s.shift[c] = sh;
    }
}

// The stream the table is read back on: created once per device, non-blocking (it orders against no other stream).
hipStream_t check_stream() {
    constexpr int kMaxDev = 64;
    static std::mutex mu;
    static hipStream_t streams[kMaxDev] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[dev] && hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess) streams[dev] = nullptr;
    return streams[dev];
}

// ---- channels 0 and 1 of one NHWC pixel, widened to fp32 -----------------------------------------------------------------------------
// PAIR: one load brings both (cstride even, base aligned to the pair); else two element loads.
template <typename T, bool PAIR> struct Pair;
template <> struct Pair<bf16_t, true> {
    static __device__ __forceinline__ void load(const bf16_t* p, float& c0, float& c1) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        c0 = __uint_as_float(u << 16);
        c1 = __uint_as_float(u & 0xffff0000u);
    }
};
template <> struct Pair<float, true> {
    static __device__ __forceinline__ void load(const float* p, float& c0, float& c1) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        c0 = v.x;
        c1 = v.y;
    }
};
template <typename T> struct Pair<T, false> {
    static __device__ __forceinline__ void load(const T* p, float& c0, float& c1) {
        c0 = to_f<T>(p[0]);
        c1 = to_f<T>(p[1]);
    }
};

template <typename T> bool pair_ok(const void* base, int cstride) { return cstride % 2 == 0 && rdval::aligned(base, 2 * sizeof(T)); }

// ---- Fundus: sigmoid + bilinear resize + threshold ----------------------------------------------------------------------------------
struct ValImages {
    rd_val_image_t im[RD_VAL_CHUNK];
};

// blockIdx.y = image of the chunk; one thread serves both planes of an output pixel (the four taps are loaded once).  Contraction is
// off as in val_threshold_kernel: the source coordinate and the three lerps round after every operation.
template <typename T, bool PAIR>
__global__ __launch_bounds__(kThreads) void val_threshold_nhwc_kernel(const T* __restrict__ logits, uint8_t* __restrict__ mask, ValImages c,
                                                                      int b0, int Sh, int Sw, int cs) {
#pragma clang fp contract(off)
    const rd_val_image_t im = c.im[blockIdx.y];
    const int H = im.h, W = im.w, n = im.h * im.w;
    const float sy = (float)Sh / (float)H, sx = (float)Sw / (float)W;
    const T* src = logits + (size_t)(b0 + (int)blockIdx.y) * Sh * Sw * cs;
    uint8_t* m0 = mask + im.off;
    uint8_t* m1 = m0 + n;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const int y = i / W, x = i - y * W;
        const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = min(y0 + 1, Sh - 1), x1 = min(x0 + 1, Sw - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        float a[2], b[2], d[2], e[2];
        Pair<T, PAIR>::load(src + ((size_t)y0 * Sw + x0) * cs, a[0], a[1]);
        Pair<T, PAIR>::load(src + ((size_t)y0 * Sw + x1) * cs, b[0], b[1]);
        Pair<T, PAIR>::load(src + ((size_t)y1 * Sw + x0) * cs, d[0], d[1]);
        Pair<T, PAIR>::load(src + ((size_t)y1 * Sw + x1) * cs, e[0], e[1]);
        uint8_t r[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float pa = rdval::sigmoid_f(a[s]), pb = rdval::sigmoid_f(b[s]);
            const float pd = rdval::sigmoid_f(d[s]), pe = rdval::sigmoid_f(e[s]);
            const float top = hx * pa + lx * pb, bot = hx * pd + lx * pe;
            const float v = hy * top + ly * bot;
            r[s] = v > 0.75f ? 1 : 0;
        }
        m0[i] = r[0];
        m1[i] = r[1];
    }
}

template <typename T>
void launch_threshold(const T* logits, uint8_t* mask, const ValImages& c, int n, int64_t px, int b0, int Sh, int Sw, int cs, hipStream_t st) {
    const dim3 grid(blocks_for(px), n), blk(kThreads);
    if (pair_ok<T>(logits, cs))
        rd_launch(val_threshold_nhwc_kernel<T, true>, grid, blk, 0, st, logits, mask, c, b0, Sh, Sw, cs);
    else
        rd_launch(val_threshold_nhwc_kernel<T, false>, grid, blk, 0, st, logits, mask, c, b0, Sh, Sw, cs);
}

// ---- Prostate: the 2.5-D batch into the network input --------------------------------------------------------------------------------
// blockIdx.y = slot of the chunk; per pixel three 4-byte loads (one per slice, each coalesced over the wave) and, SLOT (cstride is one
// 16-byte channel slot and `out` is 16-byte aligned): one 16-byte store of the padded channel vector; else element stores.
template <typename T, bool SLOT>
__global__ __launch_bounds__(kThreads) void vol_stack_nhwc_kernel(const float* __restrict__ vol, T* __restrict__ out, VolFrames f, int b0,
                                                                  int64_t hw, int cs) {
    const int jj = f.jj[blockIdx.y];
    T* dst = out + (int64_t)(b0 + (int)blockIdx.y) * hw * cs;
    const float* s = vol + (int64_t)(jj < 1 ? 0 : jj - 1) * hw;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (int64_t)gridDim.x * kThreads) {
        float v[Slot<T>::N] = {};
        if (jj >= 0) {
            v[0] = s[i];
            v[1] = s[hw + i];
            v[2] = s[2 * hw + i];
        }
        if (SLOT) {
            reinterpret_cast<uint4*>(dst)[i] = Slot<T>::pack(v);
        } else {
            for (int ch = 0; ch < cs; ++ch) dst[i * cs + ch] = from_f<T>(ch < 3 ? v[ch] : 0.f);
        }
    }
}

template <typename T>
void launch_stack(const float* vol, T* out, const VolFrames& f, int nb, int b0, int64_t hw, int cs, hipStream_t st) {
    const dim3 grid(blocks_for(hw), nb), blk(kThreads);
    if (cs == Slot<T>::N && rdval::aligned(out, 16))
        rd_launch(vol_stack_nhwc_kernel<T, true>, grid, blk, 0, st, vol, out, f, b0, hw, cs);
    else
        rd_launch(vol_stack_nhwc_kernel<T, false>, grid, blk, 0, st, vol, out, f, b0, hw, cs);
}

// ---- Prostate: argmax over the two classes -------------------------------------------------------------------------------------------
// VEC: four voxels per lane and one 4-byte store (H * W a multiple of 4, pred 4-byte aligned); else one voxel per lane.
template <typename T, bool PAIR, bool VEC>
__global__ __launch_bounds__(kThreads) void vol_argmax_nhwc_kernel(const T* __restrict__ logits, uint8_t* __restrict__ pred,
                                                                   const uint8_t* __restrict__ gt_empty, VolFrames f, int b0, int64_t hw, int cs) {
    const int jj = f.jj[blockIdx.y];
    if (jj < 0) return;
    const T* src = logits + (int64_t)(b0 + (int)blockIdx.y) * hw * cs;
    uint8_t* dst = pred + (int64_t)jj * hw;
    const bool keep = gt_empty[jj] == 0;
    const int64_t n = VEC ? hw / 4 : hw;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (VEC) {
            uint32_t r = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float l0, l1;
                Pair<T, PAIR>::load(src + (4 * i + k) * cs, l0, l1);
                r |= l1 > l0 ? 1u << (8 * k) : 0u;
            }
            reinterpret_cast<uint32_t*>(dst)[i] = keep ? r : 0u;
        } else {
            float l0, l1;
            Pair<T, PAIR>::load(src + i * cs, l0, l1);
            dst[i] = (keep && l1 > l0) ? 1 : 0;
        }
    }
}

template <typename T>
void launch_argmax(const T* logits, uint8_t* pred, const uint8_t* gt_empty, const VolFrames& f, int nb, int b0, int64_t hw, int cs,
                   hipStream_t st) {
    const bool vec = hw % 4 == 0 && rdval::aligned(pred, 4), pair = pair_ok<T>(logits, cs);
    const dim3 grid(blocks_for(vec ? hw / 4 : hw), nb), blk(kThreads);
    if (pair && vec)
        rd_launch(vol_argmax_nhwc_kernel<T, true, true>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw, cs);
    else if (pair)
        rd_launch(vol_argmax_nhwc_kernel<T, true, false>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw, cs);
    else if (vec)
        rd_launch(vol_argmax_nhwc_kernel<T, false, true>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw, cs);
    else
        rd_launch(vol_argmax_nhwc_kernel<T, false, false>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw, cs);
}

bool valid_dtype(int dtype) { return dtype == RD_F32 || dtype == RD_BF16; }

}  // namespace

extern "C" int rd_bn_eval_coeffs(const rd_bn_eval_site_t* sites_dev, int n_sites, int max_C, float eps, void* stream) {
    if (!sites_dev || n_sites < 1 || n_sites > kMaxSites || max_C < 1) return -1;
    hipStream_t cs = check_stream();
    if (!cs) return -1;
    std::vector<rd_bn_eval_site_t> host((size_t)n_sites);
    RD_CHECK(hipMemcpyAsync(host.data(), sites_dev, sizeof(rd_bn_eval_site_t) * (size_t)n_sites, hipMemcpyDeviceToHost, cs));
    RD_CHECK(hipStreamSynchronize(cs));
    for (const rd_bn_eval_site_t& s : host)
        if (!s.gamma || !s.beta || !s.running_mean || !s.running_var || !s.scale || !s.shift || s.C < 1 || s.C > max_C) return -1;
    rd_launch(bn_eval_coeffs_kernel, dim3(blocks_for(max_C), n_sites), dim3(kThreads), 0, (hipStream_t)stream, sites_dev, eps);
    return (int)hipGetLastError();
}

extern "C" int rd_val_threshold_nhwc(const void* logits, int dtype, int cstride, int B, int Sh, int Sw, const rd_val_image_t* images_host,
                                     uint8_t* mask, int64_t mask_bytes, void* stream) {
    if (!logits || !mask || !valid_dtype(dtype) || cstride < 2 || Sh < 1 || Sw < 1 || !rdval::valid_images(images_host, B)) return -1;
    for (int i = 0; i < B; ++i)
        if (images_host[i].off + 2 * (int64_t)images_host[i].h * images_host[i].w > mask_bytes) return -1;
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int n = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        ValImages c{};
        int64_t px = 0;
        for (int i = 0; i < n; ++i) {
            c.im[i] = images_host[b0 + i];
            const int64_t m = (int64_t)c.im[i].h * c.im[i].w;
            px = m > px ? m : px;
        }
        if (dtype == RD_BF16)
            launch_threshold((const bf16_t*)logits, mask, c, n, px, b0, Sh, Sw, cstride, st);
        else
            launch_threshold((const float*)logits, mask, c, n, px, b0, Sh, Sw, cstride, st);
    }
    return (int)hipGetLastError();
}

extern "C" int rd_vol_stack_nhwc(const float* volume, int D, int H, int W, const int32_t* frames_host, int B, void* out, int dtype, int cstride,
                                 void* stream) {
    if (!volume || !out || !valid_dtype(dtype) || cstride < 3 || D < 1 || H < 1 || W < 1 || (int64_t)D * H * W > rdval::kMaxVoxels ||
        !rdval::valid_frames(frames_host, B, D))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int nb = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        const VolFrames f = rdval::frames_chunk(frames_host, b0, nb);
        if (dtype == RD_BF16)
            launch_stack(volume, (bf16_t*)out, f, nb, b0, hw, cstride, st);
        else
            launch_stack(volume, (float*)out, f, nb, b0, hw, cstride, st);
    }
    return (int)hipGetLastError();
}

extern "C" int rd_vol_argmax_nhwc(const void* logits, int dtype, int cstride, int B, int H, int W, const int32_t* frames_host,
                                  const uint8_t* gt_empty, int D, uint8_t* pred, void* stream) {
    if (!logits || !gt_empty || !pred || !valid_dtype(dtype) || cstride < 2 || D < 1 || H < 1 || W < 1 ||
        (int64_t)D * H * W > rdval::kMaxVoxels || !rdval::valid_frames(frames_host, B, D))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int nb = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        const VolFrames f = rdval::frames_chunk(frames_host, b0, nb);
        if (dtype == RD_BF16)
            launch_argmax((const bf16_t*)logits, pred, gt_empty, f, nb, b0, hw, cstride, st);
        else
            launch_argmax((const float*)logits, pred, gt_empty, f, nb, b0, hw, cstride, st);
    }
    return (int)hipGetLastError();
}
