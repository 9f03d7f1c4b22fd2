// val_volume.hip -- the in-training Prostate validation around the forward pass, on the GPU (train.py --gpu_val_volumes): the 2.5-D
// batches of three neighbouring slices (code/train.py:161-168), argmax over the two classes with the slices of empty ground truth
// suppressed (:170-176), the largest 6-connected 3-D component (code/utils/utils.py:30-42) and the three integer counts a Dice
// coefficient needs.  The model these kernels are read against is ramdsir/gpu_val_volumes.py (stack_model, argmax_model,
// largest_component_model).
//
// Labelling follows val_post.hip: a union-find over the voxels in (z, y, x) raster order, node i = voxel i.  A parent is never larger
// than its child (parent[n] <= n), so the root of a component is its first voxel in raster order -- which is scipy's component
// numbering, so "largest area, then smallest root" is argmax's first maximum.  Integer atomics only; no workgroup waits for another:
// every phase is a launch of its own.
#include "common.h"
#include "val_uf.h"
#include "val_common.h"
#include "../../include/ramdsir.h"

namespace {

using rdval::aligned;
using rdval::frames_chunk;
using rdval::kMaxVoxels;
using rdval::valid_frames;
using rdval::VolFrames;                                     // the frames of a chunk as they travel in the kernel arguments

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                               // elements per thread of the per-element kernels (strided by kThreads)

// ---- the 2.5-D batch ----------------------------------------------------------------------------------------------------------------
// Slot b of the batch is the 3 * H * W consecutive floats of the volume that start at slice jj - 1.  T = uint4 (16 B per lane) when H * W
// is a multiple of 4 and both buffers are 16-byte aligned, else float.  All loads of a thread are issued before its stores.
template <typename T>
__global__ __launch_bounds__(kThreads) void vol_stack_kernel(const float* __restrict__ vol, float* __restrict__ out, VolFrames f, int b0, int64_t hw) {
    const int jj = f.jj[blockIdx.y];
    constexpr int kPer = (int)(sizeof(T) / sizeof(float));
    const int64_t n = 3 * hw / kPer;
    T* dst = reinterpret_cast<T*>(out + (int64_t)(b0 + (int)blockIdx.y) * 3 * hw);
    const T* src = reinterpret_cast<const T*>(vol + (int64_t)(jj < 1 ? 0 : jj - 1) * hw);
    T v[kPerThread] = {};
    if (jj >= 0) {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int64_t i = ((int64_t)blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
            if (i < n) v[k] = src[i];
        }
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i < n) dst[i] = v[k];
    }
}

// ---- argmax -------------------------------------------------------------------------------------------------------------------------
// pred[jj] = l1 > l0 (the first maximum wins, as torch.max over the class axis), or zeros for a slice whose ground truth is empty.
// VEC: four voxels per lane (two 16-byte loads, one 4-byte store); H * W a multiple of 4 and aligned buffers.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void vol_argmax_kernel(const float* __restrict__ logits, uint8_t* __restrict__ pred,
                                                              const uint8_t* __restrict__ gt_empty, VolFrames f, int b0, int64_t hw) {
    const int jj = f.jj[blockIdx.y];
    if (jj < 0) return;
    const float* l0 = logits + (int64_t)(b0 + (int)blockIdx.y) * 2 * hw;
    const float* l1 = l0 + hw;
    uint8_t* dst = pred + (int64_t)jj * hw;
    const bool keep = gt_empty[jj] == 0;
    const int64_t n = VEC ? hw / 4 : hw;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t i = ((int64_t)blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= n) return;
        if (VEC) {
            const float4 a = reinterpret_cast<const float4*>(l0)[i], b = reinterpret_cast<const float4*>(l1)[i];
            const uint32_t r = (b.x > a.x ? 1u : 0u) | (b.y > a.y ? 1u << 8 : 0u) | (b.z > a.z ? 1u << 16 : 0u) | (b.w > a.w ? 1u << 24 : 0u);
            reinterpret_cast<uint32_t*>(dst)[i] = keep ? r : 0u;
        } else {
            dst[i] = (keep && l1[i] > l0[i]) ? 1 : 0;
        }
    }
}

// ---- largest component --------------------------------------------------------------------------------------------------------------
struct VolSet {
    rd_val_volume_t v[RD_VAL_CHUNK];
    int64_t node_off[RD_VAL_CHUNK];                         // first node of the volume in parent[] / count[]
    int32_t key_off;                                        // first key of the chunk (one per volume)
    int32_t pad_;
};

struct Vol {
    int H, W, hw, rows, n;                                  // rows = D * H, n = D * H * W
    int64_t pix;                                            // byte offset of the volume in pred / post
    int64_t gt;                                             // byte offset of the volume in gt
    int64_t node;                                           // first node of the volume
    int key;                                                // index of the volume's key
    int slot;                                               // first of the volume's three counts
};

__device__ __forceinline__ Vol vol_of(const VolSet& c, int p) {
    const rd_val_volume_t& v = c.v[p];
    Vol r;
    r.H = v.h;
    r.W = v.w;
    r.hw = v.h * v.w;
    r.rows = v.d * v.h;
    r.n = v.d * r.hw;
    r.pix = v.off;
    r.gt = v.gt_off;
    r.node = c.node_off[p];
    r.key = c.key_off + p;
    r.slot = v.slot * 3;
    return r;
}

// One workgroup per row (z, y).  Every set voxel's parent becomes the first voxel of its run along x (a running maximum over "a run
// starts here" positions, val_post.hip's scan); count[run start] = the run's length; the volume's key is reset.
__global__ __launch_bounds__(kThreads) void vol_rows_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, int* __restrict__ count,
                                                            unsigned long long* __restrict__ keys, VolSet c) {
    __shared__ int scan[kThreads];
    const Vol vl = vol_of(c, blockIdx.y);
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= vl.rows) return;
    const uint8_t* img = img_all + vl.pix + (size_t)row * vl.W;
    int* P = parent + vl.node + (size_t)row * vl.W;
    int* N = count + vl.node + (size_t)row * vl.W;
    const int base = row * vl.W;
    if (row == 0 && tid == 0) keys[vl.key] = 0ull;
    int carry = -1;
    for (int x0 = 0; x0 < vl.W; x0 += kThreads) {
        const int x = x0 + tid;
        const bool f = x < vl.W && img[x] != 0;
        const bool starts = f && (x == 0 || img[x - 1] == 0);
        scan[tid] = starts ? x : -1;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {            // inclusive running maximum
            const int v = tid >= d ? scan[tid - d] : -1;
            __syncthreads();
            scan[tid] = max(scan[tid], v);
            __syncthreads();
        }
        const int s = max(scan[tid], carry);
        const int next_carry = max(scan[kThreads - 1], carry);
        if (f) {
            P[x] = base + s;
            if (x == vl.W - 1 || img[x + 1] == 0) N[s] = x - s + 1;
        }
        carry = next_carry;
        __syncthreads();
    }
}

// Unions through faces only: with row y - 1 of the same slice and with row y of slice z - 1, and only where a run boundary makes one
// necessary -- when the voxel to the left and its neighbour in the other row are both set, that pair has already made the connection.
__global__ __launch_bounds__(kThreads) void vol_merge_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, VolSet c) {
    const Vol vl = vol_of(c, blockIdx.y);
    const uint8_t* img = img_all + vl.pix;
    int* P = parent + vl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= vl.n) return;
        if (!img[i]) continue;
        const int row = i / vl.W, x = i - row * vl.W;
        const int z = row / vl.H, y = row - z * vl.H;
        const bool w = x > 0 && img[i - 1];
        if (y > 0 && img[i - vl.W] && !(w && img[i - vl.W - 1])) unite(P, i, i - vl.W);
        if (z > 0 && img[i - vl.hw] && !(w && img[i - vl.hw - 1])) unite(P, i, i - vl.hw);
    }
}

// Every run start points at its root (all other voxels point at their run start: two hops to the root from now on).
__global__ __launch_bounds__(kThreads) void vol_flatten_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, VolSet c) {
    const Vol vl = vol_of(c, blockIdx.y);
    const uint8_t* img = img_all + vl.pix;
    int* P = parent + vl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= vl.n) return;
        if (!img[i] || (i % vl.W != 0 && img[i - 1])) continue;
        const int r = find_root(P, i);
        if (r != i) __hip_atomic_store(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// phase 0: the run lengths of a component are added up at its root; phase 1: the roots compete for the volume's key,
// (area << 32) | ~root: largest area first, then the smallest root.  A key of 0 afterwards: the prediction is empty.
__global__ __launch_bounds__(kThreads) void vol_area_kernel(const uint8_t* __restrict__ img_all, const int* parent, int* count,
                                                            unsigned long long* __restrict__ keys, VolSet c, int phase) {
    const Vol vl = vol_of(c, blockIdx.y);
    const uint8_t* img = img_all + vl.pix;
    const int* P = parent + vl.node;
    int* N = count + vl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= vl.n) return;
        if (!img[i] || (i % vl.W != 0 && img[i - 1])) continue;
        const int r = P[i];
        if (phase == 0) {
            if (r != i) atomicAdd(N + r, N[i]);
        } else if (r == i) {
            atomicMax(keys + vl.key, ((unsigned long long)(unsigned)N[r] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r));
        }
    }
}

// post = pred restricted to the winning component, or all ones for an empty prediction (the reference's `keep == 0`); then |post|, |gt|,
// |post & gt| of the volume: summed per wave, then per workgroup in LDS, one integer atomicAdd per workgroup and quantity.
__global__ __launch_bounds__(kThreads) void vol_select_kernel(const uint8_t* __restrict__ pred, uint8_t* __restrict__ post, const int* __restrict__ parent,
                                                              const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ gt,
                                                              int* __restrict__ counts, VolSet c) {
    const Vol vl = vol_of(c, blockIdx.y);
    const int* P = parent + vl.node;
    const unsigned long long key = keys[vl.key];
    const bool empty = key == 0ull;
    const int win = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    int np = 0, ng = 0, ni = 0;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= vl.n) break;
        const int v = empty ? 1 : ((pred[vl.pix + i] && P[P[i]] == win) ? 1 : 0);
        post[vl.pix + i] = (uint8_t)v;
        if (gt) {
            const int g = gt[vl.gt + i] != 0;
            np += v;
            ng += g;
            ni += v & g;
        }
    }
    if (!gt) return;
    for (int d = 32; d > 0; d >>= 1) {
        np += __shfl_down(np, d);
        ng += __shfl_down(ng, d);
        ni += __shfl_down(ni, d);
    }
    __shared__ int part[kThreads / 64][3];
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = np;
        part[threadIdx.x >> 6][1] = ng;
        part[threadIdx.x >> 6][2] = ni;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int v = 0;
        for (int w = 0; w < kThreads / 64; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(counts + vl.slot + threadIdx.x, v);
    }
}

bool valid_volumes(const rd_val_volume_t* v, int B) {
    if (!v || B < 0) return false;
    for (int i = 0; i < B; ++i)
        if (v[i].d < 1 || v[i].h < 1 || v[i].w < 1 || (int64_t)v[i].d * v[i].h * v[i].w > kMaxVoxels || v[i].off < 0) return false;
    return true;
}

int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

int64_t total_nodes(const rd_val_volume_t* v, int B) {
    int64_t n = 0;
    for (int i = 0; i < B; ++i) n += (int64_t)v[i].d * v[i].h * v[i].w;
    return n;
}

}  // namespace

extern "C" int rd_vol_stack(const float* volume, int D, int H, int W, const int32_t* frames_host, int B, float* out, void* stream) {
    if (!volume || !out || D < 1 || H < 1 || W < 1 || (int64_t)D * H * W > kMaxVoxels || !valid_frames(frames_host, B, D)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const bool vec = hw % 4 == 0 && aligned(volume, 16) && aligned(out, 16);
    const int64_t n = vec ? 3 * hw / 4 : 3 * hw;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int nb = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        const VolFrames f = frames_chunk(frames_host, b0, nb);
        const dim3 grid((unsigned)((n + kThreads * kPerThread - 1) / (kThreads * kPerThread)), nb), blk(kThreads);
        if (vec)
            rd_launch(vol_stack_kernel<uint4>, grid, blk, 0, st, volume, out, f, b0, hw);
        else
            rd_launch(vol_stack_kernel<float>, grid, blk, 0, st, volume, out, f, b0, hw);
    }
    return (int)hipGetLastError();
}

extern "C" int rd_vol_argmax(const float* logits, int B, int H, int W, const int32_t* frames_host, const uint8_t* gt_empty, int D, uint8_t* pred,
                             void* stream) {
    if (!logits || !gt_empty || !pred || D < 1 || H < 1 || W < 1 || (int64_t)D * H * W > kMaxVoxels || !valid_frames(frames_host, B, D)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const bool vec = hw % 4 == 0 && aligned(logits, 16) && aligned(pred, 4);
    const int64_t n = vec ? hw / 4 : hw;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int nb = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        const VolFrames f = frames_chunk(frames_host, b0, nb);
        const dim3 grid((unsigned)((n + kThreads * kPerThread - 1) / (kThreads * kPerThread)), nb), blk(kThreads);
        if (vec)
            rd_launch(vol_argmax_kernel<true>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw);
        else
            rd_launch(vol_argmax_kernel<false>, grid, blk, 0, st, logits, pred, gt_empty, f, b0, hw);
    }
    return (int)hipGetLastError();
}

extern "C" int64_t rd_vol_post_workspace(const rd_val_volume_t* volumes_host, int B) {
    if (!valid_volumes(volumes_host, B)) return -1;
    return align16((int64_t)B * 8) + 2 * align16(total_nodes(volumes_host, B) * 4);
}

extern "C" int rd_vol_post(const uint8_t* pred, uint8_t* post, int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, int32_t* counts, int n_slots,
                           void* workspace, int64_t workspace_bytes, const rd_val_volume_t* volumes_host, int B, void* stream) {
    if (!pred || !post || pred == post || !workspace || !valid_volumes(volumes_host, B) || (gt != nullptr) != (counts != nullptr)) return -1;
    if (workspace_bytes < rd_vol_post_workspace(volumes_host, B)) return -1;
    for (int i = 0; i < B; ++i) {
        const rd_val_volume_t& v = volumes_host[i];
        const int64_t bytes = (int64_t)v.d * v.h * v.w;
        if (v.off + bytes > pred_bytes) return -1;
        if (gt && (v.gt_off < 0 || v.gt_off + bytes > gt_bytes || v.slot < 0 || v.slot >= n_slots)) return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t nodes = total_nodes(volumes_host, B);
    unsigned long long* keys = (unsigned long long*)workspace;
    int* parent = (int*)((char*)workspace + align16((int64_t)B * 8));
    int* count = (int*)((char*)parent + align16(nodes * 4));
    int64_t node = 0;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int n = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        VolSet c{};
        int64_t vox = 0;
        int rows = 0;
        for (int i = 0; i < n; ++i) {
            c.v[i] = volumes_host[b0 + i];
            c.node_off[i] = node;
            const int64_t m = (int64_t)c.v[i].d * c.v[i].h * c.v[i].w;
            node += m;
            vox = m > vox ? m : vox;
            rows = c.v[i].d * c.v[i].h > rows ? c.v[i].d * c.v[i].h : rows;
        }
        c.key_off = b0;
        const dim3 gp((unsigned)((vox + kThreads * kPerThread - 1) / (kThreads * kPerThread)), n), gr(rows, n), blk(kThreads);
        rd_launch(vol_rows_kernel, gr, blk, 0, st, pred, parent, count, keys, c);
        rd_launch(vol_merge_kernel, gp, blk, 0, st, pred, parent, c);
        rd_launch(vol_flatten_kernel, gp, blk, 0, st, pred, parent, c);
        rd_launch(vol_area_kernel, gp, blk, 0, st, pred, (const int*)parent, count, keys, c, 0);
        rd_launch(vol_area_kernel, gp, blk, 0, st, pred, (const int*)parent, count, keys, c, 1);
        rd_launch(vol_select_kernel, gp, blk, 0, st, pred, post, (const int*)parent, (const unsigned long long*)keys, gt, counts, c);
    }
    return (int)hipGetLastError();
}
