// val_post.hip -- the in-training Fundus validation after the forward pass, on the GPU (train.py --gpu_val): sigmoid + bilinear resize to
// the native mask size + the 0.75 threshold (code/train.py:91-132), largest 8-connected component + hole filling per structure
// (code/utils/utils.py:19-28,45-96) and the three integer counts a Dice coefficient needs.  The model these kernels are read against is
// ramdsir/gpu_val.py (resize_threshold_model, postprocess_model).
//
// Labelling is a union-find over "nodes": node 0 of a plane is the virtual image border (background pass only), node i + 1 is pixel i in
// raster order.  A parent is never larger than its child (parent[n] <= n), so a find from node n takes at most n steps and the root of a
// component is its first pixel in raster order -- which is scipy's component numbering, so "largest area, then smallest root" is
// argmax's first maximum.  Integer atomics only; no workgroup waits for another: every phase is a launch of its own.
#include "common.h"
#include "val_uf.h"
#include "val_common.h"
#include "../../include/ramdsir.h"

namespace {

using rdval::kMaxPixels;
using rdval::sigmoid_f;
using rdval::valid_images;

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                               // pixels per thread of the per-pixel kernels (strided by kThreads)

struct ValPlaneSet {
    rd_val_image_t im[RD_VAL_CHUNK];
    int64_t node_off[RD_VAL_CHUNK];                         // first node of the image's plane 0 in parent[] / count[]; plane 1 follows
    int32_t key_off;                                        // first key of the chunk (two per image)
    int32_t pad_;
};

struct Plane {
    int H, W, n;
    int64_t pix;                                            // byte offset of the plane in mask / post
    int64_t gt;                                             // byte offset of the plane in gt
    int64_t node;                                           // first node of the plane
    int key;                                                // index of the plane's key
    int slot;                                               // first of the plane's three counts
};

__device__ __forceinline__ Plane plane_of(const ValPlaneSet& c, int p) {
    const rd_val_image_t& im = c.im[p >> 1];
    const int s = p & 1;
    Plane r;
    r.H = im.h;
    r.W = im.w;
    r.n = im.h * im.w;
    r.pix = im.off + (int64_t)s * r.n;
    r.gt = im.gt_off + (int64_t)s * r.n;
    r.node = c.node_off[p >> 1] + (int64_t)s * (r.n + 1);
    r.key = c.key_off + p;
    r.slot = (im.slot * 2 + s) * 3;
    return r;
}

// ---- stage a ------------------------------------------------------------------------------------------------------------------------
// F.interpolate(sigmoid(logits), (H, W), mode='bilinear', align_corners=False) > 0.75, one thread per output pixel; the probability
// map at native size is never stored.  Contraction is off in here: the source coordinate and the three lerps round after every
// operation, as resize_threshold_model's float32 numpy does.  (sigmoid_f: val_common.h, shared with the NHWC form in infer.hip.)
__global__ __launch_bounds__(kThreads) void val_threshold_kernel(const float* __restrict__ logits, uint8_t* __restrict__ mask, ValPlaneSet c,
                                                                 int b0, int Sh, int Sw) {
#pragma clang fp contract(off)
    const Plane pl = plane_of(c, blockIdx.y);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= pl.n) return;
    const int y = i / pl.W, x = i - y * pl.W;
    const float sy = (float)Sh / (float)pl.H, sx = (float)Sw / (float)pl.W;
    const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = min(y0 + 1, Sh - 1), x1 = min(x0 + 1, Sw - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* src = logits + ((size_t)(b0 + (blockIdx.y >> 1)) * 2 + (blockIdx.y & 1)) * Sh * Sw;
    const float a = sigmoid_f(src[(size_t)y0 * Sw + x0]), b = sigmoid_f(src[(size_t)y0 * Sw + x1]);
    const float d = sigmoid_f(src[(size_t)y1 * Sw + x0]), e = sigmoid_f(src[(size_t)y1 * Sw + x1]);
    const float top = hx * a + lx * b, bot = hx * d + lx * e;
    const float v = hy * top + ly * bot;
    mask[pl.pix + i] = v > 0.75f ? 1 : 0;
}

// ---- stage b: union-find (find_root, unite: val_uf.h) -------------------------------------------------------------------------------
// BG = false: the foreground of `img` (8-connectivity); BG = true: its background (4-connectivity + the border node)
template <bool BG>
__device__ __forceinline__ bool member(const uint8_t* img, int i) { return (img[i] != 0) != BG; }

// One workgroup per row.  Every member pixel's parent becomes the first pixel of its horizontal run (a running maximum over "a run starts
// here" positions); count[run start] = the run's length; the plane's key and border node are reset.
template <bool BG>
__global__ __launch_bounds__(kThreads) void val_rows_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, int* __restrict__ count,
                                                            unsigned long long* __restrict__ keys, ValPlaneSet c) {
    __shared__ int scan[kThreads];
    const Plane pl = plane_of(c, blockIdx.y);
    const int y = blockIdx.x, tid = threadIdx.x;
    if (y >= pl.H) return;
    const uint8_t* img = img_all + pl.pix + (size_t)y * pl.W;
    int* P = parent + pl.node;
    int* N = count + pl.node;
    if (y == 0 && tid == 0) {
        P[0] = 0;
        N[0] = 0;
        keys[pl.key] = 0ull;
    }
    int carry = -1;
    for (int x0 = 0; x0 < pl.W; x0 += kThreads) {
        const int x = x0 + tid;
        const bool f = x < pl.W && member<BG>(img, x);
        const bool starts = f && (x == 0 || !member<BG>(img, x - 1));
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
            const int node = y * pl.W + x + 1;
            P[node] = y * pl.W + s + 1;
            if (x == pl.W - 1 || !member<BG>(img, x + 1)) N[y * pl.W + s + 1] = x - s + 1;
        }
        carry = next_carry;
        __syncthreads();
    }
}

// Unions between rows, only where a run boundary makes one necessary: with both left neighbours present the pixel to the left has
// already made the same connection.  Background: border pixels join node 0.
template <bool BG>
__global__ __launch_bounds__(kThreads) void val_merge_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, ValPlaneSet c) {
    const Plane pl = plane_of(c, blockIdx.y);
    const uint8_t* img = img_all + pl.pix;
    int* P = parent + pl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= pl.n) return;
        if (!member<BG>(img, i)) continue;
        const int y = i / pl.W, x = i - y * pl.W;
        const bool w = x > 0 && member<BG>(img, i - 1);
        if (BG) {
            const bool edge_x = x == 0 || x == pl.W - 1, edge_y = y == 0 || y == pl.H - 1;
            if (edge_x || (edge_y && !w)) unite(P, i + 1, 0);
        }
        if (y == 0) continue;
        const int up = i - pl.W;
        const bool n = member<BG>(img, up);
        const bool nw = x > 0 && member<BG>(img, up - 1);
        if (n) {
            if (!(w && nw)) unite(P, i + 1, up + 1);
        } else if (!BG) {
            if (nw && !w) unite(P, i + 1, up);
            if (x < pl.W - 1 && member<BG>(img, up + 1)) unite(P, i + 1, up + 2);
        }
    }
}

// Every run start points at its root (all other members point at their run start: two hops to the root from now on).
template <bool BG>
__global__ __launch_bounds__(kThreads) void val_flatten_kernel(const uint8_t* __restrict__ img_all, int* __restrict__ parent, ValPlaneSet c) {
    const Plane pl = plane_of(c, blockIdx.y);
    const uint8_t* img = img_all + pl.pix;
    int* P = parent + pl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= pl.n) return;
        if (!member<BG>(img, i)) continue;
        if (i % pl.W != 0 && member<BG>(img, i - 1)) continue;
        const int r = find_root(P, i + 1);
        if (r != i + 1) __hip_atomic_store(P + i + 1, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// phase 0: the run lengths of a component are added up at its root; phase 1: the roots compete for the plane's key,
// (area << 32) | ~root: largest area first, then the smallest root.
__global__ __launch_bounds__(kThreads) void val_area_kernel(const uint8_t* __restrict__ img_all, const int* parent, int* count,
                                                            unsigned long long* __restrict__ keys, ValPlaneSet c, int phase) {
    const Plane pl = plane_of(c, blockIdx.y);
    const uint8_t* img = img_all + pl.pix;
    const int* P = parent + pl.node;
    int* N = count + pl.node;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= pl.n) return;
        if (!img[i] || (i % pl.W != 0 && img[i - 1])) continue;
        const int r = P[i + 1];
        if (phase == 0) {
            if (r != i + 1) atomicAdd(N + r, N[i + 1]);
        } else if (r == i + 1) {
            atomicMax(keys + pl.key, ((unsigned long long)(unsigned)N[r] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r));
        }
    }
}

// post = mask restricted to the winning component
__global__ __launch_bounds__(kThreads) void val_select_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ post, const int* __restrict__ parent,
                                                              const unsigned long long* __restrict__ keys, ValPlaneSet c) {
    const Plane pl = plane_of(c, blockIdx.y);
    const int* P = parent + pl.node;
    const unsigned long long key = keys[pl.key];
    const int win = key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : -1;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= pl.n) return;
        post[pl.pix + i] = (mask[pl.pix + i] && P[P[i + 1]] == win) ? 1 : 0;
    }
}

// Background that does not reach the border becomes foreground; stage c: |post|, |gt|, |post & gt| of the plane, one integer atomicAdd
// per workgroup and quantity.
__global__ __launch_bounds__(kThreads) void val_fill_kernel(uint8_t* __restrict__ post, const int* __restrict__ parent, const uint8_t* __restrict__ gt,
                                                            int* __restrict__ counts, ValPlaneSet c) {
    const Plane pl = plane_of(c, blockIdx.y);
    const int* P = parent + pl.node;
    int np = 0, ng = 0, ni = 0;
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (blockIdx.x * kPerThread + k) * kThreads + threadIdx.x;
        if (i >= pl.n) break;
        int v = post[pl.pix + i];
        if (!v) {
            v = P[P[i + 1]] != 0;
            if (v) post[pl.pix + i] = 1;
        }
        if (gt) {
            const int g = gt[pl.gt + i] != 0;
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
        if (v) atomicAdd(counts + pl.slot + threadIdx.x, v);
    }
}

int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

int64_t total_nodes(const rd_val_image_t* im, int B) {
    int64_t n = 0;
    for (int i = 0; i < B; ++i) n += 2 * ((int64_t)im[i].h * im[i].w + 1);
    return n;
}

}  // namespace

extern "C" int rd_val_threshold(const float* logits, int B, int Sh, int Sw, const rd_val_image_t* images_host, uint8_t* mask, int64_t mask_bytes,
                                void* stream) {
    if (!logits || !mask || Sh < 1 || Sw < 1 || !valid_images(images_host, B)) return -1;
    for (int i = 0; i < B; ++i)
        if (images_host[i].off + 2 * (int64_t)images_host[i].h * images_host[i].w > mask_bytes) return -1;
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int n = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        ValPlaneSet c{};
        int64_t px = 0;
        for (int i = 0; i < n; ++i) {
            c.im[i] = images_host[b0 + i];
            const int64_t m = (int64_t)c.im[i].h * c.im[i].w;
            px = m > px ? m : px;
        }
        rd_launch(val_threshold_kernel, dim3((unsigned)((px + kThreads - 1) / kThreads), 2 * n), dim3(kThreads), 0, st, logits, mask, c, b0, Sh, Sw);
    }
    return (int)hipGetLastError();
}

extern "C" int64_t rd_val_post_workspace(const rd_val_image_t* images_host, int B) {
    if (!valid_images(images_host, B)) return -1;
    return align16(2 * (int64_t)B * 8) + 2 * align16(total_nodes(images_host, B) * 4);
}

extern "C" int rd_val_post(const uint8_t* mask, uint8_t* post, int64_t mask_bytes, const uint8_t* gt, int64_t gt_bytes, int32_t* counts, int n_slots,
                           void* workspace, int64_t workspace_bytes, const rd_val_image_t* images_host, int B, void* stream) {
    if (!mask || !post || mask == post || !workspace || !valid_images(images_host, B) || (gt != nullptr) != (counts != nullptr)) return -1;
    if (workspace_bytes < rd_val_post_workspace(images_host, B)) return -1;
    for (int i = 0; i < B; ++i) {
        const rd_val_image_t& im = images_host[i];
        const int64_t bytes = 2 * (int64_t)im.h * im.w;
        if (im.off + bytes > mask_bytes) return -1;
        if (gt && (im.gt_off < 0 || im.gt_off + bytes > gt_bytes || im.slot < 0 || im.slot >= n_slots)) return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t nodes = total_nodes(images_host, B);
    unsigned long long* keys = (unsigned long long*)workspace;
    int* parent = (int*)((char*)workspace + align16(2 * (int64_t)B * 8));
    int* count = (int*)((char*)parent + align16(nodes * 4));
    int64_t node = 0;
    for (int b0 = 0; b0 < B; b0 += RD_VAL_CHUNK) {
        const int n = B - b0 < RD_VAL_CHUNK ? B - b0 : RD_VAL_CHUNK;
        ValPlaneSet c{};
        int64_t px = 0;
        int rows = 0;
        for (int i = 0; i < n; ++i) {
            c.im[i] = images_host[b0 + i];
            c.node_off[i] = node;
            const int64_t m = (int64_t)c.im[i].h * c.im[i].w;
            node += 2 * (m + 1);
            px = m > px ? m : px;
            rows = c.im[i].h > rows ? c.im[i].h : rows;
        }
        c.key_off = 2 * b0;
        const dim3 gp((unsigned)((px + kThreads * kPerThread - 1) / (kThreads * kPerThread)), 2 * n), gr(rows, 2 * n), blk(kThreads);
        // the foreground: label, measure, keep the winner
        rd_launch(val_rows_kernel<false>, gr, blk, 0, st, mask, parent, count, keys, c);
        rd_launch(val_merge_kernel<false>, gp, blk, 0, st, mask, parent, c);
        rd_launch(val_flatten_kernel<false>, gp, blk, 0, st, mask, parent, c);
        rd_launch(val_area_kernel, gp, blk, 0, st, mask, (const int*)parent, count, keys, c, 0);
        rd_launch(val_area_kernel, gp, blk, 0, st, mask, (const int*)parent, count, keys, c, 1);
        rd_launch(val_select_kernel, gp, blk, 0, st, mask, post, (const int*)parent, (const unsigned long long*)keys, c);
        // its background: label with the border node, fill what does not reach it, count
        rd_launch(val_rows_kernel<true>, gr, blk, 0, st, (const uint8_t*)post, parent, count, keys, c);
        rd_launch(val_merge_kernel<true>, gp, blk, 0, st, (const uint8_t*)post, parent, c);
        rd_launch(val_flatten_kernel<true>, gp, blk, 0, st, (const uint8_t*)post, parent, c);
        rd_launch(val_fill_kernel, gp, blk, 0, st, post, (const int*)parent, gt, counts, c);
    }
    return (int)hipGetLastError();
}
