// sumsq_pass.h -- the ONE text of the fixed-order sum of squares: the health pass of rd_step_log (step_log.hip) and the verdict of
// rd_grad_guard (guard.hip) use all of it; ramdsir/sumsq.py restates it in numpy, bit for bit.
//
// Two launches.  (1) One workgroup of THREADS per chunk of RD_LOG_CHUNK gradient elements: chunk() sums g * g in fp64 over the chunk's
// finite elements and counts the others (accumulate, common.h) -> one Partial per chunk.  Which element a chunk starts at is the
// caller's: step_log.hip counts chunks from the start of each Adam group, guard.hip from the start of the arena.  (2) One wave per
// group: fold() adds the group's partials.
//
// The order, fixed by the indices alone -- no atomics, the same bits on every run and for every caller.  A chunk is cut at its first
// 16-byte boundary into [0, head) words, nq whole quads and [tail, len) words.  Thread t adds, in this order: head word t; the four
// words x, y, z, w of quad t + k * THREADS for k = 0 .. QUADS - 1 (all QUADS 16-byte loads in flight together); tail word tail + t.
// An absent word is 0.f and adds 0.0.  Then the xor tree over the 64 lanes of each wave (wave_sum, common.h), then the waves in
// ascending order on thread 0.  In the fold lane l adds partials begin + l, begin + l + 64, ... in ascending order, then the xor tree.
#pragma once
#include "common.h"
#include "../../include/ramdsir.h"

namespace rdsum {

constexpr int THREADS = 256;
constexpr int QUADS = RD_LOG_CHUNK / 4 / THREADS;               // 16-byte loads per thread and chunk, all in flight together
constexpr int FOLD = 8;                                         // partials per lane and pass of the second launch
static_assert(RD_LOG_CHUNK == QUADS * 4 * THREADS, "a chunk is a whole number of 16-byte loads per thread");

struct Partial {
    double sum;                 // of the squares of the finite elements
    long long count;            // of the others
};

// a workgroup of THREADS over the chunk p[0, len), 0 <= len <= RD_LOG_CHUNK; the chunk's Partial on thread 0 (only there)
__device__ __forceinline__ Partial chunk(const float* __restrict__ p, int len) {
    const int t = threadIdx.x;
    // [0, head) scalar up to the first 16-byte boundary, then nq whole quads, then [tail, len) scalar: every index is inside the chunk
    int head = (int)((0 - ((uintptr_t)p >> 2)) & 3);
    head = head < len ? head : len;
    const int nq = (len - head) >> 2, tail = head + 4 * nq;
    const float4* __restrict__ q4 = (const float4*)(p + head);
    float4 v[QUADS];
#pragma unroll
    for (int k = 0; k < QUADS; ++k) {
        const int q = t + k * THREADS;
        v[k] = q < nq ? q4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float h = t < head ? p[t] : 0.f;
    const float e = tail + t < len ? p[tail + t] : 0.f;
    double s = 0.0;
    int bad = 0;
    accumulate(h, s, bad);
#pragma unroll
    for (int k = 0; k < QUADS; ++k) {
        accumulate(v[k].x, s, bad);
        accumulate(v[k].y, s, bad);
        accumulate(v[k].z, s, bad);
        accumulate(v[k].w, s, bad);
    }
    accumulate(e, s, bad);
    __shared__ double s_sum[THREADS / 64];
    __shared__ long long s_bad[THREADS / 64];
    s = wave_sum(s);
    const long long n = wave_sum((long long)bad);
    if ((t & 63) == 0) { s_sum[t >> 6] = s; s_bad[t >> 6] = n; }
    __syncthreads();
    Partial r = {0.0, 0};
    if (t == 0) {
        r = Partial{s_sum[0], s_bad[0]};
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) { r.sum += s_sum[w]; r.count += s_bad[w]; }
    }
    return r;
}

// one wave over partial[begin, end): every lane returns the folded pair.  FOLD loads per lane in flight (the real arena has
// 481 + 298 + 151 chunks: one pass per group); an absent slot adds 0.0, which leaves the sum as it is, so the order of the additions
// is the ascending one whatever FOLD is
__device__ __forceinline__ Partial fold(const Partial* __restrict__ partial, int begin, int end, int lane) {
    double s = 0.0;
    long long n = 0;
    for (int base = begin + lane; base < end; base += 64 * FOLD) {
        Partial r[FOLD];
#pragma unroll
        for (int k = 0; k < FOLD; ++k) {
            const int i = base + 64 * k;
            r[k] = i < end ? partial[i] : Partial{0.0, 0};
        }
#pragma unroll
        for (int k = 0; k < FOLD; ++k) {
            s += r[k].sum;
            n += r[k].count;
        }
    }
    return Partial{wave_sum(s), wave_sum(n)};
}

}  // namespace rdsum
