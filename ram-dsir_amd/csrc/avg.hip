// avg.hip -- rd_avg_step: one pass over n pairs of device ranges that keeps a second copy of the model as an average along the
// training trajectory (train.py --avg_weights, ramdsir/avg.py): an exponential moving average, or the uniform average of every iterate
// from a start iteration on (SWAD's dense averaging).  No reference counterpart: the reference keeps the last iterate only.
//
// ONE launch.  The work decomposition is rd_snapshot's (csrc/snapshot.hip), restated: range i is cut into chunks of RD_AVG_CHUNK bytes
// from its start (the last one ragged, a chunk never straddles two ranges), chunk0 is the number of chunks of the ranges in front of
// it, the grid is flat over the chunks of all ranges, and a workgroup finds its range by binary search over the chunk0 column of the
// device table.  Within a chunk the part where src and dst are both 16-byte aligned moves with 16-byte loads and stores -- every load
// of a thread (AVG_QUADS of the source and as many of the average) issued before its first store; the words in front of and behind
// it, or the whole chunk when the two sides are aligned differently, with 4-byte accesses.
//
// The step count s is READ from the device (rd_adam_step leaves "number of completed steps" there, csrc/loss.hip), so every launch
// argument is the same at every step.  With k = s - 1 - start:
//     kind 1, or kind 0 with k <= 0:   dst = src            (the bits, whatever they are)
//     kind 0 with k > 0:               d = p - a;  t = w d;  a = a + t      w = one_minus_decay (mode 0) or 1 / (k + 1) (mode 1)
// three separately rounded fp32 operations, never an fma: the library is built with -ffp-contract=on, which fuses a * b + c written
// as ONE expression, so the three steps go through the _rn intrinsics.  ramdsir/avg.py model() is the same arithmetic in numpy.
//
// A chunk of 16 KiB, unlike the snapshot's 64 KiB: nothing here is reduced across the workgroup (no atomics whose count the chunk size
// would set), and the parameter arena of the network (a few million words) then gives a few workgroups to every compute unit.
#include "common.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int AVG_THREADS = 256;
constexpr int AVG_WORDS = RD_AVG_CHUNK / 4;                         // 32-bit words of a chunk
constexpr int AVG_QUADS = RD_AVG_CHUNK / 16 / AVG_THREADS;          // 16-byte accesses per thread and side: one batch is the chunk
static_assert(RD_AVG_CHUNK % (AVG_THREADS * 16) == 0 && AVG_QUADS >= 1 && AVG_QUADS <= 8, "a chunk is one batch of whole quads");
static_assert(sizeof(rd_avg_range_t) == 40, "rd_avg_range_t is five 8-byte words");

// the ranges are device allocations: global, not generic, loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

// one word of the average: p the live word, a the averaged one
__device__ __forceinline__ unsigned avg_word(unsigned p, unsigned a, float w) {
    const float fa = __uint_as_float(a);
    const float d = __fsub_rn(__uint_as_float(p), fa);
    const float t = __fmul_rn(w, d);
    return __float_as_uint(__fadd_rn(fa, t));
}

__global__ __launch_bounds__(AVG_THREADS) void avg_step_kernel(const rd_avg_range_t* __restrict__ table, int n,
                                                               const int* __restrict__ iter, int mode, float one_minus_decay, int start) {
    const long long c = blockIdx.x;
    const int t = threadIdx.x;
    // the last range whose first chunk is <= c: an empty range shares its first chunk with the range behind it and is never chosen
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    const rd_avg_range_t r = table[lo];
    const long long w0 = (c - r.chunk0) * AVG_WORDS;                // first word of this chunk within its range
    const long long rest = (r.bytes >> 2) - w0;
    if (c < r.chunk0 || rest <= 0) return;                          // a table that does not match the grid: touch nothing
    const int len = rest < AVG_WORDS ? (int)rest : AVG_WORDS;
    const long long k = (long long)*iter - 1 - start;
    const bool copy = r.kind != 0 || k <= 0;                        // uniform over the workgroup
    const float w = mode == 0 ? one_minus_decay : __fdiv_rn(1.0f, (float)(copy ? 1 : k + 1));
    const g_u32* __restrict__ src = (const g_u32*)((const unsigned*)r.src + w0);
    g_u32* dst = (g_u32*)((unsigned*)r.dst + w0);
    // [0, head) word by word up to the first 16-byte boundary, then nq whole quads, then [tail, len) word by word; sides that are
    // aligned differently have no common boundary: head = len
    int head = (int)((0 - ((uintptr_t)src >> 2)) & 3);
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0) head = len;
    head = head < len ? head : len;
    const int nq = (len - head) >> 2, tail = head + 4 * nq;
    const g_u32x4* __restrict__ s4 = (const g_u32x4*)(src + head);
    g_u32x4* d4 = (g_u32x4*)(dst + head);
    u32x4 p[AVG_QUADS], a[AVG_QUADS];
#pragma unroll
    for (int j = 0; j < AVG_QUADS; ++j) {
        const int q = t + j * AVG_THREADS;
        if (q < nq) p[j] = s4[q];
    }
    if (copy) {
#pragma unroll
        for (int j = 0; j < AVG_QUADS; ++j) {
            const int q = t + j * AVG_THREADS;
            if (q < nq) d4[q] = p[j];
        }
        for (int i = t; i < head; i += AVG_THREADS) dst[i] = src[i];
        for (int i = tail + t; i < len; i += AVG_THREADS) dst[i] = src[i];
        return;
    }
#pragma unroll
    for (int j = 0; j < AVG_QUADS; ++j) {
        const int q = t + j * AVG_THREADS;
        if (q < nq) a[j] = d4[q];
    }
#pragma unroll
    for (int j = 0; j < AVG_QUADS; ++j) {
        const int q = t + j * AVG_THREADS;
        if (q < nq)
            d4[q] = u32x4{avg_word(p[j].x, a[j].x, w), avg_word(p[j].y, a[j].y, w), avg_word(p[j].z, a[j].z, w), avg_word(p[j].w, a[j].w, w)};
    }
    for (int i = t; i < head; i += AVG_THREADS) dst[i] = avg_word(src[i], dst[i], w);
    for (int i = tail + t; i < len; i += AVG_THREADS) dst[i] = avg_word(src[i], dst[i], w);
}

}  // namespace

extern "C" int rd_avg_step(const rd_avg_range_t* table_host, const rd_avg_range_t* table_dev, int n, int64_t total_chunks,
                           const int32_t* iter_dev, int mode, float one_minus_decay, int32_t start, void* stream) {
    if (n < 0 || n > (1 << 24) || !iter_dev) return -1;
    if (mode != 0 && mode != 1) return -6;
    if (mode == 0 && !(one_minus_decay > 0.0f && one_minus_decay < 1.0f)) return -7;      // NaN fails both comparisons
    if (start < 0) return -8;
    if (n == 0) return 0;
    if (!table_host || !table_dev) return -1;
    if ((uintptr_t)iter_dev % 4 != 0) return -3;
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        const rd_avg_range_t& r = table_host[i];
        if (r.bytes < 0 || r.bytes % 4 != 0) return -2;
        if ((uintptr_t)r.src % 4 != 0 || (uintptr_t)r.dst % 4 != 0 || (r.bytes > 0 && (!r.src || !r.dst))) return -3;
        if (r.kind != 0 && r.kind != 1) return -4;
        if (r.chunk0 != chunks) return -5;
        chunks += (r.bytes + RD_AVG_CHUNK - 1) / RD_AVG_CHUNK;
        if (chunks > 0x7fffffffll) return -5;
    }
    if (chunks != total_chunks) return -5;
    if (chunks == 0) return 0;                                      // every range is empty: nothing to launch
    rd_launch(avg_step_kernel, dim3((unsigned)chunks), dim3(AVG_THREADS), 0, (hipStream_t)stream, table_dev, n, (const int*)iter_dev, mode,
              one_minus_decay, (int)start);
    return (int)hipGetLastError();
}
