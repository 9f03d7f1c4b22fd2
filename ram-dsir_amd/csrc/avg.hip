// avg.hip -- rd_avg_step: one pass over n pairs of device ranges that keeps a second copy of the model as an average along the
// training trajectory (train.py --avg_weights, ramdsir/avg.py): an exponential moving average, or the uniform average of every iterate
// from a start iteration on (SWAD's dense averaging).  No reference counterpart: the reference keeps the last iterate only.
//
// ONE launch, in the walk of range_walk.h over chunks of RD_AVG_CHUNK bytes: lookup, alignment split, host-side table check, and
// its batched copy where a chunk is copied.  Every 16-byte load of a thread (AVG_QUADS of the source and as many of the average) is
// issued before its first store.
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
#include "range_walk.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int AVG_THREADS = 256;
constexpr int AVG_WORDS = RD_AVG_CHUNK / 4;                         // 32-bit words of a chunk
constexpr int AVG_QUADS = RD_AVG_CHUNK / 16 / AVG_THREADS;          // 16-byte accesses per thread and side: one batch is the chunk
static_assert(RD_AVG_CHUNK % (AVG_THREADS * 16) == 0 && AVG_QUADS >= 1 && AVG_QUADS <= 8, "a chunk is one batch of whole quads");
static_assert(sizeof(rd_avg_range_t) == 40, "rd_avg_range_t is five 8-byte words");

using namespace rdwalk;

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
    const rd_avg_range_t r = table[find_range(table, n, c)];
    long long w0;                                                   // first word of this chunk within its range
    const int len = chunk_len<AVG_WORDS>(c, r.chunk0, r.bytes >> 2, w0);
    if (len == 0) return;
    const long long k = (long long)*iter - 1 - start;
    const bool copy = r.kind != 0 || k <= 0;                        // uniform over the workgroup
    const float w = mode == 0 ? one_minus_decay : __fdiv_rn(1.0f, (float)(copy ? 1 : k + 1));
    const g_u32* __restrict__ src = (const g_u32*)((const unsigned*)r.src + w0);
    g_u32* dst = (g_u32*)((unsigned*)r.dst + w0);
    const Split<int> sp = split16(len, src, dst);
    const int head = sp.head, nq = sp.nq, tail = sp.tail;
    g_u32x4* d4 = (g_u32x4*)(dst + head);
    u32x4 p[AVG_QUADS], a[AVG_QUADS];
    load_quads<AVG_QUADS, AVG_THREADS>((const g_u32x4*)(src + head), nq, p);
    if (copy) {                                                     // copy_chunk, its loads shared with the other branch
        store_chunk<AVG_QUADS, AVG_THREADS>(src, dst, len, sp, p);
        return;
    }
    load_quads<AVG_QUADS, AVG_THREADS>((const g_u32x4*)d4, nq, a);
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
    const int64_t chunks = walk_table<RD_AVG_CHUNK>(table_host, n, total_chunks, [](const rd_avg_range_t& r) -> int64_t {
        if (r.bytes < 0 || r.bytes % 4 != 0) return -2;
        if ((uintptr_t)r.src % 4 != 0 || (uintptr_t)r.dst % 4 != 0 || (r.bytes > 0 && (!r.src || !r.dst))) return -3;
        if (r.kind != 0 && r.kind != 1) return -4;
        return r.bytes;
    });
    if (chunks <= 0) return (int)chunks;                            // a code; or every range is empty: nothing to launch
    rd_launch(avg_step_kernel, dim3((unsigned)chunks), dim3(AVG_THREADS), 0, (hipStream_t)stream, table_dev, n, (const int*)iter_dev, mode,
              one_minus_decay, (int)start);
    return (int)hipGetLastError();
}
