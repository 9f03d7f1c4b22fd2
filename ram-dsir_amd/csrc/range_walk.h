// range_walk.h -- the ONE text of the chunked walk over a table of device ranges: rd_snapshot (snapshot.hip), rd_avg_step (avg.hip)
// and rd_guard_sync (guard.hip) use all of it, rd_optim_step (optim.hip: a lookup of its own) the split and the host side,
// rd_grad_accum (accum.hip: one range, no table) the split.
//
// A table is n records, the same bytes on the host (read for validation only) and in device memory (uploaded once by the caller).
// Range i is cut into chunks of CHUNK units (bytes, or elements in optim.hip) from its start -- the last one ragged, a chunk never
// straddles two ranges -- and its chunk0 field is the number of chunks of the ranges in front of it.  The grid is flat over the
// chunks of all ranges, one workgroup per chunk: find_range and chunk_len give it its part, split16 the 16-byte part of that,
// copy_chunk moves it; walk_table is the host side.  Chunk sizes and batch depths are the callers' (each a measured choice, recorded
// in its file's header comment).
#pragma once
#include "common.h"

namespace rdwalk {

// ranges, arenas and the staging buffer are device allocations: global, not generic, loads and stores
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
constexpr int64_t MAX_CHUNKS = 0x7fffffffll;                        // a grid's x extent

// the last range whose first chunk is <= c: an empty range shares its first chunk with the range behind it and is never chosen
template <typename R>
__device__ __forceinline__ int find_range(const R* __restrict__ table, int n, long long c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// chunk c of a range of `size` units whose first chunk is chunk0: u0 = its first unit within the range; returns its length, or 0
// for a table that does not match the grid: touch nothing
template <int UNITS>
__device__ __forceinline__ int chunk_len(long long c, long long chunk0, long long size, long long& u0) {
    u0 = (c - chunk0) * UNITS;
    const long long rest = size - u0;
    if (c < chunk0 || rest <= 0) return 0;
    return rest < UNITS ? (int)rest : UNITS;
}

// [0, head) word by word up to the first 16-byte boundary of `first`, then nq whole quads, then [tail, len) word by word; sides
// that are aligned differently (some other pointer differs from `first` in its low four bits) have no common boundary: head = len.
// split16 is split_at(len, split_head(...)); optim.hip takes the two steps apart, the head once in front of its three-way branch
// and the quads inside each body, where a value kept across the branch would cost scalar registers.
template <typename I> struct Split { I head, nq, tail; };
template <typename I, typename A, typename... B>
__device__ __forceinline__ I split_head(I len, A first, B... others) {
    I head = (I)((0 - ((uintptr_t)first >> 2)) & 3);
    if (((uintptr_t(0) | ... | ((uintptr_t)first ^ (uintptr_t)others)) & 15) != 0) head = len;
    return head < len ? head : len;
}
template <typename I>
__device__ __forceinline__ Split<I> split_at(I len, I head) {
    const I nq = (len - head) >> 2, tail = head + 4 * nq;
    return Split<I>{head, nq, tail};
}
template <typename I, typename A, typename... B>
__device__ __forceinline__ Split<I> split16(I len, A first, B... others) {
    return split_at(len, split_head(len, first, others...));
}

// the quads of a chunk of at most QUADS * THREADS of them: every 16-byte load of a thread issued before its first store
template <int QUADS, int THREADS>
__device__ __forceinline__ void load_quads(const g_u32x4* __restrict__ s4, int nq, u32x4 (&v)[QUADS]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < QUADS; ++j) {
        const int q = t + j * THREADS;
        if (q < nq) v[j] = s4[q];
    }
}
// the loaded quads to dst, then the head and tail words
template <int QUADS, int THREADS>
__device__ __forceinline__ void store_chunk(const g_u32* __restrict__ src, g_u32* dst, int len, const Split<int>& s, const u32x4 (&v)[QUADS]) {
    const int t = threadIdx.x;
    g_u32x4* d4 = (g_u32x4*)(dst + s.head);
#pragma unroll
    for (int j = 0; j < QUADS; ++j) {
        const int q = t + j * THREADS;
        if (q < s.nq) d4[q] = v[j];
    }
    for (int i = t; i < s.head; i += THREADS) dst[i] = src[i];
    for (int i = s.tail + t; i < len; i += THREADS) dst[i] = src[i];
}
template <int QUADS, int THREADS>
__device__ __forceinline__ void copy_chunk(const g_u32* __restrict__ src, g_u32* dst, int len) {
    const Split<int> s = split16(len, src, dst);
    u32x4 v[QUADS];
    load_quads<QUADS, THREADS>((const g_u32x4*)(src + s.head), s.nq, v);
    store_chunk<QUADS, THREADS>(src, dst, len, s, v);
}

// Host side.  size_of(range) returns the range's size in the units of CHUNK, or the entry point's negative code for a range it
// refuses; ranges are visited in table order, and within a range size_of's checks come before the chunk0 column.  The total is held
// to MAX_CHUNKS range by range (CAP_EACH) or once behind the loop, where `after` (the entry point's own check behind the loop, 0 or
// a code) comes first.  Returns the number of chunks, or the code.
template <int64_t CHUNK, bool CAP_EACH = true, typename R, typename F, typename A = int (*)()>
inline int64_t walk_table(const R* table, int n, int64_t total_chunks, F size_of, A after = [] { return 0; }) {
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t size = size_of(table[i]);
        if (size < 0) return size;
        if (table[i].chunk0 != chunks) return -5;
        chunks += (size + CHUNK - 1) / CHUNK;
        if (CAP_EACH && chunks > MAX_CHUNKS) return -5;
    }
    if (const int code = after()) return code;
    if (chunks != total_chunks || chunks > MAX_CHUNKS) return -5;
    return chunks;
}

}  // namespace rdwalk
