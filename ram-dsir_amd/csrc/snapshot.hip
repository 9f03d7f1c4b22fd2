// snapshot.hip -- rd_snapshot: n device ranges to (direction 0, gather) or from (direction 1, scatter) ONE contiguous staging buffer,
// with two 64-bit checksums per range (train.py --ckpt_every / --resume, ramdsir/ckpt.py).  No reference counterpart: the reference
// writes three state_dicts with torch.save and never reads one back into a trainer (code/train.py:342-360).
//
// Two launches: (1) a small clear of the 2 n sums; (2) one workgroup per chunk of RD_SNAP_CHUNK bytes, chunks counted from the start
// of their range, the grid flat over the chunks of all ranges: the walk of range_walk.h (lookup, alignment split, host-side table
// check).  A workgroup copies its chunk -- the quads of the split in batches of SNAP_QUADS loads per thread that are all issued before
// the batch's first store -- and adds the words it moved into
//     s1 = sum w[i],   s2 = sum (i + 1) w[i]      (mod 2^64, i the word index within the RANGE)
// with one pair of 64-bit integer atomic adds per workgroup.  Integer addition commutes: the same bits whatever the arrival order.
// The atomics of one range all land on one address pair, and atomics on one line are served one after the other: with 16 KiB chunks
// and the sums packed side by side, the three parameter-sized arenas of a trainer (2972 workgroups, 5944 atomics on one line) took 60 us
// against a 14 us plain copy of the same bytes; with 64 KiB chunks (1/4 of the atomics) and one 128-byte line of the sums buffer per
// range (RD_SNAP_SUM_STRIDE: the arenas' pairs in different lines) 21 us, and with both sums in one wave instruction 18 us
// (profiles/ckpt.md).
#include "range_walk.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int SNAP_THREADS = 256;
constexpr int SNAP_WORDS = RD_SNAP_CHUNK / 4;                       // 32-bit words of a chunk
// 16-byte loads per thread and batch, all in flight together.  (8 would halve the batches, but integer addition reassociates: the
// scheduler then keeps a batch's 32 products alive at once, 142 registers, 3 workgroups per CU -- or spills when bounded.)
constexpr int SNAP_QUADS = 4;
constexpr int SNAP_BATCH = SNAP_QUADS * SNAP_THREADS;               // quads of a batch (16 KiB)
static_assert(RD_SNAP_CHUNK % (SNAP_BATCH * 16) == 0, "a chunk is a whole number of batches");
static_assert(RD_SNAP_SUM_STRIDE >= 2, "two sums per range");
static_assert(sizeof(rd_snap_range_t) == 32, "rd_snap_range_t is four 8-byte words");

using namespace rdwalk;
typedef unsigned long long u64;

// the two sums of each of the n ranges; the rest of a range's line is not touched
__global__ __launch_bounds__(SNAP_THREADS) void snapshot_clear_kernel(u64* __restrict__ sums, int m) {
    const int i = blockIdx.x * SNAP_THREADS + threadIdx.x;
    if (i < m) sums[(long long)(i >> 1) * RD_SNAP_SUM_STRIDE + (i & 1)] = 0;
}

// a: s1 += w, t2 += j w (j the word index within the chunk; the range-level weight is added once per workgroup)
__device__ __forceinline__ void accumulate(unsigned w, int j, u64& s1, u64& t2) {
    s1 += w;
    t2 += (u64)(unsigned)j * w;
}

__global__ __launch_bounds__(SNAP_THREADS) void snapshot_copy_kernel(const rd_snap_range_t* __restrict__ table, int n,
                                                                     unsigned char* __restrict__ staging, u64* __restrict__ sums,
                                                                     int direction) {
    const long long c = blockIdx.x;
    const int t = threadIdx.x;
    const int lo = find_range(table, n, c);
    const rd_snap_range_t r = table[lo];
    long long w0;                                                   // first word of this chunk within its range
    const int len = chunk_len<SNAP_WORDS>(c, r.chunk0, r.bytes >> 2, w0);
    if (len == 0) return;
    unsigned* const in_range = (unsigned*)r.ptr + w0;
    unsigned* const in_stage = (unsigned*)(staging + r.offset) + w0;
    const g_u32* __restrict__ src = (const g_u32*)(direction == 0 ? in_range : in_stage);
    g_u32* __restrict__ dst = (g_u32*)(direction == 0 ? in_stage : in_range);
    const Split<int> sp = split16(len, src, dst);
    const int head = sp.head, nq = sp.nq, tail = sp.tail;
    const g_u32x4* __restrict__ s4 = (const g_u32x4*)(src + head);
    g_u32x4* __restrict__ d4 = (g_u32x4*)(dst + head);
    u64 s1 = 0, t2 = 0;
#pragma unroll 1
    for (int q0 = 0; q0 < nq; q0 += SNAP_BATCH) {
        u32x4 v[SNAP_QUADS];
#pragma unroll
        for (int k = 0; k < SNAP_QUADS; ++k) {
            const int q = q0 + t + k * SNAP_THREADS;
            v[k] = q < nq ? s4[q] : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < SNAP_QUADS; ++k) {
            const int q = q0 + t + k * SNAP_THREADS;
            if (q < nq) d4[q] = v[k];
            const int j = head + 4 * q;                             // an absent quad is four zero words: it adds nothing
            accumulate(v[k].x, j, s1, t2);
            accumulate(v[k].y, j + 1, s1, t2);
            accumulate(v[k].z, j + 2, s1, t2);
            accumulate(v[k].w, j + 3, s1, t2);
        }
    }
    for (int i = t; i < head; i += SNAP_THREADS) {
        const unsigned w = src[i];
        dst[i] = w;
        accumulate(w, i, s1, t2);
    }
    for (int i = tail + t; i < len; i += SNAP_THREADS) {
        const unsigned w = src[i];
        dst[i] = w;
        accumulate(w, i, s1, t2);
    }
    __shared__ u64 sh1[SNAP_THREADS / 64], sh2[SNAP_THREADS / 64];
    s1 = wave_sum(s1);
    t2 = wave_sum(t2);
    if ((t & 63) == 0) { sh1[t >> 6] = s1; sh2[t >> 6] = t2; }
    __syncthreads();
    if (t < 2) {
        u64 a = sh1[0], b = sh2[0];
#pragma unroll
        for (int w = 1; w < SNAP_THREADS / 64; ++w) { a += sh1[w]; b += sh2[w]; }
        // sum (w0 + j + 1) w[j] = (w0 + 1) sum w[j] + sum j w[j].  Lanes 0 and 1 add s1 and s2 in ONE wave instruction: the pair is
        // two neighbouring words of one line, and the line is visited once per workgroup instead of twice
        atomicAdd(sums + (long long)lo * RD_SNAP_SUM_STRIDE + t, t == 0 ? a : (u64)(w0 + 1) * a + b);
    }
}

}  // namespace

extern "C" int rd_snapshot(const rd_snap_range_t* table_host, const rd_snap_range_t* table_dev, int n, int64_t total_chunks,
                           void* staging, int64_t staging_bytes, uint64_t* sums_dev, int direction, void* stream) {
    if (n < 0 || n > (1 << 24)) return -1;
    if (direction != 0 && direction != 1) return -6;
    if (n == 0) return 0;
    if (!table_host || !table_dev || !staging || !sums_dev || staging_bytes < 0) return -1;
    if ((uintptr_t)staging % 4 != 0 || (uintptr_t)sums_dev % 8 != 0) return -3;
    int64_t end = 0;
    const int64_t chunks = walk_table<RD_SNAP_CHUNK>(table_host, n, total_chunks, [&](const rd_snap_range_t& r) -> int64_t {
        if (r.bytes < 0 || r.bytes % 4 != 0) return -2;
        if ((uintptr_t)r.ptr % 4 != 0 || r.offset % 4 != 0 || (r.bytes > 0 && !r.ptr)) return -3;
        // offsets ascend in table order: [offset, offset + bytes) starts behind the range in front and ends inside the staging buffer
        if (r.offset < end || r.bytes > staging_bytes || r.offset > staging_bytes - r.bytes) return -4;
        end = r.offset + r.bytes;
        return r.bytes;
    });
    if (chunks < 0) return (int)chunks;
    hipStream_t st = (hipStream_t)stream;
    rd_launch(snapshot_clear_kernel, dim3((2 * n + SNAP_THREADS - 1) / SNAP_THREADS), dim3(SNAP_THREADS), 0, st, (u64*)sums_dev, 2 * n);
    if (chunks > 0)
        rd_launch(snapshot_copy_kernel, dim3((unsigned)chunks), dim3(SNAP_THREADS), 0, st, table_dev, n, (unsigned char*)staging,
                  (u64*)sums_dev, direction);
    return (int)hipGetLastError();
}
