// hist.hip -- rd_hist: one TensorBoard histogram per tensor of the parameter, gradient and Adam-moment arenas (train.py --tb_hist,
// ramdsir/tb_hist.py).  No reference counterpart: the reference writes scalars and images only (code/train.py:298-329).  The bucket
// rule is TensorFlow's (upper_bound over a table of ascending double limits, the last bucket catching what lies above), the limits
// are DATA uploaded by the caller, so the kernel compares against the very doubles numpy compares against.
//
// Three launches over a table of ranges {src, count, chunk0} in the walk of range_walk.h (src is an absolute pointer: one table spans
// several arenas):
//   (1) zero: counts[n][n_limits] <- 0 (the entry point does not rely on the caller, and the library uses no hipMemsetAsync);
//   (2) count: a flat grid, one workgroup per chunk of RD_HIST_CHUNK elements.  A finite element is widened to fp64 (exact) and its
//       bucket found by a branch-free upper_bound over the limits (the same number of steps in every lane); the workgroup counts into
//       an LDS histogram with integer LDS atomics and then adds its NON-EMPTY bins to counts[range] with uint32 global vector
//       atomics.  Integer addition is associative and commutative: the counts are the same bits whichever workgroup finishes first.
//       The four float statistics use no atomics: min / max / sum / sum of squares of the chunk's finite elements (x * x of a widened
//       float is exact in fp64), the number of finite and of non-finite elements -> partial[chunk], every order fixed by the indices
//       (a thread's elements in ascending order, common.h's xor tree over the lanes, the four waves in order);
//   (3) finalize: one wave per range adds the partials of its range (lane l takes chunks l, l + 64, ... in ascending order, then the
//       xor tree) and writes the range's rd_hist_stats_t -- the decomposition of rd_step_log's health pass.
//
// Chunk size: 16384 ELEMENTS (64 KiB), 256 threads, four batches of four 16-byte loads per thread, each batch in flight together.  A
// workgroup pays per chunk for its LDS histogram -- n_limits words zeroed in front, n_limits words inspected behind (1551 with the
// default table: six of each per thread) -- and for its copy of the limits (12 KiB through L2); at 64 elements per thread that is a
// fraction of the work of the searches (eleven dependent steps per element), at rd_step_log's 4096 the copy alone would approach the
// chunk's own 16 KiB.  The arenas of the bench shape still give ~230 full chunks per arena beside the ~200 small tensors, which each
// take a workgroup of their own whatever the chunk size.  (Reasoned, not swept: no other chunk size has been timed.)
//
// LDS: the histogram is 4 bytes x RD_HIST_MAX_LIMITS = 16 KiB and the workgroup's copy of the limits 8 bytes x RD_HIST_MAX_LIMITS =
// 32 KiB, both static (a table of any admissible size fits; three workgroups share a CU's 160 KiB).  The limits sit in LDS because it
// was measured: on the bench shape's real table rd_hist takes 91 us (weights,grads) / 167 us (all four arenas) with the limits in LDS
// against 172 / 238 us with every step of every search going through the vector L1 / L2 (profiles/tb_hist.md) -- the searches, not
// the bytes, are what the kernel's time is made of.  The other variant stays selectable in the debug build (RD_HIST_LDS_LIMITS=0)
// for scripts/tb_hist_bench.py.
#include "range_walk.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_QUADS = 4;                                     // 16-byte loads per thread in flight
constexpr int HS_BATCH = HS_QUADS * HS_THREADS;                 // quads of one batch
static_assert(RD_HIST_CHUNK % (4 * HS_BATCH) == 0, "a chunk is a whole number of batches");
static_assert(sizeof(rd_hist_range_t) == 24 && sizeof(rd_hist_stats_t) == 48, "the record layouts of include/ramdsir.h");

typedef rd_hist_stats_t HistPartial;                            // a chunk's partial record has the fields of the result

struct HistAcc {
    double mn, mx, sum, sq;
    long long num, bad;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// #{i : lim[i] <= x}: the largest pos with lim[pos - 1] <= x, by halving steps from `top` (the largest power of two <= n_limits)
__device__ __forceinline__ int upper_bound(const double* __restrict__ lim, int n_limits, int top, double x) {
    int pos = 0;
    for (int step = top; step > 0; step >>= 1) {
        const int p = pos + step;
        if (p <= n_limits && lim[p - 1] <= x) pos = p;
    }
    return pos;
}

__device__ __forceinline__ void take(float x, const double* __restrict__ lim, int n_limits, int top, unsigned* hist, HistAcc& a) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {    // NaN, +-Inf: counted, in no bucket and no statistic
        a.bad += 1;
        return;
    }
    const double d = (double)x;
    const int pos = upper_bound(lim, n_limits, top, d);
    atomicAdd(&hist[pos < n_limits ? pos : n_limits - 1], 1u);
    a.mn = fmin(a.mn, d);
    a.mx = fmax(a.mx, d);
    a.sum += d;
    a.sq = d * d + a.sq;
    a.num += 1;
}

__global__ __launch_bounds__(HS_THREADS) void hist_zero_kernel(unsigned* __restrict__ counts, long long words) {
    for (long long i = (long long)blockIdx.x * HS_THREADS + threadIdx.x; i < words; i += (long long)gridDim.x * HS_THREADS) counts[i] = 0u;
}

template <bool LDS_LIMITS>
__global__ __launch_bounds__(HS_THREADS) void hist_count_kernel(const rd_hist_range_t* __restrict__ table, int n,
                                                                const double* __restrict__ limits, int n_limits, int top,
                                                                unsigned* __restrict__ counts, HistPartial* __restrict__ partial) {
    __shared__ unsigned s_hist[RD_HIST_MAX_LIMITS];
    __shared__ double s_lim[LDS_LIMITS ? RD_HIST_MAX_LIMITS : 1];
    __shared__ HistAcc s_acc[HS_THREADS / 64];
    const long long c = blockIdx.x;
    const int t = threadIdx.x;
    const int ri = rdwalk::find_range(table, n, c);
    const rd_hist_range_t r = table[ri];
    long long u0;                                                   // first element of this chunk within its range
    const int len = rdwalk::chunk_len<RD_HIST_CHUNK>(c, r.chunk0, r.count, u0);
    if (len == 0) return;                                           // (uniform over the workgroup, in front of every barrier)
    for (int i = t; i < n_limits; i += HS_THREADS) {
        s_hist[i] = 0u;
        if (LDS_LIMITS) s_lim[i] = limits[i];
    }
    __syncthreads();
    const double* __restrict__ lim = LDS_LIMITS ? s_lim : limits;
    const float* __restrict__ p = r.src + u0;
    // [0, head) word by word up to the first 16-byte boundary, then nq whole quads, then [tail, len): every index is inside the chunk
    const rdwalk::Split<int> s = rdwalk::split16(len, p);
    const float4* __restrict__ q4 = (const float4*)(p + s.head);
    HistAcc a = {__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0, 0};
    if (t < s.head) take(p[t], lim, n_limits, top, s_hist, a);
    for (int base = 0; base < s.nq; base += HS_BATCH) {
        float4 v[HS_QUADS];
#pragma unroll
        for (int k = 0; k < HS_QUADS; ++k) {
            const int q = base + t + k * HS_THREADS;
            if (q < s.nq) v[k] = q4[q];
        }
#pragma unroll
        for (int k = 0; k < HS_QUADS; ++k) {
            if (base + t + k * HS_THREADS < s.nq) {
                take(v[k].x, lim, n_limits, top, s_hist, a);
                take(v[k].y, lim, n_limits, top, s_hist, a);
                take(v[k].z, lim, n_limits, top, s_hist, a);
                take(v[k].w, lim, n_limits, top, s_hist, a);
            }
        }
    }
    if (s.tail + t < len) take(p[s.tail + t], lim, n_limits, top, s_hist, a);
    a.mn = wave_min(a.mn);
    a.mx = wave_max(a.mx);
    a.sum = wave_sum(a.sum);
    a.sq = wave_sum(a.sq);
    a.num = wave_sum(a.num);
    a.bad = wave_sum(a.bad);
    if ((t & 63) == 0) s_acc[t >> 6] = a;
    __syncthreads();                                                // the partials of the waves, and every LDS count of the chunk
    if (t == 0) {
        HistAcc w = s_acc[0];
#pragma unroll
        for (int k = 1; k < HS_THREADS / 64; ++k) {
            w.mn = fmin(w.mn, s_acc[k].mn);
            w.mx = fmax(w.mx, s_acc[k].mx);
            w.sum += s_acc[k].sum;
            w.sq += s_acc[k].sq;
            w.num += s_acc[k].num;
            w.bad += s_acc[k].bad;
        }
        partial[c] = HistPartial{w.mn, w.mx, w.sum, w.sq, w.num, w.bad};
    }
    unsigned* __restrict__ out = counts + (size_t)ri * n_limits;
    for (int i = t; i < n_limits; i += HS_THREADS) {
        const unsigned h = s_hist[i];
        if (h != 0u) atomicAdd(&out[i], h);
    }
}

// grid (ranges), one wave each: fold the partials of the range's chunks; a range without a finite element gets all zeros
__global__ __launch_bounds__(64) void hist_final_kernel(const rd_hist_range_t* __restrict__ table, const HistPartial* __restrict__ partial,
                                                        rd_hist_stats_t* __restrict__ stats) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const rd_hist_range_t r = table[i];
    const long long chunks = (r.count + RD_HIST_CHUNK - 1) / RD_HIST_CHUNK;
    HistAcc a = {__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0, 0};
    for (long long k = lane; k < chunks; k += 64) {
        const HistPartial q = partial[r.chunk0 + k];
        a.mn = fmin(a.mn, q.min);
        a.mx = fmax(a.mx, q.max);
        a.sum += q.sum;
        a.sq += q.sum_squares;
        a.num += q.num;
        a.bad += q.nonfinite;
    }
    a.mn = wave_min(a.mn);
    a.mx = wave_max(a.mx);
    a.sum = wave_sum(a.sum);
    a.sq = wave_sum(a.sq);
    a.num = wave_sum(a.num);
    a.bad = wave_sum(a.bad);
    if (lane != 0) return;
    const bool any = a.num > 0;
    stats[i] = rd_hist_stats_t{any ? a.mn : 0.0, any ? a.mx : 0.0, any ? a.sum : 0.0, any ? a.sq : 0.0, a.num, a.bad};
}

}  // namespace

extern "C" int64_t rd_hist_workspace(int64_t total_chunks) { return (total_chunks > 0 ? total_chunks : 0) * (int64_t)sizeof(HistPartial); }

extern "C" int rd_hist(const rd_hist_range_t* table_host, const rd_hist_range_t* table_dev, int n, int64_t total_chunks,
                       const double* limits_host, const double* limits_dev, int n_limits, uint32_t* counts, rd_hist_stats_t* stats,
                       void* workspace, void* stream) {
    if (!table_host || !table_dev || !limits_host || !limits_dev || !counts || !stats || !workspace) return -1;
    if (n < 1 || n > RD_HIST_MAX_RANGES) return -1;
    if ((uintptr_t)table_dev % 8 != 0 || (uintptr_t)limits_dev % 8 != 0 || (uintptr_t)counts % 4 != 0 || (uintptr_t)stats % 8 != 0 ||
        (uintptr_t)workspace % 8 != 0)
        return -1;
    if (n_limits < 2 || n_limits > RD_HIST_MAX_LIMITS) return -2;
    for (int i = 0; i < n_limits; ++i) {
        const double v = limits_host[i];
        if (!(v - v == 0.0) || (i > 0 && !(limits_host[i - 1] < v))) return -2;      // NaN and +-Inf fail the first test
    }
    const int64_t chunks = rdwalk::walk_table<RD_HIST_CHUNK>(table_host, n, total_chunks, [](const rd_hist_range_t& r) -> int64_t {
        if (!r.src || (uintptr_t)r.src % 4 != 0 || r.count < 0 || r.count > 0x7fffffffll) return -3;
        return r.count;
    });
    if (chunks < 0) return (int)chunks;
    int top = 1;
    while (top * 2 <= n_limits) top *= 2;
    hipStream_t st = (hipStream_t)stream;
    const long long words = (long long)n * n_limits;
    const long long zgrid = (words + HS_THREADS - 1) / HS_THREADS;
    rd_launch(hist_zero_kernel, dim3((unsigned)(zgrid < 1024 ? zgrid : 1024)), dim3(HS_THREADS), 0, st, (unsigned*)counts, words);
    if (chunks > 0) {                                               // (every range empty: the finalize launch writes the zeros)
        if (rd_switch("RD_HIST_LDS_LIMITS", 1))
            rd_launch(hist_count_kernel<true>, dim3((unsigned)chunks), dim3(HS_THREADS), 0, st, table_dev, n, limits_dev, n_limits, top,
                      (unsigned*)counts, (HistPartial*)workspace);
        else
            rd_launch(hist_count_kernel<false>, dim3((unsigned)chunks), dim3(HS_THREADS), 0, st, table_dev, n, limits_dev, n_limits, top,
                      (unsigned*)counts, (HistPartial*)workspace);
    }
    rd_launch(hist_final_kernel, dim3((unsigned)n), dim3(64), 0, st, table_dev, (const HistPartial*)workspace, stats);
    return (int)hipGetLastError();
}
