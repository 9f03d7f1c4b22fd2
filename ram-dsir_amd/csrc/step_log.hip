// step_log.hip -- rd_step_log: one row of the per-step record ring (train.py --tb_every_iter / --tb_health, ramdsir/step_log.py).
// The reference writes lr and its six loss scalars at EVERY iteration (code/train.py:298-304 Fundus, :467-473 Prostate); this appends
// them to a device-resident ring behind the step, so that the host reads them where it synchronises anyway.  With `grads` the row also
// carries the gradient norm of each of the three Adam groups (code/train.py:573-576) and the number of non-finite gradient elements
// (no reference counterpart).
//
// Two launches: (1) one workgroup per chunk of RD_LOG_CHUNK gradient elements (chunks are counted from the start of their group, so a
// chunk never straddles two groups) sums g * g in fp64 over its finite elements and counts the others -> partial[chunk]; (2) one
// workgroup adds the partials of each group (wave g: lane l takes l, l + 64, ... in ascending order, then a fixed tree over the lanes)
// and writes the 32 words of the row.  Every order is fixed by the indices: no atomics, the same bits on every run.  Without `grads`
// only (2) is launched.
#include "common.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int LOG_THREADS = 256;
constexpr int LOG_QUADS = RD_LOG_CHUNK / 4 / LOG_THREADS;       // 16-byte loads per thread and chunk, all in flight together
constexpr int LOG_FOLD = 8;                                     // partials per lane and pass of the second launch
static_assert(RD_LOG_CHUNK == LOG_QUADS * 4 * LOG_THREADS, "a chunk is a whole number of 16-byte loads per thread");
static_assert(RD_LOG_ROW == 32 && RD_LOG_MAX_REC == 16, "row layout: 8 losses, 4 hyper, 16 rec, 3 norms, 1 count");

struct LogPartial {
    double sum;
    long long count;
};

struct LogArgs {
    rd_step_log_t d;
    int cstart[4];              // chunks [cstart[g], cstart[g + 1]) belong to group g
};

// grid (chunks of the call): partial[chunk] = {sum of squares of the finite elements, number of the others}
__global__ __launch_bounds__(LOG_THREADS) void step_log_partial_kernel(LogArgs a, LogPartial* __restrict__ partial) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int g = c >= a.cstart[2] ? 2 : c >= a.cstart[1] ? 1 : 0;
    const long long lo = a.d.range[g] + (long long)(c - a.cstart[g]) * RD_LOG_CHUNK;
    const long long rest = a.d.range[g + 1] - lo;
    const int len = rest < RD_LOG_CHUNK ? (int)rest : RD_LOG_CHUNK;
    const float* __restrict__ p = a.d.grads + lo;
    // [0, head) scalar up to the first 16-byte boundary, then nq whole quads, then [tail, len) scalar: every index is inside the chunk
    int head = (int)((0 - ((uintptr_t)p >> 2)) & 3);
    head = head < len ? head : len;
    const int nq = (len - head) >> 2, tail = head + 4 * nq;
    const float4* __restrict__ q4 = (const float4*)(p + head);
    float4 v[LOG_QUADS];
#pragma unroll
    for (int k = 0; k < LOG_QUADS; ++k) {
        const int q = t + k * LOG_THREADS;
        v[k] = q < nq ? q4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float h = t < head ? p[t] : 0.f;
    const float e = tail + t < len ? p[tail + t] : 0.f;
    double s = 0.0;
    int bad = 0;
    accumulate(h, s, bad);
#pragma unroll
    for (int k = 0; k < LOG_QUADS; ++k) {
        accumulate(v[k].x, s, bad);
        accumulate(v[k].y, s, bad);
        accumulate(v[k].z, s, bad);
        accumulate(v[k].w, s, bad);
    }
    accumulate(e, s, bad);
    __shared__ double s_sum[LOG_THREADS / 64];
    __shared__ long long s_bad[LOG_THREADS / 64];
    s = wave_sum(s);
    const long long n = wave_sum((long long)bad);
    if ((t & 63) == 0) { s_sum[t >> 6] = s; s_bad[t >> 6] = n; }
    __syncthreads();
    if (t == 0) {
        LogPartial r = {s_sum[0], s_bad[0]};
#pragma unroll
        for (int w = 1; w < LOG_THREADS / 64; ++w) { r.sum += s_sum[w]; r.count += s_bad[w]; }
        partial[c] = r;
    }
}

// one workgroup: waves 0..2 fold the partials of groups 0..2, then threads 0..31 store the row
__global__ __launch_bounds__(LOG_THREADS) void step_log_row_kernel(LogArgs a, const LogPartial* __restrict__ partial) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    __shared__ double s_sum[3];
    __shared__ long long s_bad[3];
    if (a.d.grads && w < 3) {
        double s = 0.0;
        long long n = 0;
        // LOG_FOLD loads per lane in flight (the real arena has 481 + 298 + 151 chunks: one pass per group); an absent slot adds 0.0,
        // which leaves the sum as it is, so the order of the additions is the ascending one whatever LOG_FOLD is
        const int end = a.cstart[w + 1];
        for (int base = a.cstart[w] + lane; base < end; base += 64 * LOG_FOLD) {
            LogPartial r[LOG_FOLD];
#pragma unroll
            for (int k = 0; k < LOG_FOLD; ++k) {
                const int i = base + 64 * k;
                r[k] = i < end ? partial[i] : LogPartial{0.0, 0};
            }
#pragma unroll
            for (int k = 0; k < LOG_FOLD; ++k) {
                s += r[k].sum;
                n += r[k].count;
            }
        }
        s = wave_sum(s);
        n = wave_sum(n);
        if (lane == 0) { s_sum[w] = s; s_bad[w] = n; }
    }
    __syncthreads();
    if (t >= RD_LOG_ROW) return;
    float x = 0.f;
    if (t < 8) x = a.d.losses[t];
    else if (t < 12) x = a.d.hyper[t - 8];
    else if (t < 28) x = t - 12 < a.d.n_rec ? a.d.rec_mse[t - 12] : 0.f;
    else if (a.d.grads) x = t < 31 ? (float)sqrt(s_sum[t - 28]) : (float)(s_bad[0] + s_bad[1] + s_bad[2]);
    a.d.ring[(long long)a.d.row * RD_LOG_ROW + t] = x;
}

long long chunks_of(long long n) { return (n + RD_LOG_CHUNK - 1) / RD_LOG_CHUNK; }

}  // namespace

// every group may end in a ragged chunk: at most n / RD_LOG_CHUNK + 3 chunks for n elements in three groups
extern "C" int64_t rd_step_log_workspace(int64_t n) { return ((n > 0 ? n : 0) / RD_LOG_CHUNK + 3) * (int64_t)sizeof(LogPartial); }

extern "C" int rd_step_log(const rd_step_log_t* p, void* stream) {
    if (!p || !p->losses || !p->rec_mse || !p->hyper || !p->ring) return -1;
    if (p->grads && (!p->partial || (uintptr_t)p->partial % 8 != 0 || (uintptr_t)p->grads % 4 != 0)) return -1;
    if (p->rows < 1 || p->row < 0 || p->row >= p->rows) return -2;
    if (p->n_rec < 0 || p->n_rec > RD_LOG_MAX_REC) return -3;
    LogArgs a;
    a.d = *p;
    a.cstart[0] = 0;
    for (int g = 0; g < 3; ++g) a.cstart[g + 1] = 0;
    if (p->grads) {
        if (p->range[0] < 0 || p->range[3] - p->range[0] > (1ll << 24)) return -4;
        for (int g = 0; g < 3; ++g) {
            if (p->range[g + 1] < p->range[g]) return -4;
            a.cstart[g + 1] = a.cstart[g] + (int)chunks_of(p->range[g + 1] - p->range[g]);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (a.cstart[3] > 0) rd_launch(step_log_partial_kernel, dim3(a.cstart[3]), dim3(LOG_THREADS), 0, st, a, (LogPartial*)p->partial);
    rd_launch(step_log_row_kernel, dim3(1), dim3(LOG_THREADS), 0, st, a, (const LogPartial*)p->partial);
    return (int)hipGetLastError();
}
