// guard.hip -- rd_grad_guard and rd_guard_sync: the device side of train.py --clip_grad_norm / --skip_nonfinite (ramdsir/guard.py).
// They stand in front of the reference's `loss.backward(); optimizer.step()` (code/train.py:285-287), which steps on whatever gradient
// it gets: here the gradient of the whole arena is clipped by its global norm (torch.nn.utils.clip_grad_norm_ over the one optimizer),
// and a step whose gradient holds a NaN or an infinity leaves no trace in the model state.  The third entry point of the feature,
// rd_adam_step_guarded (code/train.py:285-287 as well), lives beside rd_adam_step in csrc/loss.hip, whose update body it shares.
//
// Everything is decided on the device: the verdict of a step is the 40 bytes of ONE rd_guard_state_t, written by rd_grad_guard's
// second launch and read by rd_adam_step_guarded and rd_guard_sync through the same device pointer; every launch argument is the
// same at every step, and the host reads the state only where it synchronises anyway.
//
// rd_grad_guard is the health pass of rd_step_log (csrc/step_log.hip; accumulate and wave_sum are common.h's for both) over ONE
// group: (1) one workgroup per chunk of RD_LOG_CHUNK gradient elements sums g * g in fp64 over its finite elements and counts the
// others -> partial[chunk]; (2) one wave adds the partials (lane l takes l, l + 64, ... in ascending order, then the fixed xor tree
// over the lanes) and writes norm, scale, skip and the counters.  Every order is fixed by the indices: no atomics, the same bits on
// every run.
//
// rd_guard_sync is ONE launch over range pairs {live, shadow} in the walk of range_walk.h over chunks of RD_GUARD_CHUNK bytes: its
// lookup, its batched copy of a chunk, its host-side table check.  skip set: live <- shadow (roll the BatchNorm buffers back);
// otherwise shadow <- live (remember the last good step).
#include "range_walk.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int GG_THREADS = 256;
constexpr int GG_QUADS = RD_LOG_CHUNK / 4 / GG_THREADS;         // 16-byte loads per thread and chunk, all in flight together
constexpr int GG_FOLD = 8;                                      // partials per lane and pass of the second launch
constexpr long long GG_MAX_N = 1ll << 24;                       // rd_step_log's bound: the non-finite count fits any consumer
static_assert(RD_LOG_CHUNK == GG_QUADS * 4 * GG_THREADS, "a chunk is a whole number of 16-byte loads per thread");
static_assert(sizeof(rd_guard_state_t) == 40, "rd_guard_state_t is 40 bytes");

struct GuardPartial {
    double sum;
    long long count;
};

// grid (chunks of the arena): partial[chunk] = {sum of squares of the finite elements, number of the others}
__global__ __launch_bounds__(GG_THREADS) void grad_guard_partial_kernel(const float* __restrict__ grad, long long n,
                                                                        GuardPartial* __restrict__ partial) {
    const int c = blockIdx.x, t = threadIdx.x;
    const long long lo = (long long)c * RD_LOG_CHUNK;
    const long long rest = n - lo;
    const int len = rest < RD_LOG_CHUNK ? (int)rest : RD_LOG_CHUNK;
    const float* __restrict__ p = grad + lo;
    // [0, head) scalar up to the first 16-byte boundary, then nq whole quads, then [tail, len) scalar: every index is inside the chunk
    int head = (int)((0 - ((uintptr_t)p >> 2)) & 3);
    head = head < len ? head : len;
    const int nq = (len - head) >> 2, tail = head + 4 * nq;
    const float4* __restrict__ q4 = (const float4*)(p + head);
    float4 v[GG_QUADS];
#pragma unroll
    for (int k = 0; k < GG_QUADS; ++k) {
        const int q = t + k * GG_THREADS;
        v[k] = q < nq ? q4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float h = t < head ? p[t] : 0.f;
    const float e = tail + t < len ? p[tail + t] : 0.f;
    double s = 0.0;
    int bad = 0;
    accumulate(h, s, bad);
#pragma unroll
    for (int k = 0; k < GG_QUADS; ++k) {
        accumulate(v[k].x, s, bad);
        accumulate(v[k].y, s, bad);
        accumulate(v[k].z, s, bad);
        accumulate(v[k].w, s, bad);
    }
    accumulate(e, s, bad);
    __shared__ double s_sum[GG_THREADS / 64];
    __shared__ long long s_bad[GG_THREADS / 64];
    s = wave_sum(s);
    const long long m = wave_sum((long long)bad);
    if ((t & 63) == 0) { s_sum[t >> 6] = s; s_bad[t >> 6] = m; }
    __syncthreads();
    if (t == 0) {
        GuardPartial r = {s_sum[0], s_bad[0]};
#pragma unroll
        for (int w = 1; w < GG_THREADS / 64; ++w) { r.sum += s_sum[w]; r.count += s_bad[w]; }
        partial[c] = r;
    }
}

// one wave: fold the partials, lane 0 writes the verdict and the counters
__global__ __launch_bounds__(64) void grad_guard_final_kernel(const GuardPartial* __restrict__ partial, int chunks, float max_norm,
                                                              rd_guard_state_t* __restrict__ state) {
    const int lane = threadIdx.x;
    double s = 0.0;
    long long bad = 0;
    // GG_FOLD loads per lane in flight; an absent slot adds 0.0, which leaves the sum as it is, so the order of the additions is the
    // ascending one whatever GG_FOLD is
    for (int base = lane; base < chunks; base += 64 * GG_FOLD) {
        GuardPartial r[GG_FOLD];
#pragma unroll
        for (int k = 0; k < GG_FOLD; ++k) {
            const int i = base + 64 * k;
            r[k] = i < chunks ? partial[i] : GuardPartial{0.0, 0};
        }
#pragma unroll
        for (int k = 0; k < GG_FOLD; ++k) {
            s += r[k].sum;
            bad += r[k].count;
        }
    }
    s = wave_sum(s);
    bad = wave_sum(bad);
    if (lane != 0) return;
    const float norm = (float)sqrt(s);
    const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
    const bool skip = bad > 0 || !finite;
    float scale = 1.f;
    if (!skip && max_norm > 0.f) scale = fminf(__fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)), 1.f);
    state->norm = norm;
    state->scale = scale;
    state->skip = skip ? 1 : 0;
    state->nonfinite = (int)bad;
    state->steps += 1;
    state->clipped += (scale < 1.f && !skip) ? 1 : 0;
    state->skipped += skip ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------- rd_guard_sync
constexpr int GS_THREADS = 256;
constexpr int GS_WORDS = RD_GUARD_CHUNK / 4;                        // 32-bit words of a chunk
constexpr int GS_QUADS = RD_GUARD_CHUNK / 16 / GS_THREADS;          // 16-byte accesses per thread: one batch is the chunk
static_assert(RD_GUARD_CHUNK % (GS_THREADS * 16) == 0 && GS_QUADS >= 1 && GS_QUADS <= 8, "a chunk is one batch of whole quads");
static_assert(sizeof(rd_guard_range_t) == 32, "rd_guard_range_t is four 8-byte words");

__global__ __launch_bounds__(GS_THREADS) void guard_sync_kernel(const rd_guard_range_t* __restrict__ table, int n,
                                                                const rd_guard_state_t* __restrict__ guard) {
    const long long c = blockIdx.x;
    const rd_guard_range_t r = table[rdwalk::find_range(table, n, c)];
    long long w0;                                                   // first word of this chunk within its range
    const int len = rdwalk::chunk_len<GS_WORDS>(c, r.chunk0, r.bytes >> 2, w0);
    if (len == 0) return;
    const bool back = guard->skip != 0;                             // uniform over the grid: live <- shadow
    const rdwalk::g_u32* src = (const rdwalk::g_u32*)((const unsigned*)(back ? r.shadow : r.live) + w0);
    rdwalk::g_u32* dst = (rdwalk::g_u32*)((unsigned*)(back ? r.live : r.shadow) + w0);
    rdwalk::copy_chunk<GS_QUADS, GS_THREADS>(src, dst, len);
}

}  // namespace

extern "C" int64_t rd_grad_guard_workspace(int64_t n) {
    return ((n > 0 ? n : 0) + RD_LOG_CHUNK - 1) / RD_LOG_CHUNK * (int64_t)sizeof(GuardPartial);
}

extern "C" int rd_grad_guard(const rd_grad_guard_t* p, void* stream) {
    if (!p || !p->grad || !p->workspace || !p->state) return -1;
    if ((uintptr_t)p->grad % 4 != 0 || (uintptr_t)p->workspace % 8 != 0 || (uintptr_t)p->state % 8 != 0) return -1;
    if (p->n < 1 || p->n > GG_MAX_N) return -2;
    if (!(p->max_norm >= 0.0f) || p->max_norm > 3.402823466e38f) return -3;         // NaN fails the first comparison, +Inf the second
    const int chunks = (int)((p->n + RD_LOG_CHUNK - 1) / RD_LOG_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    rd_launch(grad_guard_partial_kernel, dim3(chunks), dim3(GG_THREADS), 0, st, p->grad, (long long)p->n, (GuardPartial*)p->workspace);
    rd_launch(grad_guard_final_kernel, dim3(1), dim3(64), 0, st, (const GuardPartial*)p->workspace, chunks, p->max_norm, p->state);
    return (int)hipGetLastError();
}

extern "C" int rd_guard_sync(const rd_guard_range_t* table_host, const rd_guard_range_t* table_dev, int n, int64_t total_chunks,
                             const rd_guard_state_t* guard_dev, void* stream) {
    if (n < 0 || n > (1 << 24) || !guard_dev) return -1;
    if (n == 0) return 0;
    if (!table_host || !table_dev) return -1;
    if ((uintptr_t)guard_dev % 8 != 0) return -3;
    const int64_t chunks = rdwalk::walk_table<RD_GUARD_CHUNK>(table_host, n, total_chunks, [](const rd_guard_range_t& r) -> int64_t {
        if (r.bytes < 0 || r.bytes % 4 != 0) return -2;
        if ((uintptr_t)r.live % 4 != 0 || (uintptr_t)r.shadow % 4 != 0 || (r.bytes > 0 && (!r.live || !r.shadow))) return -3;
        return r.bytes;
    });
    if (chunks <= 0) return (int)chunks;                            // a code; or every range is empty: nothing to launch
    rd_launch(guard_sync_kernel, dim3((unsigned)chunks), dim3(GS_THREADS), 0, (hipStream_t)stream, table_dev, n, guard_dev);
    return (int)hipGetLastError();
}
