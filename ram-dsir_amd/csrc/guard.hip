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
// rd_grad_guard is the health pass of rd_step_log (step_log.hip) over ONE group, the whole arena: (1) one workgroup per chunk of
// RD_LOG_CHUNK gradient elements -> partial[chunk]; (2) one wave folds the partials and writes norm, scale, skip and the counters.
// The sum itself -- what a chunk and the fold add, in which order, hence every bit -- is the text of sumsq_pass.h for both.
//
// rd_guard_sync is ONE launch over range pairs {live, shadow} in the walk of range_walk.h over chunks of RD_GUARD_CHUNK bytes: its
// lookup, its batched copy of a chunk, its host-side table check.  skip set: live <- shadow (roll the BatchNorm buffers back);
// otherwise shadow <- live (remember the last good step).
#include "range_walk.h"
#include "sumsq_pass.h"

namespace {

using rdsum::Partial;
constexpr int GG_THREADS = rdsum::THREADS;
constexpr long long GG_MAX_N = 1ll << 24;                       // rd_step_log's bound: the non-finite count fits any consumer
static_assert(sizeof(rd_guard_state_t) == 40, "rd_guard_state_t is 40 bytes");

// grid (chunks of the arena): partial[chunk] = {sum of squares of the finite elements, number of the others}
__global__ __launch_bounds__(GG_THREADS) void grad_guard_partial_kernel(const float* __restrict__ grad, long long n,
                                                                        Partial* __restrict__ partial) {
    const int c = blockIdx.x;
    const long long lo = (long long)c * RD_LOG_CHUNK;
    const long long rest = n - lo;
    const int len = rest < RD_LOG_CHUNK ? (int)rest : RD_LOG_CHUNK;
    const Partial r = rdsum::chunk(grad + lo, len);
    if (threadIdx.x == 0) partial[c] = r;
}

// one wave: fold the partials, lane 0 writes the verdict and the counters
__global__ __launch_bounds__(64) void grad_guard_final_kernel(const Partial* __restrict__ partial, int chunks, float max_norm,
                                                              rd_guard_state_t* __restrict__ state) {
    const int lane = threadIdx.x;
    const Partial total = rdsum::fold(partial, 0, chunks, lane);
    const double s = total.sum;
    const long long bad = total.count;
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
    return ((n > 0 ? n : 0) + RD_LOG_CHUNK - 1) / RD_LOG_CHUNK * (int64_t)sizeof(Partial);
}

extern "C" int rd_grad_guard(const rd_grad_guard_t* p, void* stream) {
    if (!p || !p->grad || !p->workspace || !p->state) return -1;
    if ((uintptr_t)p->grad % 4 != 0 || (uintptr_t)p->workspace % 8 != 0 || (uintptr_t)p->state % 8 != 0) return -1;
    if (p->n < 1 || p->n > GG_MAX_N) return -2;
    if (!(p->max_norm >= 0.0f) || p->max_norm > 3.402823466e38f) return -3;         // NaN fails the first comparison, +Inf the second
    const int chunks = (int)((p->n + RD_LOG_CHUNK - 1) / RD_LOG_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    rd_launch(grad_guard_partial_kernel, dim3(chunks), dim3(GG_THREADS), 0, st, p->grad, (long long)p->n, (Partial*)p->workspace);
    rd_launch(grad_guard_final_kernel, dim3(1), dim3(64), 0, st, (const Partial*)p->workspace, chunks, p->max_norm, p->state);
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
