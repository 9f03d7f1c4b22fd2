// step_log.hip -- rd_step_log: one row of the per-step record ring (train.py --tb_every_iter / --tb_health, ramdsir/step_log.py).
// The reference writes lr and its six loss scalars at EVERY iteration (code/train.py:298-304 Fundus, :467-473 Prostate); this appends
// them to a device-resident ring behind the step, so that the host reads them where it synchronises anyway.  With `grads` the row also
// carries the gradient norm of each of the three Adam groups (code/train.py:573-576) and the number of non-finite gradient elements
// (no reference counterpart).
//
// Two launches: (1) one workgroup per chunk of RD_LOG_CHUNK gradient elements (chunks are counted from the start of their group, so a
// chunk never straddles two groups) -> partial[chunk]; (2) one workgroup folds the partials of each group (wave g: group g) and
// writes the 32 words of the row.  The sum itself -- what a chunk and a fold add, in which order, hence every bit -- is the text of
// sumsq_pass.h, shared with rd_grad_guard (guard.hip).  Without `grads` only (2) is launched.
#include "sumsq_pass.h"

namespace {

using rdsum::Partial;
constexpr int LOG_THREADS = rdsum::THREADS;
static_assert(RD_LOG_ROW == 32 && RD_LOG_MAX_REC == 16, "row layout: 8 losses, 4 hyper, 16 rec, 3 norms, 1 count");

struct LogArgs {
    rd_step_log_t d;
    int cstart[4];              // chunks [cstart[g], cstart[g + 1]) belong to group g
};

// grid (chunks of the call): partial[chunk] = {sum of squares of the finite elements, number of the others}
__global__ __launch_bounds__(LOG_THREADS) void step_log_partial_kernel(LogArgs a, Partial* __restrict__ partial) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int g = c >= a.cstart[2] ? 2 : c >= a.cstart[1] ? 1 : 0;
    const long long lo = a.d.range[g] + (long long)(c - a.cstart[g]) * RD_LOG_CHUNK;
    const long long rest = a.d.range[g + 1] - lo;
    const int len = rest < RD_LOG_CHUNK ? (int)rest : RD_LOG_CHUNK;
    const Partial r = rdsum::chunk(a.d.grads + lo, len);
    if (t == 0) partial[c] = r;
}

// one workgroup: waves 0..2 fold the partials of groups 0..2, then threads 0..31 store the row
__global__ __launch_bounds__(LOG_THREADS) void step_log_row_kernel(LogArgs a, const Partial* __restrict__ partial) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    __shared__ double s_sum[3];
    __shared__ long long s_bad[3];
    if (a.d.grads && w < 3) {
        const Partial r = rdsum::fold(partial, a.cstart[w], a.cstart[w + 1], lane);
        if (lane == 0) { s_sum[w] = r.sum; s_bad[w] = r.count; }
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
extern "C" int64_t rd_step_log_workspace(int64_t n) { return ((n > 0 ? n : 0) / RD_LOG_CHUNK + 3) * (int64_t)sizeof(Partial); }

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
    if (a.cstart[3] > 0) rd_launch(step_log_partial_kernel, dim3(a.cstart[3]), dim3(LOG_THREADS), 0, st, a, (Partial*)p->partial);
    rd_launch(step_log_row_kernel, dim3(1), dim3(LOG_THREADS), 0, st, a, (const Partial*)p->partial);
    return (int)hipGetLastError();
}
