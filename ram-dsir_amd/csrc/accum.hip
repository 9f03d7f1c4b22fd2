// accum.hip -- rd_grad_accum: gradient accumulation for train.py --accum_steps N (ramdsir/accum.py).  Every iteration of the fused
// step leaves the gradient of its micro-batch in the gradient arena (the writers overwrite: the split reduction of wgrad.hip stores
// with beta baked into its descriptors, and rd_zero at the head of every step is part of the contract of the writers that add), so
// the sum over a window of N micro-batches lives in a SECOND fp32 arena of the same length, and this launch sits between the encoder
// backward and the optimizer tail.  No reference counterpart: the reference's batch sizes are its tables (code/train.py:35-45).
//
// ONE launch per iteration, chosen by the position k of the micro-batch in its window:
//     k == 0               acc = grad                        a word copy: the bits, NaN payloads included; grad untouched
//     0 < k < steps - 1    acc = acc + grad                  grad untouched
//     k == steps - 1       grad = (acc + grad) * inv_steps   IN PLACE in the gradient arena; acc is not written
// so everything behind it (rd_adam_step, rd_grad_guard + rd_adam_step_guarded, rd_optim_step) reads the arena it always read.  Each
// operation is rounded on its own: the library is built with -ffp-contract=on, so sum and product go through the _rn intrinsics (as
// avg.hip's three steps do).  ramdsir/accum.py model() is the same arithmetic in numpy.
//
// Elementwise, no LDS, no atomics, no reduction: the bits are a function of the inputs alone.  ONE range, so the grid-stride form
// of rd_adam_step and not the chunk table of avg.hip / optim.hip (profiles/optim.md: what the table costs on a single arena).  The
// part of the arena behind grad's first 16-byte boundary moves as 16-byte accesses where acc shares that phase -- ACC_BATCH quads of
// each side per thread and trip, every load issued before the first store -- the words in front of and behind it (at most six) one
// by one; arenas that are aligned differently have no common boundary and go word by word throughout, in the same batched form
// (the alignment split of range_walk.h, over 64-bit indices).
#include <cstring>

#include "range_walk.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int ACC_THREADS = 256;
constexpr int ACC_BATCH = 4;                                        // accesses per thread, side and trip of the grid-stride loop
// workgroups at most: 256 Ki threads with eight 16-byte loads in flight each are far more than the memory system needs, and a
// trainer's arena (a few million words) still takes ONE trip of the loop -- 4 Mi words on the 16-byte path
constexpr int ACC_MAX_BLOCKS = 1024;

using namespace rdwalk;

// MODE: 0 copy, 1 add, 2 mean.  g the gradient word, a the accumulated one
template <int MODE>
__device__ __forceinline__ unsigned accum_word(unsigned g, unsigned a, float inv) {
    if (MODE == 0) return g;
    const float s = __fadd_rn(__uint_as_float(a), __uint_as_float(g));
    return __float_as_uint(MODE == 1 ? s : __fmul_rn(s, inv));
}

template <int MODE>
__global__ __launch_bounds__(ACC_THREADS) void grad_accum_kernel(unsigned* grad_, unsigned* acc_, long long n, float inv) {
    g_u32* grad = (g_u32*)grad_;
    g_u32* acc = (g_u32*)acc_;
    g_u32* dst = MODE == 2 ? grad : acc;
    const long long tid = (long long)blockIdx.x * ACC_THREADS + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * ACC_THREADS;
    const Split<long long> sp = split16(n, grad_, acc_);
    const long long head = sp.head, nq = sp.nq, tail = sp.tail;
    const g_u32x4* g4 = (const g_u32x4*)(grad + head);
    const g_u32x4* a4 = (const g_u32x4*)(acc + head);
    g_u32x4* d4 = (g_u32x4*)(dst + head);
    for (long long q0 = tid; q0 < nq; q0 += nthreads * ACC_BATCH) {
        u32x4 G[ACC_BATCH], A[ACC_BATCH];
#pragma unroll
        for (int j = 0; j < ACC_BATCH; ++j) {
            const long long q = q0 + j * nthreads;
            if (q < nq) {
                G[j] = g4[q];
                if (MODE != 0) A[j] = a4[q];
            }
        }
#pragma unroll
        for (int j = 0; j < ACC_BATCH; ++j) {
            const long long q = q0 + j * nthreads;
            if (q < nq)
                d4[q] = MODE == 0 ? G[j]
                                  : u32x4{accum_word<MODE>(G[j].x, A[j].x, inv), accum_word<MODE>(G[j].y, A[j].y, inv),
                                          accum_word<MODE>(G[j].z, A[j].z, inv), accum_word<MODE>(G[j].w, A[j].w, inv)};
        }
    }
    // the words outside the quads: word i of them is element i in front of the quads, element tail + (i - head) behind them
    const long long nw = head + (n - tail);
    for (long long i0 = tid; i0 < nw; i0 += nthreads * ACC_BATCH) {
        unsigned G[ACC_BATCH], A[ACC_BATCH];
#pragma unroll
        for (int j = 0; j < ACC_BATCH; ++j) {
            const long long i = i0 + j * nthreads;
            if (i < nw) {
                const long long e = i < head ? i : tail + (i - head);
                G[j] = grad[e];
                if (MODE != 0) A[j] = acc[e];
            }
        }
#pragma unroll
        for (int j = 0; j < ACC_BATCH; ++j) {
            const long long i = i0 + j * nthreads;
            if (i < nw) {
                const long long e = i < head ? i : tail + (i - head);
                dst[e] = accum_word<MODE>(G[j], MODE != 0 ? A[j] : 0u, inv);
            }
        }
    }
}

}  // namespace

extern "C" int rd_grad_accum(float* grad, float* acc, int64_t n, int32_t k, int32_t steps, float inv_steps, void* stream) {
    if (!grad || !acc) return -1;
    if ((uintptr_t)grad % 4 != 0 || (uintptr_t)acc % 4 != 0) return -2;
    if (n < 1 || n > RD_ACCUM_MAX_N) return -3;
    if (steps < 1 || steps > RD_ACCUM_MAX_STEPS) return -4;
    if (k < 0 || k >= steps) return -5;
    const float want = (float)(1.0 / (double)steps);
    if (std::memcmp(&want, &inv_steps, sizeof(float)) != 0) return -6;          // the bits: NaN and -0 are refused with the rest
    const uintptr_t g0 = (uintptr_t)grad, a0 = (uintptr_t)acc, bytes = (uintptr_t)n * 4;
    if (g0 < a0 + bytes && a0 < g0 + bytes) return -7;
    if (steps == 1) return 0;                                       // a window of one: the gradient is its own mean
    const bool quads = ((g0 ^ a0) & 15) == 0;
    const int64_t per_block = (int64_t)ACC_THREADS * ACC_BATCH * (quads ? 4 : 1);
    int64_t nb = (n + per_block - 1) / per_block;
    if (nb > ACC_MAX_BLOCKS) nb = ACC_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    unsigned* g = (unsigned*)grad;
    unsigned* a = (unsigned*)acc;
    if (k == 0)
        rd_launch(grad_accum_kernel<0>, dim3((unsigned)nb), dim3(ACC_THREADS), 0, st, g, a, (long long)n, inv_steps);
    else if (k < steps - 1)
        rd_launch(grad_accum_kernel<1>, dim3((unsigned)nb), dim3(ACC_THREADS), 0, st, g, a, (long long)n, inv_steps);
    else
        rd_launch(grad_accum_kernel<2>, dim3((unsigned)nb), dim3(ACC_THREADS), 0, st, g, a, (long long)n, inv_steps);
    return (int)hipGetLastError();
}
