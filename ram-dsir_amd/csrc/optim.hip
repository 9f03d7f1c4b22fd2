// optim.hip -- rd_optim_step: the grouped Adam of train.py --weight_decay / --wd_mode / --lr_schedule / --warmup_iters /
// --enc_lr_mult (ramdsir/optim.py).  torch's param_groups as a device table of contiguous ranges of the parameter arena, each with
// its own learning-rate multiplier and weight decay; the schedule (poly, cosine, constant, with a linear warm-up) is evaluated on the
// device from the iteration counter, so every launch argument is the same at every step.  The reference's optimizer (rd_adam_step,
// csrc/loss.hip: no decay, lr / 2 on the encoder, poly) is the two-range special case, and with that table the bits are the same:
// the per-element arithmetic is the ONE text of adam_body.h.
//
// TWO launches.  The prepare launch is one thread in fp64.  The update launch is the walk of range_walk.h over chunks of
// RD_OPT_CHUNK ELEMENTS (its alignment split and host-side table check; one workgroup per chunk, not capped: an arena of 2^31
// chunks would be 2^43 elements), with a lookup of its own, which also checks the arena bounds: a workgroup finds its range by a
// search over the chunk0 column once per workgroup, its threads looking at one entry each.  Multiplier, decay and decay mode are
// therefore uniform over the workgroup: the decay variant is chosen by ONE scalar branch into a chunk body compiled for it, and a range without decay executes neither decay
// operation (not a multiplication by one: -0 and NaN payloads would pass, but the text would no longer be rd_adam_step's).
// Range starts have any 4-byte alignment (the arena packs tensors back to back): the part of a chunk behind the first 16-byte
// boundary moves as 16-byte accesses -- the four loads per array of a thread all issued before its first store -- the words in front
// of and behind it one by one; arenas that are aligned differently from one another have no common boundary and go word by word.
#include <cmath>

#include "range_walk.h"
#include "adam_body.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_QUADS = RD_OPT_CHUNK / 4 / OPT_THREADS;           // 16-byte accesses per thread and array: one batch is the chunk
static_assert(RD_OPT_CHUNK % (OPT_THREADS * 4) == 0 && OPT_QUADS >= 1 && OPT_QUADS <= 8, "a chunk is one batch of whole quads");
static_assert(sizeof(rd_optim_range_t) == 32, "rd_optim_range_t is four 8-byte words");
static_assert(sizeof(rd_optim_t) == 88, "rd_optim_t: ramdsir/_lib.py RdOptim restates the layout");

// the arenas are device allocations: global, not generic, loads and stores
typedef __attribute__((address_space(1))) float g_f32;
typedef __attribute__((address_space(1))) f32x4 g_f32x4;

// what is uniform over a workgroup
struct OptConsts {
    float lr_g, bc1, sq_bc2, beta1, beta2, eps;
    float scale;            // the guard's (GUARDED only)
    float decay;            // D (WD == 2)
    float keep;             // 1 - lr_g * D (WD == 1)
};

// WD: 0 no decay, 1 decoupled, 2 L2
template <bool GUARDED, int WD>
__device__ __forceinline__ void optim_element(float& w, float& m, float& v, float g, const OptConsts& k) {
    if (GUARDED) g = __fmul_rn(g, k.scale);
    if (WD == 1) w = __fmul_rn(w, k.keep);
    if (WD == 2) g = __fmaf_rn(k.decay, w, g);
    adam_element(w, m, v, g, k.lr_g, k.bc1, k.sq_bc2, k.beta1, k.beta2, k.eps);
}

// len <= RD_OPT_CHUNK elements at w / g / m / v; [0, head) and [tail, len) word by word, the quads between them 16 bytes at a time
template <bool GUARDED, int WD>
__device__ __forceinline__ void optim_chunk(g_f32* w, const g_f32* __restrict__ g, g_f32* m, g_f32* v, int len, int head, const OptConsts& k) {
    const int t = threadIdx.x;
    const rdwalk::Split<int> sp = rdwalk::split_at(len, head);
    const int nq = sp.nq, tail = sp.tail;
    g_f32x4* w4 = (g_f32x4*)(w + head);
    const g_f32x4* __restrict__ g4 = (const g_f32x4*)(g + head);
    g_f32x4* m4 = (g_f32x4*)(m + head);
    g_f32x4* v4 = (g_f32x4*)(v + head);
    f32x4 W[OPT_QUADS], G[OPT_QUADS], M[OPT_QUADS], V[OPT_QUADS];
#pragma unroll
    for (int j = 0; j < OPT_QUADS; ++j) {
        const int q = t + j * OPT_THREADS;
        if (q < nq) {
            W[j] = w4[q];
            G[j] = g4[q];
            M[j] = m4[q];
            V[j] = v4[q];
        }
    }
#pragma unroll
    for (int j = 0; j < OPT_QUADS; ++j) {
        const int q = t + j * OPT_THREADS;
        if (q < nq) {
            float a[4] = {W[j].x, W[j].y, W[j].z, W[j].w}, b[4] = {M[j].x, M[j].y, M[j].z, M[j].w}, c[4] = {V[j].x, V[j].y, V[j].z, V[j].w};
            const float d[4] = {G[j].x, G[j].y, G[j].z, G[j].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) optim_element<GUARDED, WD>(a[e], b[e], c[e], d[e], k);
            m4[q] = f32x4{b[0], b[1], b[2], b[3]};
            v4[q] = f32x4{c[0], c[1], c[2], c[3]};
            w4[q] = f32x4{a[0], a[1], a[2], a[3]};
        }
    }
    // head and tail together are at most 6 words
    for (int i = t; i < head + (len - tail); i += OPT_THREADS) {
        const int e = i < head ? i : tail + (i - head);
        float a = w[e], b = m[e], c = v[e];
        optim_element<GUARDED, WD>(a, b, c, g[e], k);
        m[e] = b;
        v[e] = c;
        w[e] = a;
    }
}

__global__ void optim_prepare_kernel(const rd_optim_t p, const rd_guard_state_t* __restrict__ guard) {
    const int it = *p.iter;
    double s = 1.0;
    if (p.schedule == 0) {
        // rd_adam_step's expression: the LR in force at iteration `it` was written after iteration it-1 from ITS iter_num (train.py:289)
        if (it > 0) s = pow(1.0 - (double)(it - 1) / (double)p.total_iters, 0.9);
    } else if (p.schedule == 1) {
        const int c = it < p.total_iters ? it : p.total_iters;
        s = 0.5 * (1.0 + cos(3.14159265358979323846 * (double)c / (double)p.total_iters));
    }
    double w = 1.0;
    if (p.warmup_iters > 0) {
        w = (double)(it + 1) / (double)p.warmup_iters;
        if (w > 1.0) w = 1.0;
    }
    p.hyper_out[0] = (float)((double)p.base_lr * s * w);
    // bias corrections: the iteration number itself, or (guarded step) less the skipped steps, as adam_prepare_guarded_kernel
    long long applied = it;
    if (guard) {
        applied = (long long)it - guard->skipped;
        if (applied < 0) applied = 0;
    }
    adam_prepare_words(p.hyper_out, p.iter, p.beta1, p.beta2, it, applied);
}

template <bool GUARDED>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const rd_optim_t p, const rd_optim_range_t* __restrict__ table, int n_ranges,
                                                                   const rd_guard_state_t* __restrict__ guard) {
    OptConsts k;
    k.scale = 1.f;
    if (GUARDED) {
        if (guard->skip != 0) return;                               // a skipped step stores nothing: uniform over the grid
        k.scale = guard->scale;
    }
    const long long c = blockIdx.x;
    // the last range whose first chunk is <= c (every range has at least one chunk; chunk0 of range 0 is 0).  A binary search is a
    // chain of dependent loads in front of every workgroup's first access (seven for the trainer's 80 ranges: measured, it was most of
    // what the table cost, profiles/optim.md), so it only narrows the candidates to one per thread -- no step at all below 257
    // ranges, four for 4096 -- and the rest is ONE load per thread and a count over the workgroup: the column is ascending, so the
    // entries <= c are a prefix of the window.
    int lo = 0, hi = n_ranges - 1;
    while (hi - lo >= OPT_THREADS) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    const int cand = lo + (int)threadIdx.x;
    lo += __syncthreads_count(cand <= hi && table[cand].chunk0 <= c) - 1;
    if (lo < 0) return;                                             // (chunk0 of range 0 above c: not a table the host side accepts)
    const rd_optim_range_t r = table[lo];
    const long long e0 = (c - r.chunk0) * RD_OPT_CHUNK;             // first element of this chunk within its range
    const long long rest = r.count - e0;
    // a table that does not match the grid or the arena: touch nothing
    if (c < r.chunk0 || rest <= 0 || r.first < 0 || r.first + r.count > p.n) return;
    const int len = rest < RD_OPT_CHUNK ? (int)rest : RD_OPT_CHUNK;
    const long long base = r.first + e0;
    const float bc2 = p.hyper_out[2];
    k.lr_g = __fmul_rn(r.lr_mult, p.hyper_out[0]);
    k.bc1 = p.hyper_out[1];
    k.sq_bc2 = sqrtf(bc2);
    k.beta1 = p.beta1;
    k.beta2 = p.beta2;
    k.eps = p.eps;
    k.decay = r.weight_decay;
    k.keep = 1.f;
    g_f32* w = (g_f32*)(p.param + base);
    const g_f32* g = (const g_f32*)(p.grad + base);
    g_f32* m = (g_f32*)(p.exp_avg + base);
    g_f32* v = (g_f32*)(p.exp_avg_sq + base);
    const int head = rdwalk::split_head(len, w, g, m, v);
    if (!(r.weight_decay > 0.f)) {
        optim_chunk<GUARDED, 0>(w, g, m, v, len, head, k);
    } else if (p.wd_mode == 0) {
        k.keep = __fsub_rn(1.f, __fmul_rn(k.lr_g, r.weight_decay));
        optim_chunk<GUARDED, 1>(w, g, m, v, len, head, k);
    } else {
        optim_chunk<GUARDED, 2>(w, g, m, v, len, head, k);
    }
}

}  // namespace

extern "C" int rd_optim_step(const rd_optim_t* p, const rd_optim_range_t* table_host, const rd_optim_range_t* table_dev, int n_ranges,
                             int64_t total_chunks, const rd_guard_state_t* guard_dev, void* stream) {
    if (!p || !table_host || !table_dev || n_ranges < 1 || n_ranges > RD_OPT_MAX_RANGES) return -1;
    if (!p->param || !p->grad || !p->exp_avg || !p->exp_avg_sq || !p->iter || !p->hyper_out || p->n < 1) return -1;
    if (p->schedule < 0 || p->schedule > 2 || (p->wd_mode != 0 && p->wd_mode != 1)) return -4;
    if (p->warmup_iters < 0 || p->warmup_iters >= p->total_iters) return -4;
    int64_t next = 0;
    auto size_of = [&](const rd_optim_range_t& r) -> int64_t {
        if (r.count < 1 || r.first != next || r.count > p->n - next) return -2;
        if (!std::isfinite(r.lr_mult) || !(r.lr_mult > 0.f)) return -3;
        if (!std::isfinite(r.weight_decay) || r.weight_decay < 0.f) return -3;
        next += r.count;
        return r.count;
    };
    const int64_t chunks = rdwalk::walk_table<RD_OPT_CHUNK, false>(table_host, n_ranges, total_chunks, size_of, [&] { return next != p->n ? -2 : 0; });
    if (chunks < 0) return (int)chunks;
    hipStream_t st = (hipStream_t)stream;
    rd_launch(optim_prepare_kernel, dim3(1), dim3(1), 0, st, *p, guard_dev);
    if (guard_dev)
        rd_launch(optim_update_kernel<true>, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, *p, table_dev, n_ranges, guard_dev);
    else
        rd_launch(optim_update_kernel<false>, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, *p, table_dev, n_ranges, guard_dev);
    return (int)hipGetLastError();
}
