// bn_recal.hip -- rd_bn_recal: the cumulative average of BatchNorm batch statistics over ALL sites of a forward plan in one launch
// (train.py --avg_bn_recal, ramdsir/avg_bn.py): what torch.optim.swa_utils.update_bn leaves in a BatchNorm with momentum=None --
// running_mean the running mean of the batch means, running_var the running mean of the unbiased batch variances,
// num_batches_tracked the number of batches.  No reference counterpart: the reference keeps the last iterate only.
//
// ONE launch per batch, behind the forward list of a recal plan (engine.Plan recal_bn: its finalize launches write scale / shift and
// the saved mean but no running statistic).  The grid is bn_eval_coeffs_kernel's (csrc/infer.hip): blockIdx.y = site of a device
// table, blockIdx.x strides over the channels up to the largest C of the table, so a site narrower than that has workgroups (or a
// ragged last one) that find nothing to do.  Per site and channel the batch values come from the site's statistic slots through the
// finalize's OWN device functions (bn_fin.h slot_sums + fwd_stat, contraction off): the batch mean has the bits of the `mean` vector
// the finalize of the same launch list saved.  With x the batch value and k the batch index, passed by value:
//     k == 0:  run = x                                       (a plain store: the old content is not read)
//     k > 0:   d = x - run;  t = w * d;  run = run + t       w = 1.0f / (float)(k + 1), the division correctly rounded
// three separately rounded fp32 operations, never an fma -- rd_avg_step's form (csrc/avg.hip): the library is built with
// -ffp-contract=on, so the three steps go through the _rn intrinsics.  ramdsir/avg_bn.py model() is the same arithmetic in numpy.
// A few thousand channels with up to 64 slot pairs each: the kernel is latency-bound and only has to be one launch.
#include "common.h"
#include "bn_fin.h"
#include "../../include/ramdsir.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                            // over the channels of a site: the stride loop takes the rest
static_assert(sizeof(rd_bn_recal_site_t) == 56, "rd_bn_recal_site_t is five pointers, a float and three 32-bit integers");

__device__ __forceinline__ float recal_word(float x, float run, float w) {
    const float d = __fsub_rn(x, run);
    const float t = __fmul_rn(w, d);
    return __fadd_rn(run, t);
}

__global__ __launch_bounds__(kThreads) void bn_recal_kernel(const rd_bn_recal_site_t* __restrict__ sites, int k, float eps) {
    const rd_bn_recal_site_t s = sites[blockIdx.y];
    const float w = __fdiv_rn(1.0f, (float)((long long)k + 1));
    for (int c = blockIdx.x * kThreads + threadIdx.x; c < s.C; c += gridDim.x * kThreads) {
        double s1, s2;
        rdfin::slot_sums(s.stats, 0, c, s.C, s.nslots, s1, s2);
        const float cbias = s.conv_bias ? s.conv_bias[c] : 0.f;
        const rdfin::FwdStat r = rdfin::fwd_stat(s1, s2, s.count, cbias, eps);
        if (k == 0) {
            s.running_mean[c] = r.mean;
            s.running_var[c] = r.unb;
        } else {
            s.running_mean[c] = recal_word(r.mean, s.running_mean[c], w);
            s.running_var[c] = recal_word(r.unb, s.running_var[c], w);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<long long*>(s.num_batches_tracked) = (long long)k + 1;
}

}  // namespace

extern "C" int rd_bn_recal(const rd_bn_recal_site_t* sites_host, const rd_bn_recal_site_t* sites_dev, int n_sites, int max_C, int32_t k,
                           float eps, void* stream) {
    if (!sites_host || !sites_dev || n_sites < 1 || n_sites > RD_BN_RECAL_MAX_SITES || max_C < 1) return -1;
    if (k < 0) return -2;
    if (!(eps >= 0.0f)) return -7;                                      // NaN fails the comparison
    for (int i = 0; i < n_sites; ++i) {
        const rd_bn_recal_site_t& s = sites_host[i];
        if (!s.stats || !s.running_mean || !s.running_var || !s.num_batches_tracked) return -3;
        if ((uintptr_t)s.stats % 16 != 0 || (uintptr_t)s.running_mean % 4 != 0 || (uintptr_t)s.running_var % 4 != 0 ||
            (uintptr_t)s.conv_bias % 4 != 0 || (uintptr_t)s.num_batches_tracked % 8 != 0)
            return -3;
        if (s.C < 1 || s.C > max_C) return -4;
        if (!(s.count >= 1.0f)) return -5;                              // NaN fails the comparison
        if (s.nslots < 8 || s.nslots > RD_STAT_SLOTS || s.nslots % 8 != 0) return -6;
    }
    const int64_t b = ((int64_t)max_C + kThreads - 1) / kThreads;
    rd_launch(bn_recal_kernel, dim3((unsigned)(b > kMaxBlocks ? kMaxBlocks : b), (unsigned)n_sites), dim3(kThreads), 0, (hipStream_t)stream,
              sites_dev, (int)k, eps);
    return (int)hipGetLastError();
}
