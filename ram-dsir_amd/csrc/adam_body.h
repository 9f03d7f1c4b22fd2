// adam_body.h -- the ONE source text of Adam's per-element update, shared by adam_update_kernel, adam_update_guarded_kernel
// (csrc/loss.hip) and optim_update_kernel (csrc/optim.hip).  The library is built with -ffp-contract=on: which products and sums
// become one fma is decided by the front end from the expressions below, so every kernel that includes this text rounds alike.
#pragma once

// w, m, v: parameter and both moments of one element (memory or registers); g: its gradient as the step uses it; lr_g: the
// learning rate of the element's group; bc1, sq_bc2: bias correction 1 and the square root of bias correction 2.
__device__ __forceinline__ void adam_element(float& w, float& m_io, float& v_io, float g, float lr_g, float bc1, float sq_bc2,
                                             float beta1, float beta2, float eps) {
    const float m = beta1 * m_io + (1.f - beta1) * g;
    const float v = beta2 * v_io + (1.f - beta2) * g * g;
    m_io = m;
    v_io = v;
    const float step = lr_g / bc1;
    const float denom = sqrtf(v) / sq_bc2 + eps;
    w -= step * (m / denom);
}

// the bias corrections of update number `applied` + 1 and the iteration word, rounded once from fp64; the counter advances
__device__ __forceinline__ void adam_prepare_words(float* hyper_out, int32_t* iter, float beta1, float beta2, int it, long long applied) {
    const double t = (double)(applied + 1);
    hyper_out[1] = (float)(1.0 - pow((double)beta1, t));
    hyper_out[2] = (float)(1.0 - pow((double)beta2, t));
    hyper_out[3] = (float)it;
    *iter = it + 1;
}
