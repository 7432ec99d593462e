// fc_optimizer.h -- the optimizer's update of one training step on the flat weight / gradient buffers (include/mztrain.h
// mztrain_opt_*), written once for the HIP kernel of fc_optimizer.hip and for a host compiler (mztrain_opt_reference,
// tests/fc_optimizer_check.cpp).  No HIP include.
//
// Every fused multiply-add is spelled fmaf / fma and nothing of the form a * b + c is left to the compiler (the library is
// built with -ffp-contract=off), division and sqrtf are the correctly rounded ones: host and device produce the same bits.
//
// Per element, float32:
//   both kinds  g1 = fmaf(wd, w, g)                          (wd == 0: g1 = g)
//   Adam        m = fmaf(1 - beta1, g1 - m, m)               torch's lerp; non-AMSGrad, coupled weight decay
//               v = fmaf((1 - beta2) * g1, g1, beta2 * v)
//               d = sqrtf(v) / bc2s + eps
//               w = fmaf(-step_size, m / d, w)
//   SGD         momentum != 0: buf = fmaf(momentum, buf, g1), g1 = buf    (a zero buffer: the first buf is g1 exactly)
//               w = fmaf(-lr, g1, w)                         dampening 0, no Nesterov
// Per step, float64, the expressions Python evaluates in torch's eager Adam with t the count of this step (1 for the first):
//   bc1 = 1 - beta1 ** t, bc2 = 1 - beta2 ** t, step_size = lr / bc1, bc2s = bc2 ** 0.5
// with glibc's pow (glibc_libm.h: finite non-negative bases, exponents in [2^-65, 2^63)); beta == 0 without a call.  Each
// scalar is rounded to float32 once.
#pragma once
#include <cstdint>

#include "glibc_libm.h"

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {
namespace fco {

constexpr int kAdam = 0, kSgd = 1;   // MZTRAIN_OPT_ADAM / MZTRAIN_OPT_SGD

struct AdamScalars64 {
    double bc1, bc2, step_size, bc2s;
};

MZ_HD inline double beta_power(double beta, int64_t t) {
    return beta == 0.0 ? 0.0 : libm::glibc_pow(beta, static_cast<double>(t));
}

MZ_HD inline AdamScalars64 adam_scalars(double lr, double beta1, double beta2, int64_t t) {
    AdamScalars64 s;
    s.bc1 = 1.0 - beta_power(beta1, t);
    s.bc2 = 1.0 - beta_power(beta2, t);
    s.step_size = lr / s.bc1;
    s.bc2s = libm::glibc_pow(s.bc2, 0.5);
    return s;
}

// what an element's update reads: the step's scalars, each rounded to float32 once
struct Step {
    float wd;
    float one_minus_beta1, beta2, one_minus_beta2, bc2s, eps, neg_step_size;   // Adam
    float momentum, neg_lr;                                                     // SGD
};

MZ_HD inline Step make_step(int kind, double lr, int64_t t, double beta1, double beta2, double eps, double weight_decay,
                            double momentum) {
    Step s{};
    s.wd = static_cast<float>(weight_decay);
    if (kind == kAdam) {
        const AdamScalars64 a = adam_scalars(lr, beta1, beta2, t);
        s.one_minus_beta1 = static_cast<float>(1.0 - beta1);
        s.beta2 = static_cast<float>(beta2);
        s.one_minus_beta2 = static_cast<float>(1.0 - beta2);
        s.bc2s = static_cast<float>(a.bc2s);
        s.eps = static_cast<float>(eps);
        s.neg_step_size = -static_cast<float>(a.step_size);
    } else {
        s.momentum = static_cast<float>(momentum);
        s.neg_lr = -static_cast<float>(lr);
    }
    return s;
}

MZ_HD inline float decayed(const Step& s, float w, float g) { return s.wd != 0.f ? __builtin_fmaf(s.wd, w, g) : g; }

MZ_HD inline void adam_element(const Step& s, float g, float* w, float* m, float* v) {
    const float g1 = decayed(s, *w, g);
    const float m1 = __builtin_fmaf(s.one_minus_beta1, g1 - *m, *m);
    const float scaled = s.one_minus_beta2 * g1;
    const float kept = s.beta2 * *v;
    const float v1 = __builtin_fmaf(scaled, g1, kept);
    const float root = __builtin_sqrtf(v1) / s.bc2s;
    const float d = root + s.eps;
    const float ratio = m1 / d;
    *m = m1;
    *v = v1;
    *w = __builtin_fmaf(s.neg_step_size, ratio, *w);
}

// `buf` is null for momentum 0
MZ_HD inline void sgd_element(const Step& s, float g, float* w, float* buf) {
    float g1 = decayed(s, *w, g);
    if (buf) {
        g1 = __builtin_fmaf(s.momentum, *buf, g1);
        *buf = g1;
    }
    *w = __builtin_fmaf(s.neg_lr, g1, *w);
}

// One whole step on arrays the caller can index: what mztrain_opt_reference runs on host arrays.
inline void reference_step(int kind, int64_t n, float* weights, const float* grads, float* moment1, float* moment2, double lr,
                           int64_t t, double beta1, double beta2, double eps, double weight_decay, double momentum) {
    const Step s = make_step(kind, lr, t, beta1, beta2, eps, weight_decay, momentum);
    const bool with_buffer = momentum != 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (kind == kAdam)
            adam_element(s, grads[i], weights + i, moment1 + i, moment2 + i);
        else
            sgd_element(s, grads[i], weights + i, with_buffer ? moment1 + i : nullptr);
    }
}

}  // namespace fco
}  // namespace mz
