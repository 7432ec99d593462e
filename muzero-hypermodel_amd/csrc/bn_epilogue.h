// bn_epilogue.h -- relu(batch_norm(x) [+ residual]) of a residual network IN TRAINING, forward and backward (include/mztrain.h
// mztrain_epilogue_*), written once for the HIP kernels of bn_epilogue.hip and for a host compiler
// (mztrain_epilogue_reference_*, tests/bn_epilogue_check.cpp).  No HIP include.
//
// Every fused multiply-add is spelled fmaf / fma and nothing of the form a * b + c is left to the compiler (the library is
// built with -ffp-contract=off); float64 division and square root are the correctly rounded ones: host and device produce
// the same bits.
//
// x is NCHW float32; channel c holds M = N * HW values, value i (0 <= i < M) at x[((i / HW) * C + c) * HW + i % HW].
//
// The order of every sum over a channel (kLanes = 256, the workgroup's thread count):
//   lane t adds its terms i = t, t + kLanes, t + 2 kLanes, ... in ascending i to a float64 zero;
//   the kLanes partial sums are folded as a tree: for s = kLanes / 2, kLanes / 4, ..., 1: p[t] = p[t] + p[t + s], t < s;
//   p[0] is the sum.  (A lane without a term contributes +0.)
//
// Forward, per channel:
//   mean64 = sum(x) / M                         mean = float(mean64)            (saved)
//   var64  = sum(fma(d, d, .)) / M, d = double(x) - mean64                      (second pass; sums as above)
//   invstd = float(1 / sqrt(var64 + eps))                                       (saved; eps a double)
//   xhat = (x - mean) * invstd                  float32, with the ROUNDED mean and invstd
//   y = fmaf(xhat, gamma, beta) [+ residual]    out = y <= 0 ? 0 : y            (a NaN stays a NaN)
//   running_mean = fmaf(m, mean, (1 - m) * running_mean)                        m and 1 - m rounded to float32 once
//   running_var  = fmaf(m, float(sumsq / (M - 1)), (1 - m) * running_var)       the unbiased variance
// Backward, per channel, g = out > 0 ? dy : 0 (0 at out == 0, as torch's threshold_backward; a NaN out gives 0):
//   dbeta64  = sum(g)                           dbeta  = float(dbeta64)
//   dgamma64 = sum(fma(g, xhat, .))             dgamma = float(dgamma64)        xhat as in the forward, bit for bit
//   kb = float(dbeta64 / M), kg = float(dgamma64 / M)
//   dx = (gamma * invstd) * fmaf(-xhat, kg, g - kb)
//   dresidual = g
#pragma once
#include <cstdint>

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {
namespace bne {

constexpr int kLanes = 256;        // terms of a sum are dealt to this many lanes; the kernels' workgroup size
constexpr int kKeepValues = 4096;  // a channel of at most this many values stays in LDS between the kernel's passes

// where value i of a channel lives, kept incrementally: no division inside a pass
struct Cursor {
    int64_t n;      // i / HW
    int32_t hw;     // i % HW
};

MZ_HD inline Cursor cursor_at(int64_t i, int32_t hw_size) {
    Cursor c;
    c.n = i / hw_size;
    c.hw = static_cast<int32_t>(i - c.n * hw_size);
    return c;
}

// the step from value i to value i + kLanes: dn = kLanes / HW, dhw = kLanes % HW
MZ_HD inline void advance(Cursor* c, int32_t dn, int32_t dhw, int32_t hw_size) {
    c->n += dn;
    c->hw += dhw;
    if (c->hw >= hw_size) {
        c->hw -= hw_size;
        c->n += 1;
    }
}

MZ_HD inline int64_t offset_of(const Cursor& c, int32_t channel, int32_t channels, int32_t hw_size) {
    return (c.n * channels + channel) * hw_size + c.hw;
}

// ---- a channel's scalars ----------------------------------------------------------------------------------------------
struct Stats {
    float mean, invstd, unbiased;
};

MZ_HD inline double mean_of(double sum, int64_t m) { return sum / static_cast<double>(m); }

MZ_HD inline double centred_square(float x, double mean64, double acc) {
    const double d = static_cast<double>(x) - mean64;
    return __builtin_fma(d, d, acc);
}

MZ_HD inline Stats make_stats(double mean64, double sumsq, int64_t m, double eps) {
    Stats s;
    s.mean = static_cast<float>(mean64);
    const double var64 = sumsq / static_cast<double>(m);
    s.invstd = static_cast<float>(1.0 / __builtin_sqrt(var64 + eps));
    s.unbiased = static_cast<float>(sumsq / static_cast<double>(m - 1));
    return s;
}

MZ_HD inline float running_update(float running, float batch_value, double momentum) {
    const float m = static_cast<float>(momentum);
    const float keep = static_cast<float>(1.0 - momentum);
    const float kept = keep * running;
    return __builtin_fmaf(m, batch_value, kept);
}

// ---- per element ------------------------------------------------------------------------------------------------------
MZ_HD inline float xhat_of(float x, float mean, float invstd) {
    const float d = x - mean;
    return d * invstd;
}

// `residual` is read only when `with_residual`
MZ_HD inline float forward_element(float x, float mean, float invstd, float gamma, float beta, bool with_residual,
                                   float residual) {
    float y = __builtin_fmaf(xhat_of(x, mean, invstd), gamma, beta);
    if (with_residual) y = y + residual;
    return y <= 0.f ? 0.f : y;
}

MZ_HD inline float masked(float dy, float out) { return out > 0.f ? dy : 0.f; }

struct BackwardScalars {
    float dbeta, dgamma, kb, kg, scale;
};

MZ_HD inline BackwardScalars make_backward(double dbeta64, double dgamma64, int64_t m, float gamma, float invstd) {
    BackwardScalars b;
    b.dbeta = static_cast<float>(dbeta64);
    b.dgamma = static_cast<float>(dgamma64);
    b.kb = static_cast<float>(dbeta64 / static_cast<double>(m));
    b.kg = static_cast<float>(dgamma64 / static_cast<double>(m));
    b.scale = gamma * invstd;
    return b;
}

MZ_HD inline float dx_element(const BackwardScalars& b, float g, float xhat) {
    const float centred = g - b.kb;
    const float inner = __builtin_fmaf(-xhat, b.kg, centred);
    return b.scale * inner;
}

// ---- whole tensors on arrays the caller can index: what the host entries run -------------------------------------------
// Folds kLanes partial sums in place in the header's order; p[0] is the sum.
inline double fold(double* p) {
    for (int s = kLanes / 2; s >= 1; s /= 2)
        for (int t = 0; t < s; ++t) p[t] = p[t] + p[t + s];
    return p[0];
}

struct Shape {
    int64_t batch;      // N
    int32_t channels;   // C
    int32_t hw;         // H * W
    int64_t m() const { return batch * hw; }
};

// term(i, offset, acc) returns acc plus the term of value i
template <typename Term>
inline double channel_sum(const Shape& s, int32_t channel, Term term) {
    double partial[kLanes];
    const int64_t m = s.m();
    const int32_t dn = kLanes / s.hw, dhw = kLanes % s.hw;
    for (int t = 0; t < kLanes; ++t) {
        double acc = 0.0;
        if (t < m) {
            Cursor c = cursor_at(t, s.hw);
            for (int64_t i = t; i < m; i += kLanes) {
                acc = term(offset_of(c, channel, s.channels, s.hw), acc);
                advance(&c, dn, dhw, s.hw);
            }
        }
        partial[t] = acc;
    }
    return fold(partial);
}

template <typename Visit>
inline void channel_each(const Shape& s, int32_t channel, Visit visit) {
    for (int64_t n = 0; n < s.batch; ++n)
        for (int32_t hw = 0; hw < s.hw; ++hw) visit((n * s.channels + channel) * s.hw + hw);
}

// residual may be null; running_mean / running_var are updated in place
inline void reference_forward(const Shape& s, const float* x, const float* residual, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, double eps, double momentum, float* out,
                              float* save_mean, float* save_invstd) {
    const int64_t m = s.m();
    for (int32_t c = 0; c < s.channels; ++c) {
        const double sum = channel_sum(s, c, [&](int64_t at, double acc) { return acc + static_cast<double>(x[at]); });
        const double mean64 = mean_of(sum, m);
        const double sumsq = channel_sum(s, c, [&](int64_t at, double acc) { return centred_square(x[at], mean64, acc); });
        const Stats st = make_stats(mean64, sumsq, m, eps);
        save_mean[c] = st.mean;
        save_invstd[c] = st.invstd;
        running_mean[c] = running_update(running_mean[c], st.mean, momentum);
        running_var[c] = running_update(running_var[c], st.unbiased, momentum);
        const float g = gamma[c], b = beta[c];
        channel_each(s, c, [&](int64_t at) {
            out[at] = forward_element(x[at], st.mean, st.invstd, g, b, residual != nullptr, residual ? residual[at] : 0.f);
        });
    }
}

// dresidual may be null
inline void reference_backward(const Shape& s, const float* dy, const float* x, const float* out, const float* gamma,
                               const float* save_mean, const float* save_invstd, float* dx, float* dresidual, float* dgamma,
                               float* dbeta) {
    const int64_t m = s.m();
    for (int32_t c = 0; c < s.channels; ++c) {
        const float mean = save_mean[c], invstd = save_invstd[c];
        const double sum_g =
            channel_sum(s, c, [&](int64_t at, double acc) { return acc + static_cast<double>(masked(dy[at], out[at])); });
        const double sum_gx = channel_sum(s, c, [&](int64_t at, double acc) {
            return __builtin_fma(static_cast<double>(masked(dy[at], out[at])),
                                 static_cast<double>(xhat_of(x[at], mean, invstd)), acc);
        });
        const BackwardScalars b = make_backward(sum_g, sum_gx, m, gamma[c], invstd);
        dbeta[c] = b.dbeta;
        dgamma[c] = b.dgamma;
        channel_each(s, c, [&](int64_t at) {
            const float g = masked(dy[at], out[at]);
            dx[at] = dx_element(b, g, xhat_of(x[at], mean, invstd));
            if (dresidual) dresidual[at] = g;
        });
    }
}

}  // namespace bne
}  // namespace mz
