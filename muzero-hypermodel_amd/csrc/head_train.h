// head_train.h -- the reward / value / policy heads of a residual network IN TRAINING: 1 x 1 convolution with bias, flatten,
// Linear, ELU (alpha 1), Linear, forward and backward (include/mztrain.h mztrain_heads_*), written once for the HIP kernels of
// head_train.hip and for a host compiler (mztrain_heads_reference_*, tests/head_train_check.cpp).  No HIP include.
//
// Every fused multiply-add is spelled fmaf and nothing of the form a * b + c is left to the compiler (the library is built
// with -ffp-contract=off): host and device produce the same bits wherever no ELU meets a negative pre-activation (below).
//
// One call: 1 or 2 heads read one x [B][C][P] (P = H * W).  Head h has conv_w [R][C], conv_b [R], fc1_w [Hd][R P], fc1_b [Hd],
// fc2_w [O][Hd], fc2_b [O]; the flatten order is i = r * P + p.  All float32, contiguous.
//
// Forward, per sample b (float32 chains, ascending index, one rounding per fmaf):
//     flat[i = r P + p] = chain from conv_b[r]:        for c = 0..C-1:      acc = fmaf(conv_w[r][c], x[b][c][p], acc)
//     part[j][q], q = 0..3 = chain from 0:             for i = q, q + 4, .. < R P:   acc = fmaf(fc1_w[j][i], flat[i], acc)
//     pre[j]  = ((part[j][0] + part[j][1]) + (part[j][2] + part[j][3])) + fc1_b[j]
//     h[j]    = pre[j] > 0 ? pre[j] : expm1f(pre[j])                        (a NaN pre-activation takes the expm1f side)
//     logits[o] = chain from fc2_b[o]:                 for j = 0..Hd-1:     acc = fmaf(fc2_w[o][j], h[j], acc)
// flat and pre are written out for the backward, which recomputes h and nothing else.
//
// Backward, per sample b (float32 chains from 0, ascending):
//     dh[j]     = for o = 0..O-1:   acc = fmaf(dlogits[o], fc2_w[o][j], acc)
//     dpre[j]   = dh[j] * (pre[j] > 0 ? 1 : expf(pre[j]))                   (one product; * 1 is exact)
//     dflat[i]  = for j = 0..Hd-1:  acc = fmaf(dpre[j], fc1_w[j][i], acc)
//     dx[c][p]  = for head h = 0.., for r = 0..R_h-1:   acc = fmaf(conv_w_h[r][c], dflat_h[r P + p], acc)
// dx is ONE chain over every head that reads the tensor, written once, never accumulated into.
//
// Parameter gradients: every entry is a sum of T terms u_t * v_t, T = B (t = b) for the four Linear gradients, T = B P
// (t = b * P + p) for the two of the convolution:
//     dfc2_w[o][j] = sum_b dlogits[b][o] * h[b][j]          dfc2_b[o] = sum_b dlogits[b][o]
//     dfc1_w[j][i] = sum_b dpre[b][j] * flat[b][i]          dfc1_b[j] = sum_b dpre[b][j]
//     dconv_w[r][c] = sum_(b,p) dflat[b][r P + p] * x[b][c][p]        dconv_b[r] = sum_(b,p) dflat[b][r P + p]
// The order: kReduceLanes = 16 partial sums, partial l takes the terms t = l, l + 16, l + 32, .. ascending, each product
// formed exactly in float64 (24 + 24 significant bits) and added to a float64 zero with one rounding per addition (a bias term
// is u_t * 1); the 16 partials are then added in ascending l to a float64 zero and the total is rounded to float32 once.  No
// atomics, no workspace that has to be zeroed; every entry is written by every call.
//
// Host and device.  expm1f and expf are the one place where a host libm and the device's differ in bits.  Where no fc1
// pre-activation of a call is negative (or NaN) neither is evaluated on a value that matters -- expf(+-0) = 1 and
// expm1f(+-0) = +-0 exactly everywhere -- and the device entries and the reference entries agree BIT FOR BIT in every
// output.  With negative pre-activations each h[j] and each derivative expf(pre[j]) agrees within kEluUlps = 4 float32 ulps
// (both libraries are good to 1 - 2 ulps); every tensor downstream agrees within what such a relative perturbation of 4 *
// 2^-23 of h and of the derivative amounts to when it is carried through the same sums with absolute values in place of
// every operand, plus the float32 rounding of those sums (tests/head_train_reference.py: ulp_bounds).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "launch_plan.h"

namespace mz {
namespace hdt {

constexpr int kMaxHeads = 2;          // heads of one call (value and policy; the reward head alone)
constexpr int kFc1Parts = 4;          // interleaved partial chains of an fc1 pre-activation
constexpr int kReduceLanes = 16;      // partial sums of a parameter gradient's entry
constexpr int kEluUlps = 4;           // host against device: float32 ulps of an ELU output and of its derivative
constexpr int kMaxChannels = 256, kMaxPlane = 128, kMaxReduced = 16, kMaxHidden = 128, kMaxOutputs = 256;
constexpr int kMaxFlat = kMaxReduced * kMaxPlane;
constexpr int64_t kMaxBatch = 65536;  // samples of one call (a workgroup each; batch * plane and every offset stay far within int64)
constexpr int kBlock = 256;           // threads of every workgroup

// nullptr: covered; else why not
inline const char* refusal(int channels, int plane, int reduced, int hidden, int outputs, int n_heads) {
    if (n_heads < 1 || n_heads > kMaxHeads) return "one or two heads read a tensor in one call";
    if (channels < 1 || channels > kMaxChannels) return "channels must lie in [1, 256]";
    if (plane < 1 || plane > kMaxPlane) return "plane (H * W) must lie in [1, 128]";
    if (reduced < 1 || reduced > kMaxReduced) return "reduced channels must lie in [1, 16]";
    if (hidden < 1 || hidden > kMaxHidden) return "hidden units must lie in [1, 128]";
    if (outputs < 1 || outputs > kMaxOutputs) return "outputs must lie in [1, 256]";
    return nullptr;
}

struct Head {
    const float *conv_w, *conv_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    int R, Hd, O;
};

// ---- the chains ----------------------------------------------------------------------------------------------------------------
MZ_HD inline float conv_value(const float* xb, const float* w_row, float bias, int C, int P, int p) {
    float acc = bias;
    for (int c = 0; c < C; ++c) acc = fmaf(w_row[c], xb[static_cast<size_t>(c) * P + p], acc);
    return acc;
}
MZ_HD inline float fc1_part(const float* flat, const float* w_row, int n, int q) {
    float acc = 0.f;
    for (int i = q; i < n; i += kFc1Parts) acc = fmaf(w_row[i], flat[i], acc);
    return acc;
}
MZ_HD inline float fc1_fold(const float* part, float bias) { return ((part[0] + part[1]) + (part[2] + part[3])) + bias; }
MZ_HD inline float elu(float a) { return a > 0.f ? a : expm1f(a); }
MZ_HD inline float elu_slope(float a) { return a > 0.f ? 1.f : expf(a); }
MZ_HD inline float fc2_value(const float* h, const float* w_row, float bias, int Hd) {
    float acc = bias;
    for (int j = 0; j < Hd; ++j) acc = fmaf(w_row[j], h[j], acc);
    return acc;
}
MZ_HD inline float dh_value(const float* dlogits, const float* fc2_w, int O, int Hd, int j) {
    float acc = 0.f;
    for (int o = 0; o < O; ++o) acc = fmaf(dlogits[o], fc2_w[static_cast<size_t>(o) * Hd + j], acc);
    return acc;
}
MZ_HD inline float dflat_value(const float* dpre, const float* fc1_w, int Hd, int n, int i) {
    float acc = 0.f;
    for (int j = 0; j < Hd; ++j) acc = fmaf(dpre[j], fc1_w[static_cast<size_t>(j) * n + i], acc);
    return acc;
}
// one entry of dx: `dflat[h]` is head h's dflat row of this sample
MZ_HD inline float dx_value(const Head* heads, int n_heads, const float* const* dflat, int C, int P, int c, int p) {
    float acc = 0.f;
    for (int h = 0; h < n_heads; ++h)
        for (int r = 0; r < heads[h].R; ++r) acc = fmaf(heads[h].conv_w[r * C + c], dflat[h][r * P + p], acc);
    return acc;
}

// ---- the parameter gradients -----------------------------------------------------------------------------------------------------
enum Kind { kConvW = 0, kConvB, kFc1W, kFc1B, kFc2W, kFc2B, kKinds };

struct ReduceHead {                   // what the reduction of one head reads, and where its six gradients go (nullptr: not wanted)
    const float *x, *flat, *pre, *dlogits, *dpre, *dflat;
    float* out[kKinds];
    int R, Hd, O;
};

MZ_HD inline int64_t kind_entries(const ReduceHead& h, int kind, int C, int P) {
    switch (kind) {
        case kConvW: return static_cast<int64_t>(h.R) * C;
        case kConvB: return h.R;
        case kFc1W: return static_cast<int64_t>(h.Hd) * h.R * P;
        case kFc1B: return h.Hd;
        case kFc2W: return static_cast<int64_t>(h.O) * h.Hd;
        default: return h.O;
    }
}
MZ_HD inline int64_t kind_terms(int kind, int64_t batch, int P) { return kind <= kConvB ? batch * P : batch; }

// partial l of entry e: the terms l, l + 16, .. ascending, each the exact float64 product.  The entry is taken apart once, the
// (sample, position) of a convolution term is stepped, not divided out: the term loop holds two loads, a product and an add.
MZ_HD inline double reduce_partial(const ReduceHead& h, int kind, int64_t entry, int64_t terms, int lane, int C, int P) {
    const int n = h.R * P;
    const int e = static_cast<int>(entry);              // at most kMaxHidden * kMaxFlat entries in a gradient
    double acc = 0.0;
    if (kind <= kConvB) {                               // t = b * P + p
        const int r = kind == kConvW ? e / C : e, c = kind == kConvW ? e % C : 0;
        const float* u = h.dflat + r * P;
        const float* v = h.x + static_cast<size_t>(c) * P;
        int b = lane / P, p = lane % P;
        for (int64_t t = lane; t < terms; t += kReduceLanes) {
            const double a = static_cast<double>(u[static_cast<size_t>(b) * n + p]);
            acc = kind == kConvW ? acc + a * static_cast<double>(v[static_cast<size_t>(b) * C * P + p]) : acc + a;
            p += kReduceLanes;
            while (p >= P) p -= P, ++b;
        }
        return acc;
    }
    // t = b: u[t * us] (* v[t * vs], through ELU for fc2's weight); the entry is (row, col) of its gradient, a bias (row, 0)
    const bool of_fc1 = kind == kFc1W || kind == kFc1B, weight = kind == kFc1W || kind == kFc2W;
    const int cols = kind == kFc1W ? n : kind == kFc2W ? h.Hd : 1;
    const int row = e / cols, col = e - row * cols;
    const float* u = (of_fc1 ? h.dpre : h.dlogits) + row;
    const float* v = (of_fc1 ? h.flat : h.pre) + col;
    const int us = of_fc1 ? h.Hd : h.O, vs = of_fc1 ? n : h.Hd;
    for (int64_t t = lane; t < terms; t += kReduceLanes) {
        const double a = static_cast<double>(u[t * us]);
        if (!weight)
            acc = acc + a;
        else
            acc = acc + a * static_cast<double>(kind == kFc2W ? elu(v[t * vs]) : v[t * vs]);
    }
    return acc;
}
MZ_HD inline float reduce_fold(const double* partials, int stride) {
    double total = 0.0;
    for (int l = 0; l < kReduceLanes; ++l) total = total + partials[l * stride];
    return static_cast<float>(total);
}

// entries of all wanted gradients of a call, in the order head-major, kind-minor: the reduction launch's index space
struct ReducePlan {
    int64_t first[kMaxHeads * kKinds + 1];   // first[s] = entries before segment s = head * kKinds + kind
    int segments;
};
inline ReducePlan plan_reduce(const ReduceHead* heads, int n_heads, int C, int P) {
    ReducePlan plan{};
    plan.segments = n_heads * kKinds;
    for (int s = 0; s < plan.segments; ++s) {
        const ReduceHead& h = heads[s / kKinds];
        plan.first[s + 1] = plan.first[s] + (h.out[s % kKinds] ? kind_entries(h, s % kKinds, C, P) : 0);
    }
    return plan;
}

// ---- the rule on host arrays -------------------------------------------------------------------------------------------------------
inline void reference_forward(const float* x, const Head* heads, int n_heads, float* const* logits, float* const* flat,
                              float* const* pre, int64_t batch, int C, int P) {
    for (int h = 0; h < n_heads; ++h) {
        const Head& hd = heads[h];
        const int n = hd.R * P;
        for (int64_t b = 0; b < batch; ++b) {
            const float* xb = x + b * C * P;
            float* fl = flat[h] + b * n;
            for (int i = 0; i < n; ++i) fl[i] = conv_value(xb, hd.conv_w + (i / P) * C, hd.conv_b[i / P], C, P, i % P);
            float hid[kMaxHidden];
            for (int j = 0; j < hd.Hd; ++j) {
                float part[kFc1Parts];
                for (int q = 0; q < kFc1Parts; ++q) part[q] = fc1_part(fl, hd.fc1_w + static_cast<size_t>(j) * n, n, q);
                const float a = fc1_fold(part, hd.fc1_b[j]);
                pre[h][b * hd.Hd + j] = a;
                hid[j] = elu(a);
            }
            for (int o = 0; o < hd.O; ++o)
                logits[h][b * hd.O + o] = fc2_value(hid, hd.fc2_w + static_cast<size_t>(o) * hd.Hd, hd.fc2_b[o], hd.Hd);
        }
    }
}

// dpre / dflat: [B][Hd] / [B][R P] per head, written in full (the reduction reads them); dx may be nullptr
inline void reference_backward(const Head* heads, ReduceHead* red, int n_heads, float* const* dpre, float* const* dflat,
                               float* dx, int64_t batch, int C, int P) {
    for (int64_t b = 0; b < batch; ++b) {
        const float* rows[kMaxHeads] = {nullptr, nullptr};
        for (int h = 0; h < n_heads; ++h) {
            const Head& hd = heads[h];
            const int n = hd.R * P;
            float* dp = dpre[h] + b * hd.Hd;
            float* df = dflat[h] + b * n;
            for (int j = 0; j < hd.Hd; ++j)
                dp[j] = dh_value(red[h].dlogits + b * hd.O, hd.fc2_w, hd.O, hd.Hd, j) * elu_slope(red[h].pre[b * hd.Hd + j]);
            for (int i = 0; i < n; ++i) df[i] = dflat_value(dp, hd.fc1_w, hd.Hd, n, i);
            rows[h] = df;
        }
        if (dx)
            for (int c = 0; c < C; ++c)
                for (int p = 0; p < P; ++p) dx[(b * C + c) * P + p] = dx_value(heads, n_heads, rows, C, P, c, p);
    }
    for (int h = 0; h < n_heads; ++h)
        for (int kind = 0; kind < kKinds; ++kind) {
            if (!red[h].out[kind]) continue;
            const int64_t entries = kind_entries(red[h], kind, C, P), terms = kind_terms(kind, batch, P);
            for (int64_t e = 0; e < entries; ++e) {
                double partials[kReduceLanes];
                for (int l = 0; l < kReduceLanes; ++l) partials[l] = reduce_partial(red[h], kind, e, terms, l, C, P);
                red[h].out[kind][e] = reduce_fold(partials, 1);
            }
        }
}

}  // namespace hdt
}  // namespace mz
