// rescale_train.h -- the backward of the per-plane min-max rescale of a residual network's hidden state IN TRAINING
// (include/mztrain.h mztrain_rescale_*; models.board_rescale, reference models.py:525-549), written once for the HIP kernel of
// rescale_train.hip and for a host compiler (mztrain_rescale_reference_backward, tests/rescale_train_check.cpp), and the
// launch's plan.  No HIP include.
//
// A row is one (sample, channel) plane of P = h * w floats; x is the forward's input, g the gradient of its output.
//
// Forward (unit_rescale_kernel of net_kernels.hip, not repeated here), float32:
//   lo, hi = min, max of the row (a NaN wins both);  s = hi - lo;  if s < 1e-5f: s = s + 1e-5f;  y_p = (x_p - lo) / s
// Backward: lo, hi, s and y_p are formed again from x by exactly those float32 operations -- the same bits, nothing but x is
// saved --, then in float64:
//   n_lo = #{p: x_p == lo}, n_hi = #{p: x_p == hi}        (-0.0 == +0.0: both are counted)
//   S0 = sum_p g_p, S1 = sum_p g_p * y_p                   ascending p from a float64 zero; each product is exact in float64
//   dlo = -(S0 - S1) / s                                   every path into lo: the shift, and the span (s = hi - lo)
//   dhi = -S1 / s                                          the span alone; the 1e-5 branch has derivative 1 on both sides
//   dx_p = g_p / s  [+ dlo / n_lo if x_p == lo]  [+ dhi / n_hi if x_p == hi], added in this order, rounded to float32 once
// Ties share an extreme's gradient evenly (torch's amin / amax), the usual case: the input is a ReLU output, whose minimum
// is a run of zeros.  A constant plane has every position at both extremes.  A NaN in a row makes s, and with it the whole
// row's dx, NaN, and no other row's.  Nothing of the form a * b + c is left to the compiler (the library is built with
// -ffp-contract=off) and float64 division is the correctly rounded one: host and device produce the same bits.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {
namespace rst {

constexpr int kMaxRowLen = 128;            // the bound of mzmcts_unit_rescale
constexpr int kBlock = 256;                // threads of a workgroup; at most this many rows per workgroup
constexpr int kMinRows = 16;               // rows per workgroup a small launch is not split below
constexpr int kSpread = 256;               // workgroups a launch is spread over where it has the rows: the CUs of an MI355X
constexpr size_t kLdsBytes = 160 * 1024;   // LDS of a CU
constexpr int64_t kMaxFloats = INT64_C(0x7fffffff);   // rows * P stays below 2^31

// ---- the rule, one row: x, g and dx are the row's P floats; dx may be g (every dx_p is written after g_p's last read) -----
struct Extremes {
    float lo, hi, s;
};

MZ_HD inline Extremes extremes_of(const float* x, int P) {
    float lo = x[0], hi = x[0];
    for (int p = 1; p < P; ++p) {
        const float v = x[p];
        lo = (v < lo || v != v) ? v : lo;
        hi = (v > hi || v != v) ? v : hi;
    }
    float s = hi - lo;
    if (s < 1e-5f) s = s + 1e-5f;
    return Extremes{lo, hi, s};
}

MZ_HD inline float unit_of(float x, const Extremes& e) {
    const float shifted = x - e.lo;
    return shifted / e.s;
}

MZ_HD inline void row_backward(const float* x, const float* g, float* dx, int P) {
    const Extremes e = extremes_of(x, P);
    int n_lo = 0, n_hi = 0;
    double s0 = 0.0, s1 = 0.0;
    for (int p = 0; p < P; ++p) {
        const float v = x[p];
        n_lo += v == e.lo ? 1 : 0;
        n_hi += v == e.hi ? 1 : 0;
        const double gp = static_cast<double>(g[p]);
        const double product = gp * static_cast<double>(unit_of(v, e));
        s0 = s0 + gp;
        s1 = s1 + product;
    }
    const double s = static_cast<double>(e.s);
    const double dlo = -(s0 - s1) / s;
    const double dhi = -s1 / s;
    const double lo_share = dlo / static_cast<double>(n_lo);     // (n_lo == 0 only in a NaN row, where nothing reads it)
    const double hi_share = dhi / static_cast<double>(n_hi);
    for (int p = 0; p < P; ++p) {
        const float v = x[p];
        double t = static_cast<double>(g[p]) / s;
        if (v == e.lo) t = t + lo_share;
        if (v == e.hi) t = t + hi_share;
        dx[p] = static_cast<float>(t);
    }
}

// ---- what the launch covers, and its plan -------------------------------------------------------------------------------------
// nullptr where covered, else the reason
inline const char* refusal(int64_t rows, int32_t row_len) {
    if (row_len < 1 || row_len > kMaxRowLen) return "row_len (H * W) must lie in [1, 128]";
    if (rows < 1) return "rows must be positive";
    if (rows > kMaxFloats / row_len) return "rows * row_len must stay below 2^31";
    return nullptr;
}

// A workgroup moves `rows_per_group` rows of x and of g through LDS, each row at `row_stride` floats from the one before:
// odd, so that the row-owning threads of a 32-lane half read 32 different banks at every p (P = 36 or 42 unpadded: 4-way and
// 2-way conflicts; an even P such as 64 or 128: all 32 lanes on one bank).  Both tiles fit a CU's LDS (at P = 128: 158 rows), and a launch with few rows is cut into small groups
// so that it reaches many CUs: TicTacToe at batch 64 is 1 024 rows of 9 -> 64 workgroups of 16 rows, not 4 of 256.
struct Plan {
    unsigned grid, block;
    int rows_per_group, row_stride;
    size_t lds;     // bytes: x rows | g rows (dx is written over g)
};

inline int row_stride_of(int32_t row_len) { return row_len | 1; }

inline bool plan_rescale_backward(int64_t rows, int32_t row_len, Plan* out) {
    *out = Plan{};
    if (refusal(rows, row_len)) return false;
    const int stride = row_stride_of(row_len);
    const int64_t fit = static_cast<int64_t>(kLdsBytes / (2 * sizeof(float) * static_cast<size_t>(stride)));
    int64_t per_group = (rows + kSpread - 1) / kSpread;
    if (per_group < kMinRows) per_group = kMinRows;
    if (per_group > kBlock) per_group = kBlock;
    if (per_group > fit) per_group = fit;
    out->rows_per_group = static_cast<int>(per_group);
    out->row_stride = stride;
    out->grid = static_cast<unsigned>((rows + per_group - 1) / per_group);
    out->block = kBlock;
    out->lds = 2 * sizeof(float) * static_cast<size_t>(per_group) * static_cast<size_t>(stride);
    return true;
}

// ---- whole tensors on arrays the caller can index: what the host entry runs -------------------------------------------------
inline void reference_backward(const float* x, const float* grad_out, float* grad_x, int64_t rows, int32_t row_len) {
    for (int64_t r = 0; r < rows; ++r)
        row_backward(x + r * row_len, grad_out + r * row_len, grad_x + r * row_len, row_len);
}

}  // namespace rst
}  // namespace mz
