// bn_epilogue.hip -- relu(batch_norm(x) [+ residual]) of a residual network in training as one launch forward and one
// backward (include/mztrain.h mztrain_epilogue_*): the rule and the order of the sums of csrc/bn_epilogue.h.
//
//   bn_epilogue_forward   a workgroup of 256 per channel: the sum, the centred squares and the write pass in one launch;
//                         thread 0 saves mean / invstd and updates the running statistics
//   bn_epilogue_backward  the same workgroup: sum(g) and sum(g * xhat) in one pass, then dx [and dresidual]
// kKeep (a channel of at most bne::kKeepValues values): the first pass leaves what the later passes read in LDS (forward: x;
// backward: g and xhat); larger channels are read again through L2.  Channel slices start at multiples of H * W floats,
// which need not be 16-byte aligned (15 channels of 9 values): every access is one float.  Thread t is lane t of the header's
// order and the tree over LDS pairs as bne::fold does, so the bits are the host entry's.  No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "bn_epilogue.h"
#include "engine_host.h"

namespace {

namespace bne = mz::bne;

constexpr int kThreads = bne::kLanes;
constexpr int kKept = bne::kKeepValues;
static_assert(kKept == MZTRAIN_EPILOGUE_KEEP_VALUES, "mztrain.h states the switch of form");

// every thread leaves with the sum; `partial` may be reused after the call
__device__ inline double block_fold(double* partial, double mine) {
    const int t = threadIdx.x;
    partial[t] = mine;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s /= 2) {
        if (t < s) partial[t] = partial[t] + partial[t + s];
        __syncthreads();
    }
    const double total = partial[0];
    __syncthreads();
    return total;
}

struct ForwardParams {
    const float* x;
    const float* residual;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* out;
    float* save_mean;
    float* save_invstd;
    int64_t m;
    int32_t channels, hw;
    double eps, momentum;
};

template <bool kKeep>
__global__ __launch_bounds__(kThreads) void bn_epilogue_forward(ForwardParams p) {
    __shared__ double partial[kThreads];
    __shared__ float kept[kKeep ? kKept : 1];
    const int t = threadIdx.x;
    const int32_t c = blockIdx.x;
    const int32_t dn = kThreads / p.hw, dhw = kThreads % p.hw;
    const bne::Cursor first = bne::cursor_at(t, p.hw);

    double acc = 0.0;
    bne::Cursor at = first;
    for (int64_t i = t; i < p.m; i += kThreads) {
        const float v = p.x[bne::offset_of(at, c, p.channels, p.hw)];
        if (kKeep) kept[i] = v;
        acc = acc + static_cast<double>(v);
        bne::advance(&at, dn, dhw, p.hw);
    }
    const double mean64 = bne::mean_of(block_fold(partial, acc), p.m);

    acc = 0.0;
    at = first;
    for (int64_t i = t; i < p.m; i += kThreads) {
        const float v = kKeep ? kept[i] : p.x[bne::offset_of(at, c, p.channels, p.hw)];
        acc = bne::centred_square(v, mean64, acc);
        bne::advance(&at, dn, dhw, p.hw);
    }
    const double sumsq = block_fold(partial, acc);
    const bne::Stats st = bne::make_stats(mean64, sumsq, p.m, p.eps);
    if (t == 0) {
        p.save_mean[c] = st.mean;
        p.save_invstd[c] = st.invstd;
        p.running_mean[c] = bne::running_update(p.running_mean[c], st.mean, p.momentum);
        p.running_var[c] = bne::running_update(p.running_var[c], st.unbiased, p.momentum);
    }

    const float gamma = p.gamma[c], beta = p.beta[c];
    const bool with_residual = p.residual != nullptr;
    at = first;
    for (int64_t i = t; i < p.m; i += kThreads) {
        const int64_t off = bne::offset_of(at, c, p.channels, p.hw);
        const float v = kKeep ? kept[i] : p.x[off];
        p.out[off] = bne::forward_element(v, st.mean, st.invstd, gamma, beta, with_residual, with_residual ? p.residual[off] : 0.f);
        bne::advance(&at, dn, dhw, p.hw);
    }
}

struct BackwardParams {
    const float* dy;
    const float* x;
    const float* out;
    const float* gamma;
    const float* save_mean;
    const float* save_invstd;
    float* dx;
    float* dresidual;
    float* dgamma;
    float* dbeta;
    int64_t m;
    int32_t channels, hw;
};

template <bool kKeep>
__global__ __launch_bounds__(kThreads) void bn_epilogue_backward(BackwardParams p) {
    __shared__ double partial[kThreads];
    __shared__ float kept_g[kKeep ? kKept : 1];
    __shared__ float kept_xhat[kKeep ? kKept : 1];
    const int t = threadIdx.x;
    const int32_t c = blockIdx.x;
    const int32_t dn = kThreads / p.hw, dhw = kThreads % p.hw;
    const bne::Cursor first = bne::cursor_at(t, p.hw);
    const float mean = p.save_mean[c], invstd = p.save_invstd[c];

    double sum_g = 0.0, sum_gx = 0.0;
    bne::Cursor at = first;
    for (int64_t i = t; i < p.m; i += kThreads) {
        const int64_t off = bne::offset_of(at, c, p.channels, p.hw);
        const float g = bne::masked(p.dy[off], p.out[off]);
        const float xhat = bne::xhat_of(p.x[off], mean, invstd);
        if (kKeep) {
            kept_g[i] = g;
            kept_xhat[i] = xhat;
        }
        sum_g = sum_g + static_cast<double>(g);
        sum_gx = __builtin_fma(static_cast<double>(g), static_cast<double>(xhat), sum_gx);
        bne::advance(&at, dn, dhw, p.hw);
    }
    const double dbeta64 = block_fold(partial, sum_g);
    const double dgamma64 = block_fold(partial, sum_gx);
    const bne::BackwardScalars b = bne::make_backward(dbeta64, dgamma64, p.m, p.gamma[c], invstd);
    if (t == 0) {
        p.dbeta[c] = b.dbeta;
        p.dgamma[c] = b.dgamma;
    }

    at = first;
    for (int64_t i = t; i < p.m; i += kThreads) {
        const int64_t off = bne::offset_of(at, c, p.channels, p.hw);
        const float g = kKeep ? kept_g[i] : bne::masked(p.dy[off], p.out[off]);
        const float xhat = kKeep ? kept_xhat[i] : bne::xhat_of(p.x[off], mean, invstd);
        p.dx[off] = bne::dx_element(b, g, xhat);
        if (p.dresidual) p.dresidual[off] = g;
        bne::advance(&at, dn, dhw, p.hw);
    }
}

int refuse(const char* entry, const std::string& msg) {
    return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg);
}

// the refusals shared by the four entries, decided on the sizes alone
int check_shape(const char* entry, int64_t batch, int32_t channels, int32_t hw) {
    if (channels < 1) return refuse(entry, "channels must be at least 1");
    if (batch < 1 || hw < 1) return refuse(entry, "batch and hw must be positive");
    if (hw > (1 << 30) || batch > (INT64_C(1) << 40) / hw)
        return refuse(entry, "hw beyond 2^30 or batch * hw beyond 2^40 values per channel");
    if (batch * hw < 2) return refuse(entry, "batch * hw must be at least 2 values per channel (M < 2 has no variance)");
    return MZMCTS_OK;
}

int check_forward(const char* entry, const mztrain_epilogue_forward_args* a) {
    if (!a) return refuse(entry, "null args");
    if (!a->x || !a->gamma || !a->beta || !a->running_mean || !a->running_var || !a->out || !a->save_mean || !a->save_invstd)
        return refuse(entry, "null pointer in args (residual alone may be null)");
    const int rc = check_shape(entry, a->batch, a->channels, a->hw);
    if (rc != MZMCTS_OK) return rc;
    if (!(a->eps >= 0.0) || !(a->momentum >= 0.0 && a->momentum <= 1.0))
        return refuse(entry, "eps must not be negative and momentum must lie in [0, 1]");
    return MZMCTS_OK;
}

int check_backward(const char* entry, const mztrain_epilogue_backward_args* a) {
    if (!a) return refuse(entry, "null args");
    if (!a->dy || !a->x || !a->out || !a->gamma || !a->save_mean || !a->save_invstd || !a->dx || !a->dgamma || !a->dbeta)
        return refuse(entry, "null pointer in args (dresidual alone may be null)");
    return check_shape(entry, a->batch, a->channels, a->hw);
}

}  // namespace

extern "C" {

int mztrain_epilogue_forward(const mztrain_epilogue_forward_args* a, void* stream_) {
    const int rc = check_forward("mztrain_epilogue_forward", a);
    if (rc != MZMCTS_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const ForwardParams p{a->x, a->residual, a->gamma, a->beta, a->running_mean, a->running_var, a->out,
                          a->save_mean, a->save_invstd, a->batch * a->hw, a->channels, a->hw, a->eps, a->momentum};
    const dim3 grid(static_cast<unsigned>(a->channels)), block(kThreads);
    if (p.m <= kKept)
        bn_epilogue_forward<true><<<grid, block, 0, stream>>>(p);
    else
        bn_epilogue_forward<false><<<grid, block, 0, stream>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_epilogue_backward(const mztrain_epilogue_backward_args* a, void* stream_) {
    const int rc = check_backward("mztrain_epilogue_backward", a);
    if (rc != MZMCTS_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const BackwardParams p{a->dy, a->x, a->out, a->gamma, a->save_mean, a->save_invstd, a->dx, a->dresidual,
                           a->dgamma, a->dbeta, a->batch * a->hw, a->channels, a->hw};
    const dim3 grid(static_cast<unsigned>(a->channels)), block(kThreads);
    if (p.m <= kKept)
        bn_epilogue_backward<true><<<grid, block, 0, stream>>>(p);
    else
        bn_epilogue_backward<false><<<grid, block, 0, stream>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_epilogue_reference_forward(const mztrain_epilogue_forward_args* a) {
    const int rc = check_forward("mztrain_epilogue_reference_forward", a);
    if (rc != MZMCTS_OK) return rc;
    bne::reference_forward(bne::Shape{a->batch, a->channels, a->hw}, a->x, a->residual, a->gamma, a->beta, a->running_mean,
                           a->running_var, a->eps, a->momentum, a->out, a->save_mean, a->save_invstd);
    return MZMCTS_OK;
}

int mztrain_epilogue_reference_backward(const mztrain_epilogue_backward_args* a) {
    const int rc = check_backward("mztrain_epilogue_reference_backward", a);
    if (rc != MZMCTS_OK) return rc;
    bne::reference_backward(bne::Shape{a->batch, a->channels, a->hw}, a->dy, a->x, a->out, a->gamma, a->save_mean,
                            a->save_invstd, a->dx, a->dresidual, a->dgamma, a->dbeta);
    return MZMCTS_OK;
}

}  // extern "C"
