// fc_optimizer.hip -- the optimizer's step on the flat weight / gradient buffers (include/mztrain.h mztrain_opt_*): Adam or
// SGD, the rule of csrc/fc_optimizer.h, as two launches queued on the caller's stream.
//
//   fc_optimizer_kernel   a grid-stride loop over the elements; thread 0 of every workgroup reads the step count and the
//                         learning rate, forms the step's scalars in float64 (two glibc pows for Adam) and leaves them in LDS
//                         for the workgroup; 128-bit accesses when every pointer is 16-byte aligned, with a scalar tail for
//                         n % 4, scalar accesses throughout otherwise
//   fc_optimizer_advance  one thread: steps_done += 1
// The count is advanced by a launch of its own BEHIND the update on the same stream: launches of one stream run in order and
// a launch sees every write of the one before it, so every workgroup of the update reads the old count and the next step's
// update reads the new one; no thread of the updating grid writes what another block of that grid reads.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "engine_host.h"
#include "fc_optimizer.h"

namespace {

namespace fco = mz::fco;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

struct OptParams {
    int64_t n;
    float* weights;
    const float* grads;
    float* moment1;
    float* moment2;
    const double* lr;
    const int64_t* steps_done;
    double beta1, beta2, eps, weight_decay, momentum;
};

template <int kKind, bool kVector>
__global__ __launch_bounds__(kThreads) void fc_optimizer_kernel(OptParams p) {
    __shared__ fco::Step shared_step;
    if (threadIdx.x == 0)
        shared_step = fco::make_step(kKind, *p.lr, *p.steps_done + 1, p.beta1, p.beta2, p.eps, p.weight_decay, p.momentum);
    __syncthreads();
    const fco::Step s = shared_step;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const bool with_buffer = kKind == fco::kSgd && p.moment1 != nullptr;
    int64_t scalar_from = 0;
    if (kVector) {
        const int64_t quads = p.n / 4;
        scalar_from = quads * 4;
        float4* w4 = reinterpret_cast<float4*>(p.weights);
        const float4* g4 = reinterpret_cast<const float4*>(p.grads);
        float4* m4 = reinterpret_cast<float4*>(p.moment1);
        float4* v4 = reinterpret_cast<float4*>(p.moment2);
        for (int64_t q = first; q < quads; q += stride) {
            float4 w = w4[q];
            const float4 g = g4[q];
            if (kKind == fco::kAdam) {
                float4 m = m4[q], v = v4[q];
                fco::adam_element(s, g.x, &w.x, &m.x, &v.x);
                fco::adam_element(s, g.y, &w.y, &m.y, &v.y);
                fco::adam_element(s, g.z, &w.z, &m.z, &v.z);
                fco::adam_element(s, g.w, &w.w, &m.w, &v.w);
                m4[q] = m;
                v4[q] = v;
            } else if (with_buffer) {
                float4 m = m4[q];
                fco::sgd_element(s, g.x, &w.x, &m.x);
                fco::sgd_element(s, g.y, &w.y, &m.y);
                fco::sgd_element(s, g.z, &w.z, &m.z);
                fco::sgd_element(s, g.w, &w.w, &m.w);
                m4[q] = m;
            } else {
                fco::sgd_element(s, g.x, &w.x, nullptr);
                fco::sgd_element(s, g.y, &w.y, nullptr);
                fco::sgd_element(s, g.z, &w.z, nullptr);
                fco::sgd_element(s, g.w, &w.w, nullptr);
            }
            w4[q] = w;
        }
    }
    for (int64_t i = scalar_from + first; i < p.n; i += stride) {
        float w = p.weights[i];
        const float g = p.grads[i];
        if (kKind == fco::kAdam) {
            float m = p.moment1[i], v = p.moment2[i];
            fco::adam_element(s, g, &w, &m, &v);
            p.moment1[i] = m;
            p.moment2[i] = v;
        } else if (with_buffer) {
            float m = p.moment1[i];
            fco::sgd_element(s, g, &w, &m);
            p.moment1[i] = m;
        } else {
            fco::sgd_element(s, g, &w, nullptr);
        }
        p.weights[i] = w;
    }
}

__global__ __launch_bounds__(64) void fc_optimizer_advance(int64_t* steps_done) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *steps_done = *steps_done + 1;
}

// the refusals of both entries, decided on the arguments alone
int check(const char* entry, const mztrain_opt_args* a) {
    auto refuse = [&](const std::string& msg) { return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg); };
    if (!a) return refuse("null args");
    if (a->kind != MZTRAIN_OPT_ADAM && a->kind != MZTRAIN_OPT_SGD)
        return refuse("unknown kind " + std::to_string(a->kind) + " (MZTRAIN_OPT_ADAM or MZTRAIN_OPT_SGD)");
    if (a->n <= 0) return refuse("n must be positive");
    if (!a->weights || !a->grads || !a->lr || !a->steps_done)
        return refuse("null pointer in args (weights, grads, lr and steps_done are required)");
    if (!(a->weight_decay >= 0.0) || !std::isfinite(a->weight_decay))
        return refuse("weight_decay must be finite and not negative");
    if (!(a->momentum >= 0.0) || !std::isfinite(a->momentum)) return refuse("momentum must be finite and not negative");
    if (a->kind == MZTRAIN_OPT_ADAM) {
        if (!a->moment1 || !a->moment2) return refuse("null pointer in args (Adam needs moment1 and moment2)");
        if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0))
            return refuse("beta1 and beta2 must lie in [0, 1)");
        if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return refuse("eps must be positive");
    } else if (a->momentum != 0.0 && !a->moment1) {
        return refuse("null pointer in args (SGD with momentum needs moment1)");
    }
    return MZMCTS_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// what grad_fold.hip shares with the entries below: their refusals and the launch that advances the count
namespace mz {
namespace fco {

int check_opt_args(const char* entry, const mztrain_opt_args* a) { return check(entry, a); }

int queue_advance(int64_t* steps_done, void* stream) {
    fc_optimizer_advance<<<dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream)>>>(steps_done);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

}  // namespace fco
}  // namespace mz

extern "C" {

int mztrain_opt_step(const mztrain_opt_args* a, void* stream_) {
    const int rc = check("mztrain_opt_step", a);
    if (rc != MZMCTS_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool adam = a->kind == MZTRAIN_OPT_ADAM;
    OptParams p{a->n, a->weights, a->grads, nullptr, nullptr, a->lr, a->steps_done,
                a->beta1, a->beta2, a->eps, a->weight_decay, a->momentum};
    if (adam) {
        p.moment1 = a->moment1;
        p.moment2 = a->moment2;
    } else if (a->momentum != 0.0) {
        p.moment1 = a->moment1;      // (momentum 0: the kernel never sees the buffer)
    }
    const bool vector = a->n >= 4 && aligned16(p.weights) && aligned16(p.grads) && aligned16(p.moment1) && aligned16(p.moment2);
    const int64_t items = vector ? (a->n + 3) / 4 : a->n;
    const int64_t wanted = (items + kThreads - 1) / kThreads;
    const dim3 grid(static_cast<unsigned>(wanted < kMaxBlocks ? wanted : kMaxBlocks)), block(kThreads);
    if (adam && vector)
        fc_optimizer_kernel<fco::kAdam, true><<<grid, block, 0, stream>>>(p);
    else if (adam)
        fc_optimizer_kernel<fco::kAdam, false><<<grid, block, 0, stream>>>(p);
    else if (vector)
        fc_optimizer_kernel<fco::kSgd, true><<<grid, block, 0, stream>>>(p);
    else
        fc_optimizer_kernel<fco::kSgd, false><<<grid, block, 0, stream>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    fc_optimizer_advance<<<dim3(1), dim3(64), 0, stream>>>(a->steps_done);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_opt_reference(const mztrain_opt_args* a) {
    const int rc = check("mztrain_opt_reference", a);
    if (rc != MZMCTS_OK) return rc;
    fco::reference_step(a->kind == MZTRAIN_OPT_ADAM ? fco::kAdam : fco::kSgd, a->n, a->weights, a->grads, a->moment1,
                        a->moment2, *a->lr, *a->steps_done + 1, a->beta1, a->beta2, a->eps, a->weight_decay, a->momentum);
    *a->steps_done += 1;
    return MZMCTS_OK;
}

int mztrain_opt_scalars(double lr, double beta1, double beta2, int64_t t, double* out) {
    if (!out) return fail(nullptr, MZMCTS_ERR_INVALID, "mztrain_opt_scalars: null out");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || t < 1)
        return fail(nullptr, MZMCTS_ERR_INVALID, "mztrain_opt_scalars: beta1 and beta2 must lie in [0, 1), t must be positive");
    const fco::AdamScalars64 s = fco::adam_scalars(lr, beta1, beta2, t);
    out[0] = s.bc1;
    out[1] = s.bc2;
    out[2] = s.step_size;
    out[3] = s.bc2s;
    return MZMCTS_OK;
}

}  // extern "C"
