// grad_fold.hip -- the weight gradients of a residual training step folded and the optimizer applied (include/mztrain.h
// mztrain_fold_*): the rule of csrc/grad_fold.h as ONE launch over all parameter tensors, queued on the caller's stream, with
// fc_optimizer.hip's one-thread launch behind it that advances the step count.
//
//   grad_fold_kernel   a workgroup of 256 walks the chunk table grid-stride (at most 1 024 workgroups); a chunk is up to 1 024
//                      floats of one segment.  Thread 0 of every workgroup forms the step's scalars as fc_optimizer_kernel
//                      does.  Per chunk the segment and its `uses` are workgroup-uniform: uses == 0 skips the chunk; where the
//                      weight, moment, gradient and slot addresses are all 16-byte aligned a thread folds and updates one
//                      float4 (and the chunk's last count % 4 floats go one per thread), else every access is scalar.
// The chunk table, the segments and the per-segment uses live on the device behind the handle; the step allocates nothing,
// decides nothing on the host beyond the alignment of the base pointers, and does not synchronise.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mztrain.h"
#include "engine_host.h"
#include "grad_fold.h"

namespace mz {
namespace fco {
int check_opt_args(const char* entry, const mztrain_opt_args* a);     // fc_optimizer.hip
int queue_advance(int64_t* steps_done, void* stream);
}  // namespace fco
}  // namespace mz

struct mztrain_fold {
    int32_t n_segments = 0;
    int64_t n = 0, staging_floats = 0;
    std::vector<mz::gfold::Segment> segments;
    std::vector<int32_t> uses;
    bool uses_set = false;
    mz::gfold::FoldPlan plan{};
    mz::gfold::Segment* d_segments = nullptr;
    mz::gfold::Chunk* d_chunks = nullptr;
    int32_t* d_uses = nullptr;
};

namespace {

namespace fco = mz::fco;
namespace gfold = mz::gfold;

static_assert(sizeof(gfold::Segment) == sizeof(mztrain_fold_segment), "grad_fold.h mirrors mztrain_fold_segment");

struct FoldParams {
    const gfold::Segment* segments;
    const int32_t* uses;
    const gfold::Chunk* chunks;
    int64_t n_chunks;
    const float* staging;
    float* weights;
    float* grads;
    float* moment1;
    float* moment2;
    const double* lr;
    const int64_t* steps_done;
    double beta1, beta2, eps, weight_decay, momentum;
    int bases_aligned;      // weights, grads, staging and the moments in use all start on 16 bytes
};

template <int kKind>
__global__ __launch_bounds__(gfold::kThreads) void grad_fold_kernel(FoldParams p) {
    __shared__ fco::Step shared_step;
    if (threadIdx.x == 0)
        shared_step = fco::make_step(kKind, *p.lr, *p.steps_done + 1, p.beta1, p.beta2, p.eps, p.weight_decay, p.momentum);
    __syncthreads();
    const fco::Step s = shared_step;
    const bool with_m = kKind == fco::kAdam || p.moment1 != nullptr;
    const int t = threadIdx.x;
    for (int64_t c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const gfold::Chunk ch = p.chunks[c];
        const gfold::Segment sg = p.segments[ch.segment];
        const int32_t uses = p.uses[ch.segment];
        if (uses == 0) continue;
        const int64_t at = sg.offset + ch.first;
        const float* slot0 = p.staging + sg.slot_base + ch.first;
        float* w = p.weights + at;
        float* g_out = p.grads + at;
        float* m = with_m ? p.moment1 + at : nullptr;
        float* v = kKind == fco::kAdam ? p.moment2 + at : nullptr;
        int scalar_from = 0;
        if (p.bases_aligned && gfold::segment_vector(sg)) {
            const int quads = ch.count / 4;
            scalar_from = quads * 4;
            if (t < quads) {
                float4 g = reinterpret_cast<const float4*>(slot0)[t];
                for (int32_t k = 1; k < uses; ++k) {
                    const float4 a = reinterpret_cast<const float4*>(slot0 + k * sg.slot_stride)[t];
                    g.x = g.x + a.x;
                    g.y = g.y + a.y;
                    g.z = g.z + a.z;
                    g.w = g.w + a.w;
                }
                reinterpret_cast<float4*>(g_out)[t] = g;
                float4 w4 = reinterpret_cast<float4*>(w)[t];
                float4 m4 = with_m ? reinterpret_cast<float4*>(m)[t] : float4{};
                float4 v4 = kKind == fco::kAdam ? reinterpret_cast<float4*>(v)[t] : float4{};
                if (with_m) {        // (two spellings: a pointer chosen at run time would put the float4 into scratch)
                    gfold::apply_element<kKind>(s, g.x, &w4.x, &m4.x, &v4.x);
                    gfold::apply_element<kKind>(s, g.y, &w4.y, &m4.y, &v4.y);
                    gfold::apply_element<kKind>(s, g.z, &w4.z, &m4.z, &v4.z);
                    gfold::apply_element<kKind>(s, g.w, &w4.w, &m4.w, &v4.w);
                } else {
                    gfold::apply_element<kKind>(s, g.x, &w4.x, nullptr, nullptr);
                    gfold::apply_element<kKind>(s, g.y, &w4.y, nullptr, nullptr);
                    gfold::apply_element<kKind>(s, g.z, &w4.z, nullptr, nullptr);
                    gfold::apply_element<kKind>(s, g.w, &w4.w, nullptr, nullptr);
                }
                reinterpret_cast<float4*>(w)[t] = w4;
                if (with_m) reinterpret_cast<float4*>(m)[t] = m4;
                if (kKind == fco::kAdam) reinterpret_cast<float4*>(v)[t] = v4;
            }
        }
        for (int i = scalar_from + t; i < ch.count; i += gfold::kThreads) {
            const float g = gfold::fold_slots(slot0 + i, sg.slot_stride, uses);
            g_out[i] = g;
            float w1 = w[i];
            float m1 = with_m ? m[i] : 0.f;
            float v1 = kKind == fco::kAdam ? v[i] : 0.f;
            if (with_m)
                gfold::apply_element<kKind>(s, g, &w1, &m1, &v1);
            else
                gfold::apply_element<kKind>(s, g, &w1, nullptr, nullptr);
            w[i] = w1;
            if (with_m) m[i] = m1;
            if (kKind == fco::kAdam) v[i] = v1;
        }
    }
}

int refuse(const char* entry, const std::string& msg) {
    return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg);
}

int check_list(const char* entry, const mztrain_fold_segment* segments, int32_t n_segments, int64_t n, int64_t staging_floats) {
    int32_t at = -1;
    const char* why = gfold::check_segments(reinterpret_cast<const gfold::Segment*>(segments), n_segments, n, staging_floats, &at);
    if (!why) return MZMCTS_OK;
    return refuse(entry, std::string(why) + (at >= 0 ? " (segment " + std::to_string(at) + ")" : ""));
}

int check_step_args(const char* entry, const mztrain_fold_args* a, int64_t n, int64_t staging_floats) {
    if (!a) return refuse(entry, "null args");
    const int rc = fco::check_opt_args(entry, &a->opt);
    if (rc != MZMCTS_OK) return rc;
    if (!a->staging) return refuse(entry, "null pointer in args (staging)");
    if (a->opt.n != n) return refuse(entry, "opt.n is not the flat buffers' size the segments were checked against");
    if (a->staging_floats < staging_floats) return refuse(entry, "staging_floats below what the segments were checked against");
    return MZMCTS_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int mztrain_fold_create(const mztrain_fold_segment* segments, int32_t n_segments, int64_t n, int64_t staging_floats,
                        int32_t device, mztrain_fold** out) {
    if (!out) return refuse("mztrain_fold_create", "null out");
    *out = nullptr;
    const int rc = check_list("mztrain_fold_create", segments, n_segments, n, staging_floats);
    if (rc != MZMCTS_OK) return rc;
    auto* h = new mztrain_fold;
    h->n_segments = n_segments;
    h->n = n;
    h->staging_floats = staging_floats;
    const auto* seg = reinterpret_cast<const gfold::Segment*>(segments);
    h->segments.assign(seg, seg + n_segments);
    h->uses.assign(n_segments, 0);
    h->plan = gfold::plan_fold(seg, n_segments);
    std::vector<gfold::Chunk> chunks(h->plan.chunks);
    gfold::fill_chunks(seg, n_segments, chunks.data());
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&h->d_segments), sizeof(gfold::Segment) * n_segments);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&h->d_chunks), sizeof(gfold::Chunk) * chunks.size());
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&h->d_uses), sizeof(int32_t) * n_segments);
    if (err == hipSuccess)
        err = hipMemcpy(h->d_segments, seg, sizeof(gfold::Segment) * n_segments, hipMemcpyHostToDevice);
    if (err == hipSuccess)
        err = hipMemcpy(h->d_chunks, chunks.data(), sizeof(gfold::Chunk) * chunks.size(), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(h->d_uses, 0, sizeof(int32_t) * n_segments);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) {
        mztrain_fold_destroy(h);
        return hip_fail(nullptr, err, "mztrain_fold_create");
    }
    *out = h;
    return MZMCTS_OK;
}

void mztrain_fold_destroy(mztrain_fold* h) {
    if (!h) return;
    if (h->d_segments) (void)hipFree(h->d_segments);
    if (h->d_chunks) (void)hipFree(h->d_chunks);
    if (h->d_uses) (void)hipFree(h->d_uses);
    delete h;
}

int mztrain_fold_set_uses(mztrain_fold* h, const int32_t* uses, int32_t n_segments) {
    if (!h) return refuse("mztrain_fold_set_uses", "null handle");
    if (n_segments != h->n_segments) return refuse("mztrain_fold_set_uses", "n_segments is not the handle's");
    int32_t at = -1;
    if (const char* why = gfold::check_uses(h->segments.data(), uses, n_segments, &at))
        return refuse("mztrain_fold_set_uses", std::string(why) + (at >= 0 ? " (segment " + std::to_string(at) + ")" : ""));
    // every step queued so far has read the old values before the new ones land
    MZ_HIP(nullptr, hipDeviceSynchronize());
    MZ_HIP(nullptr, hipMemcpy(h->d_uses, uses, sizeof(int32_t) * n_segments, hipMemcpyHostToDevice));
    MZ_HIP(nullptr, hipDeviceSynchronize());
    h->uses.assign(uses, uses + n_segments);
    h->uses_set = true;
    return MZMCTS_OK;
}

int mztrain_fold_step(mztrain_fold* h, const mztrain_fold_args* a, void* stream_) {
    if (!h) return refuse("mztrain_fold_step", "null handle");
    const int rc = check_step_args("mztrain_fold_step", a, h->n, h->staging_floats);
    if (rc != MZMCTS_OK) return rc;
    if (!h->uses_set) return refuse("mztrain_fold_step", "mztrain_fold_set_uses has not been called");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const mztrain_opt_args& o = a->opt;
    const bool adam = o.kind == MZTRAIN_OPT_ADAM;
    FoldParams p{h->d_segments, h->d_uses, h->d_chunks, h->plan.chunks, a->staging, o.weights, const_cast<float*>(o.grads),
                 nullptr, nullptr, o.lr, o.steps_done, o.beta1, o.beta2, o.eps, o.weight_decay, o.momentum, 0};
    if (adam) {
        p.moment1 = o.moment1;
        p.moment2 = o.moment2;
    } else if (o.momentum != 0.0) {
        p.moment1 = o.moment1;       // (momentum 0: the kernel never sees the buffer)
    }
    p.bases_aligned = aligned16(p.weights) && aligned16(p.grads) && aligned16(p.staging) && aligned16(p.moment1) &&
                      aligned16(p.moment2);
    const dim3 grid(h->plan.grid), block(h->plan.block);
    if (adam)
        grad_fold_kernel<fco::kAdam><<<grid, block, 0, stream>>>(p);
    else
        grad_fold_kernel<fco::kSgd><<<grid, block, 0, stream>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    return fco::queue_advance(o.steps_done, stream_);
}

int mztrain_fold_reference(const mztrain_fold_segment* segments, const int32_t* uses, int32_t n_segments,
                           const mztrain_fold_args* a) {
    const char* entry = "mztrain_fold_reference";
    if (!a) return refuse(entry, "null args");
    int rc = check_list(entry, segments, n_segments, a->opt.n, a->staging_floats);
    if (rc != MZMCTS_OK) return rc;
    const auto* seg = reinterpret_cast<const gfold::Segment*>(segments);
    int32_t at = -1;
    if (const char* why = gfold::check_uses(seg, uses, n_segments, &at))
        return refuse(entry, std::string(why) + (at >= 0 ? " (segment " + std::to_string(at) + ")" : ""));
    rc = check_step_args(entry, a, a->opt.n, a->staging_floats);
    if (rc != MZMCTS_OK) return rc;
    const mztrain_opt_args& o = a->opt;
    gfold::reference_step(o.kind == MZTRAIN_OPT_ADAM ? fco::kAdam : fco::kSgd, seg, uses, n_segments, a->staging, o.weights,
                          const_cast<float*>(o.grads), o.moment1, o.moment2, *o.lr, *o.steps_done + 1, o.beta1, o.beta2, o.eps,
                          o.weight_decay, o.momentum);
    *o.steps_done += 1;
    return MZMCTS_OK;
}

int mztrain_fold_plan(const mztrain_fold_segment* segments, int32_t n_segments, int64_t n, int64_t staging_floats,
                      int64_t* out, int64_t* chunks, int64_t max_chunks) {
    if (out) out[0] = out[1] = out[2] = out[3] = 0;
    if (!out) return refuse("mztrain_fold_plan", "null out");
    const int rc = check_list("mztrain_fold_plan", segments, n_segments, n, staging_floats);
    if (rc != MZMCTS_OK) return rc;
    const auto* seg = reinterpret_cast<const gfold::Segment*>(segments);
    const gfold::FoldPlan plan = gfold::plan_fold(seg, n_segments);
    out[0] = plan.chunks;
    out[1] = plan.grid;
    out[2] = plan.block;
    out[3] = gfold::kChunk;
    if (chunks) {
        if (max_chunks < plan.chunks) return refuse("mztrain_fold_plan", "max_chunks below the plan's chunks");
        std::vector<gfold::Chunk> table(plan.chunks);
        gfold::fill_chunks(seg, n_segments, table.data());
        for (int64_t c = 0; c < plan.chunks; ++c) {
            chunks[4 * c + 0] = table[c].segment;
            chunks[4 * c + 1] = table[c].first;
            chunks[4 * c + 2] = table[c].count;
            chunks[4 * c + 3] = gfold::segment_vector(seg[table[c].segment]) ? 1 : 0;
        }
    }
    return MZMCTS_OK;
}

}  // extern "C"
