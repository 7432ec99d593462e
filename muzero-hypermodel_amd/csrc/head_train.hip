// head_train.hip -- the reward / value / policy heads of a residual network in training as HIP launches (include/mztrain.h
// mztrain_heads_*): the rule and the order of every sum of csrc/head_train.h, whose chains the kernels call as they stand.
//
//   heads_forward_kernel    a workgroup of 256 per sample, every head of the call: the 1 x 1 convolution straight from global
//                           memory (position fastest across lanes: coalesced), its output kept in LDS and written out; fc1 as
//                           four interleaved partial chains per unit (four lanes, 16 contiguous bytes of the weight row),
//                           folded with the bias; ELU; fc2 a chain per logit.  Three barriers, no weight in LDS.
//   heads_backward_kernel   the same workgroup backwards: dpre and dflat through LDS and out to the caller's buffers, then dx
//                           as one chain over (head, reduced channel) per (channel, position); the dx stage is skipped as a
//                           whole where nobody wants it.
//   heads_reduce_kernel     the parameter gradients: a workgroup owns 16 consecutive entries of the call's concatenated
//                           gradients; thread (lane l = tid / 16, entry tid % 16) adds its interleaved terms in float64,
//                           the 16 partials of an entry are folded in ascending l by one thread.  No atomics, no workspace.
// At batch 64 these launches are latency from end to end (a TicTacToe call is under a million multiply-adds): the form spends its
// effort on few launches, few barriers and short dependent chains, not on the matrix cores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "engine_host.h"
#include "head_train.h"

namespace {

namespace hdt = mz::hdt;

static_assert(hdt::kMaxHeads == MZTRAIN_HEADS_MAX, "mztrain.h states the heads of a call");
static_assert(hdt::kEluUlps == MZTRAIN_HEADS_ELU_ULPS, "mztrain.h states the ulp bound");
static_assert(hdt::kMaxBatch == MZTRAIN_HEADS_MAX_BATCH, "mztrain.h states the largest batch");
static_assert(hdt::kBlock == hdt::kReduceLanes * 16, "a reduction workgroup is 16 entries by 16 partials");

struct ForwardParams {
    const float* x;
    hdt::Head heads[hdt::kMaxHeads];
    float* logits[hdt::kMaxHeads];
    float* flat[hdt::kMaxHeads];
    float* pre[hdt::kMaxHeads];
    int n_heads, C, P;
};

struct BackwardParams {
    hdt::Head heads[hdt::kMaxHeads];
    hdt::ReduceHead red[hdt::kMaxHeads];
    float* dpre[hdt::kMaxHeads];
    float* dflat[hdt::kMaxHeads];
    float* dx;
    hdt::ReducePlan plan;
    int64_t batch;
    int n_heads, C, P;
};

// item `idx` of the two heads' items laid end to end (n0 of head 0 first): its head, and its index within the head
__device__ inline int split_head(int idx, int n0, int* within) {
    const int h = idx >= n0 ? 1 : 0;
    *within = idx - h * n0;
    return h;
}

__global__ __launch_bounds__(hdt::kBlock) void heads_forward_kernel(ForwardParams a) {
    __shared__ float s_flat[hdt::kMaxHeads][hdt::kMaxFlat];
    __shared__ float s_part[hdt::kMaxHeads][hdt::kMaxHidden * hdt::kFc1Parts];
    __shared__ float s_h[hdt::kMaxHeads][hdt::kMaxHidden];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int C = a.C, P = a.P;
    const float* xb = a.x + b * C * P;
    const int two = a.n_heads > 1 ? 1 : 0;
    const int n0 = a.heads[0].R * P, n1 = two ? a.heads[1].R * P : 0;
    const int hd0 = a.heads[0].Hd, hd1 = two ? a.heads[1].Hd : 0;
    const int o0 = a.heads[0].O, o1 = two ? a.heads[1].O : 0;

    for (int idx = tid; idx < n0 + n1; idx += hdt::kBlock) {
        int i;
        const int h = split_head(idx, n0, &i);
        const hdt::Head& hd = a.heads[h];
        const int r = i / P, p = i - r * P;
        const float v = hdt::conv_value(xb, hd.conv_w + r * C, hd.conv_b[r], C, P, p);
        s_flat[h][i] = v;
        a.flat[h][b * (hd.R * P) + i] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < (hd0 + hd1) * hdt::kFc1Parts; idx += hdt::kBlock) {
        int i;
        const int h = split_head(idx, hd0 * hdt::kFc1Parts, &i);
        const hdt::Head& hd = a.heads[h];
        const int n = hd.R * P;
        s_part[h][i] = hdt::fc1_part(s_flat[h], hd.fc1_w + static_cast<size_t>(i / hdt::kFc1Parts) * n, n, i % hdt::kFc1Parts);
    }
    __syncthreads();
    for (int idx = tid; idx < hd0 + hd1; idx += hdt::kBlock) {
        int j;
        const int h = split_head(idx, hd0, &j);
        const hdt::Head& hd = a.heads[h];
        const float pre = hdt::fc1_fold(&s_part[h][j * hdt::kFc1Parts], hd.fc1_b[j]);
        a.pre[h][b * hd.Hd + j] = pre;
        s_h[h][j] = hdt::elu(pre);
    }
    __syncthreads();
    for (int idx = tid; idx < o0 + o1; idx += hdt::kBlock) {
        int o;
        const int h = split_head(idx, o0, &o);
        const hdt::Head& hd = a.heads[h];
        a.logits[h][b * hd.O + o] = hdt::fc2_value(s_h[h], hd.fc2_w + static_cast<size_t>(o) * hd.Hd, hd.fc2_b[o], hd.Hd);
    }
}

__global__ __launch_bounds__(hdt::kBlock) void heads_backward_kernel(BackwardParams a) {
    __shared__ float s_dpre[hdt::kMaxHeads][hdt::kMaxHidden];
    __shared__ float s_dflat[hdt::kMaxHeads][hdt::kMaxFlat];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int C = a.C, P = a.P;
    const int two = a.n_heads > 1 ? 1 : 0;
    const int n0 = a.heads[0].R * P, n1 = two ? a.heads[1].R * P : 0;
    const int hd0 = a.heads[0].Hd, hd1 = two ? a.heads[1].Hd : 0;

    for (int idx = tid; idx < hd0 + hd1; idx += hdt::kBlock) {
        int j;
        const int h = split_head(idx, hd0, &j);
        const hdt::Head& hd = a.heads[h];
        const float v = hdt::dh_value(a.red[h].dlogits + b * hd.O, hd.fc2_w, hd.O, hd.Hd, j) *
                        hdt::elu_slope(a.red[h].pre[b * hd.Hd + j]);
        s_dpre[h][j] = v;
        a.dpre[h][b * hd.Hd + j] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < n0 + n1; idx += hdt::kBlock) {
        int i;
        const int h = split_head(idx, n0, &i);
        const hdt::Head& hd = a.heads[h];
        const float v = hdt::dflat_value(s_dpre[h], hd.fc1_w, hd.Hd, hd.R * P, i);
        s_dflat[h][i] = v;
        a.dflat[h][b * (hd.R * P) + i] = v;
    }
    if (!a.dx) return;                                   // uniform over the launch
    __syncthreads();
    const float* rows[hdt::kMaxHeads];
    rows[0] = s_dflat[0];
    rows[1] = s_dflat[1];
    float* dxb = a.dx + b * C * P;
    for (int idx = tid; idx < C * P; idx += hdt::kBlock) {
        const int c = idx / P, p = idx - c * P;
        dxb[idx] = hdt::dx_value(a.heads, a.n_heads, rows, C, P, c, p);
    }
}

__global__ __launch_bounds__(hdt::kBlock) void heads_reduce_kernel(BackwardParams a) {
    __shared__ double s_partial[hdt::kReduceLanes][16];
    const int tid = threadIdx.x;
    const int slot = tid & 15, lane = tid >> 4;
    const int64_t g = static_cast<int64_t>(blockIdx.x) * 16 + slot;
    const int64_t total = a.plan.first[a.plan.segments];
    int seg = 0;
    if (g < total)
        while (g >= a.plan.first[seg + 1]) ++seg;        // (empty segments are stepped over: first[seg + 1] == first[seg] <= g)
    const int head = seg / hdt::kKinds, kind = seg % hdt::kKinds;
    const int64_t e = g - a.plan.first[seg];
    double partial = 0.0;
    if (g < total)
        partial = hdt::reduce_partial(a.red[head], kind, e, hdt::kind_terms(kind, a.batch, a.P), lane, a.C, a.P);
    s_partial[lane][slot] = partial;
    __syncthreads();
    if (tid < 16 && g < total) a.red[head].out[kind][e] = hdt::reduce_fold(&s_partial[0][slot], 16);
}

int refuse(const char* entry, const std::string& msg) {
    return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg);
}

// the shapes of a call's heads, checked; C and P come back
int check_heads(const char* entry, const mzmcts_head_desc* heads, int32_t n_heads, int64_t batch, int* C, int* P) {
    if (n_heads < 1 || n_heads > hdt::kMaxHeads) return refuse(entry, hdt::refusal(1, 1, 1, 1, 1, n_heads));
    for (int h = 0; h < n_heads; ++h) {
        const mzmcts_head_desc& d = heads[h];
        if (!d.conv_w || !d.conv_b || !d.fc1_w || !d.fc1_b || !d.fc2_w || !d.fc2_b) return refuse(entry, "null parameter of a head");
        if (d.channels != heads[0].channels || d.plane != heads[0].plane)
            return refuse(entry, "the heads of a call share channels and plane");
        if (const char* why = hdt::refusal(d.channels, d.plane, d.reduced, d.hidden, d.outputs, n_heads)) return refuse(entry, why);
    }
    if (batch < 1 || batch > hdt::kMaxBatch) return refuse(entry, "batch must lie in [1, 65536]");
    *C = heads[0].channels;
    *P = heads[0].plane;
    return MZMCTS_OK;
}

hdt::Head head_of(const mzmcts_head_desc& d) {
    return hdt::Head{d.conv_w, d.conv_b, d.fc1_w, d.fc1_b, d.fc2_w, d.fc2_b, d.reduced, d.hidden, d.outputs};
}

int fill_forward(const char* entry, const mztrain_heads_forward_args* a, ForwardParams* p) {
    if (!a) return refuse(entry, "null args");
    const int rc = check_heads(entry, a->heads, a->n_heads, a->batch, &p->C, &p->P);
    if (rc != MZMCTS_OK) return rc;
    if (!a->x) return refuse(entry, "null x");
    p->x = a->x;
    p->n_heads = a->n_heads;
    for (int h = 0; h < a->n_heads; ++h) {
        if (!a->logits[h] || !a->flat[h] || !a->pre[h]) return refuse(entry, "null logits, flat or pre of a head");
        p->heads[h] = head_of(a->heads[h]);
        p->logits[h] = a->logits[h], p->flat[h] = a->flat[h], p->pre[h] = a->pre[h];
    }
    return MZMCTS_OK;
}

int fill_backward(const char* entry, const mztrain_heads_backward_args* a, BackwardParams* p) {
    if (!a) return refuse(entry, "null args");
    const int rc = check_heads(entry, a->heads, a->n_heads, a->batch, &p->C, &p->P);
    if (rc != MZMCTS_OK) return rc;
    if (!a->x) return refuse(entry, "null x");
    p->n_heads = a->n_heads;
    p->batch = a->batch;
    p->dx = a->dx;
    for (int h = 0; h < a->n_heads; ++h) {
        if (!a->dlogits[h] || !a->flat[h] || !a->pre[h] || !a->dpre[h] || !a->dflat[h])
            return refuse(entry, "null dlogits, flat, pre, dpre or dflat of a head");
        p->heads[h] = head_of(a->heads[h]);
        p->dpre[h] = a->dpre[h], p->dflat[h] = a->dflat[h];
        const mztrain_heads_grads& g = a->grads[h];
        p->red[h] = hdt::ReduceHead{a->x, a->flat[h], a->pre[h], a->dlogits[h], a->dpre[h], a->dflat[h],
                                    {g.conv_w, g.conv_b, g.fc1_w, g.fc1_b, g.fc2_w, g.fc2_b},
                                    a->heads[h].reduced, a->heads[h].hidden, a->heads[h].outputs};
    }
    p->plan = hdt::plan_reduce(p->red, p->n_heads, p->C, p->P);
    return MZMCTS_OK;
}

}  // namespace

extern "C" {

int mztrain_heads_supported(int32_t channels, int32_t plane, int32_t reduced, int32_t hidden, int32_t outputs, int32_t n_heads) {
    const char* why = hdt::refusal(channels, plane, reduced, hidden, outputs, n_heads);
    if (why) refuse("mztrain_heads_supported", why);
    return why ? 0 : 1;
}

int mztrain_heads_forward(const mztrain_heads_forward_args* a, void* stream_) {
    ForwardParams p{};
    const int rc = fill_forward("mztrain_heads_forward", a, &p);
    if (rc != MZMCTS_OK) return rc;
    heads_forward_kernel<<<dim3(static_cast<unsigned>(a->batch)), dim3(hdt::kBlock), 0, static_cast<hipStream_t>(stream_)>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_heads_backward(const mztrain_heads_backward_args* a, void* stream_) {
    BackwardParams p{};
    const int rc = fill_backward("mztrain_heads_backward", a, &p);
    if (rc != MZMCTS_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    heads_backward_kernel<<<dim3(static_cast<unsigned>(a->batch)), dim3(hdt::kBlock), 0, stream>>>(p);
    MZ_HIP(nullptr, hipGetLastError());
    const int64_t total = p.plan.first[p.plan.segments];
    if (total > 0) {
        heads_reduce_kernel<<<dim3(static_cast<unsigned>(mz::ceil_div(total, 16))), dim3(hdt::kBlock), 0, stream>>>(p);
        MZ_HIP(nullptr, hipGetLastError());
    }
    return MZMCTS_OK;
}

int mztrain_heads_reference_forward(const mztrain_heads_forward_args* a) {
    ForwardParams p{};
    const int rc = fill_forward("mztrain_heads_reference_forward", a, &p);
    if (rc != MZMCTS_OK) return rc;
    hdt::reference_forward(p.x, p.heads, p.n_heads, p.logits, p.flat, p.pre, a->batch, p.C, p.P);
    return MZMCTS_OK;
}

int mztrain_heads_reference_backward(const mztrain_heads_backward_args* a) {
    BackwardParams p{};
    const int rc = fill_backward("mztrain_heads_reference_backward", a, &p);
    if (rc != MZMCTS_OK) return rc;
    hdt::reference_backward(p.heads, p.red, p.n_heads, p.dpre, p.dflat, p.dx, a->batch, p.C, p.P);
    return MZMCTS_OK;
}

}  // extern "C"
