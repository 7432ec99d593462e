// fc_train.hip -- one training step of a MuZeroFullyConnectedNetwork as four launches (include/mztrain.h mztrain_fc_*).
//
//   fc_train_forward_kernel   a lane group of 16 owns a sample and walks its K1 positions with fc_initial<16> /
//                             fc_recurrent<16> (fc_net_device.h, what the search runs) on an FcNet whose hidden layers each
//                             have a scratch region of their own, so that after a position the scratch holds every
//                             layer's input; the scratch, plus the rescale's min index, max index and scale, is the
//                             position's record in the activation workspace.  Logits go out step-major for the loss launch.
//   mztrain_unroll_loss       trainer_kernels.hip, untouched
//   fc_train_backward_kernel  the same lane group walks k = K1-1 .. 0 with csrc/fc_backward.h: the gradient of every layer's
//                             pre-activation, into the delta workspace (the activation record's layout)
//   fc_train_wgrad_kernel     a workgroup per (weight row, 16 inputs incl. the bias): 16 slices of the positions, each summed
//                             in order in float64 (the products are exact), the slices added in order, rounded once
// Weights are staged in LDS once per workgroup (forward and backward), padded as the search pads them.  Rows per workgroup:
// 16, or 8 / 4 where 16 scratches beside the weights would not fit 160 KB; a network that does not fit with 4 is refused.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "engine_host.h"
#include "fc_backward.h"
#include "fc_net_host.h"

namespace {

using mz::FcNet;
namespace fcb = mz::fcb;

constexpr int kGroup = 16;          // lanes per sample
constexpr int kMaxRows = 16;        // samples per workgroup
constexpr int kMaxThreads = kGroup * kMaxRows;
constexpr int kSlices = 16;         // of the positions, in the weight-gradient launch
constexpr int kMaxWgLayers = 5 * mz::kFcMaxLayers;

struct LaneGroup {
    int j;
    __device__ int lane() const { return j; }
    __device__ int width() const { return kGroup; }
    __device__ void fence() const { mz::group_memory_fence(); }
    __device__ float sum(float v) const { return mz::group_sumf<kGroup>(v); }
};

__global__ __launch_bounds__(kMaxThreads) void fc_train_forward_kernel(
    FcNet net, int rows, int B, int K1, const float* __restrict__ weights, const float* __restrict__ observations,
    const int64_t* __restrict__ actions, float* __restrict__ value_logits, float* __restrict__ reward_logits,
    float* __restrict__ policy_logits, float* __restrict__ act, int record_floats) {
    extern __shared__ __attribute__((aligned(16))) float fwd_smem[];   // [padded weights][neuron tables][rows][scratch]
    const int threads = rows * kGroup;
    float* w_lds = fwd_smem;
    mz::NeuronDesc* table = reinterpret_cast<mz::NeuronDesc*>(fwd_smem + ((net.n_weights_lds + 3) & ~3));
    mz::stage_fc_weights(net, weights, w_lds, threadIdx.x, threads);
    __syncthreads();
    mz::build_fc_tables(net, w_lds, table, kGroup, threadIdx.x, threads);
    __syncthreads();
    const int init_entries = mz::phase_list_entries(net.init_pre, net.n_init_pre, kGroup) +
                             mz::phase_list_entries(net.init_post, net.n_init_post, kGroup);
    const int group = threadIdx.x / kGroup, j = threadIdx.x % kGroup;
    const int b = blockIdx.x * rows + group;
    if (b >= B) return;   // (after the last barrier)
    float* scratch = reinterpret_cast<float*>(table + mz::fc_table_entries(net, kGroup)) +
                     static_cast<size_t>(group) * net.scratch_floats;
    mz::fc_clear_scratch<kGroup>(net, scratch, j);
    for (int k = 0; k < K1; ++k) {
        if (k == 0) {
            mz::fc_initial<kGroup>(net, table, w_lds, scratch, observations + static_cast<size_t>(b) * net.obs, j);
        } else {
            const int64_t a = actions[static_cast<size_t>(b) * K1 + k];
            const int action = (a >= 0 && a < net.A) ? static_cast<int>(a) : -1;
            mz::fc_recurrent<kGroup>(net, table + init_entries, w_lds, scratch, scratch + net.off_norm, action, j);
        }
        const size_t row = static_cast<size_t>(k) * B + b;
        for (int i = j; i < net.F; i += kGroup) value_logits[row * net.F + i] = scratch[net.off_value + i];
        if (k > 0)
            for (int i = j; i < net.F; i += kGroup) reward_logits[row * net.F + i] = scratch[net.off_reward + i];
        for (int i = j; i < net.A; i += kGroup) policy_logits[row * net.A + i] = scratch[net.off_policy + i];
        // the rescale's statistics, as unit_rescale forms them; the first index that attains each extreme
        const float* raw = scratch + net.off_raw;
        float mn = INFINITY, mx = -INFINITY;
        for (int i = j; i < net.enc; i += kGroup) {
            mn = fminf(mn, raw[i]);
            mx = fmaxf(mx, raw[i]);
        }
        mn = mz::group_minf<kGroup>(mn);
        mx = mz::group_maxf<kGroup>(mx);
        float at_min = 1e9f, at_max = 1e9f;
        for (int i = j; i < net.enc; i += kGroup) {
            if (raw[i] == mn && at_min > static_cast<float>(i)) at_min = static_cast<float>(i);
            if (raw[i] == mx && at_max > static_cast<float>(i)) at_max = static_cast<float>(i);
        }
        at_min = mz::group_minf<kGroup>(at_min);
        at_max = mz::group_minf<kGroup>(at_max);
        float scale = mx - mn;
        if (scale < 1e-5f) scale += 1e-5f;
        float* record = act + (static_cast<size_t>(b) * K1 + k) * record_floats;
        for (int i = j; i < net.scratch_floats; i += kGroup) record[i] = scratch[i];
        if (j < 4) record[net.scratch_floats + j] = (j == 0) ? at_min : (j == 1) ? at_max : (j == 2) ? scale : 0.f;
        mz::group_memory_fence();
    }
}

__global__ __launch_bounds__(kMaxThreads) void fc_train_backward_kernel(
    FcNet net, fcb::Net rule, int rows, int B, int K1, const float* __restrict__ weights, const float* __restrict__ act,
    float* __restrict__ del, const float* __restrict__ grad_value, const float* __restrict__ grad_reward,
    const float* __restrict__ grad_policy, float inv_batch) {
    extern __shared__ __attribute__((aligned(16))) float bwd_smem[];   // [padded weights][rows][kBuffers][width]
    const int threads = rows * kGroup;
    float* w_lds = bwd_smem;
    mz::stage_fc_weights(net, weights, w_lds, threadIdx.x, threads);
    __syncthreads();
    const int group = threadIdx.x / kGroup;
    const int b = blockIdx.x * rows + group;
    if (b >= B) return;
    float* mine = bwd_smem + ((net.n_weights_lds + 3) & ~3) + static_cast<size_t>(group) * fcb::kBuffers * rule.width;
    fcb::Buffers u;
    u.t0 = mine;
    u.t1 = mine + rule.width;
    u.g_policy = mine + 2 * rule.width;
    u.g_value = mine + 3 * rule.width;
    u.g_reward = mine + 4 * rule.width;
    u.g_hidden = mine + 5 * rule.width;
    const LaneGroup g{static_cast<int>(threadIdx.x % kGroup)};
    fcb::sample_backward(g, rule, w_lds, B, K1, b, act, del, grad_value, grad_reward, grad_policy, inv_batch, u);
}

struct WgLayer {
    int32_t in, out, x_off, y_off, w_dst, b_dst, steps, tiles;   // tiles of 16 over the in + 1 entries of a row
};
struct WgPlan {
    int32_t n_layers;
    WgLayer layer[kMaxWgLayers];
};

__global__ __launch_bounds__(kGroup * kSlices) void fc_train_wgrad_kernel(WgPlan plan, int record_floats, int B, int K1,
                                                                         const float* __restrict__ act,
                                                                         const float* __restrict__ del,
                                                                         float* __restrict__ grads) {
    __shared__ double part[kSlices][kGroup];
    const WgLayer L = plan.layer[blockIdx.y];
    const int row = blockIdx.x / L.tiles, tile = blockIdx.x % L.tiles;
    if (row >= L.out) return;   // (block-uniform)
    const int lane = threadIdx.x % kGroup, slice = threadIdx.x / kGroup;
    const int i = tile * kGroup + lane;
    const bool valid = i <= L.in;
    const int P = B * K1, chunk = (P + kSlices - 1) / kSlices;
    const int p0 = slice * chunk < P ? slice * chunk : P, p1 = p0 + chunk < P ? p0 + chunk : P;
    part[slice][lane] = valid ? fcb::weight_grad_partial(act, del, record_floats, i < L.in ? L.x_off + i : -1, L.y_off + row,
                                                         K1, L.steps, p0, p1)
                              : 0.0;
    __syncthreads();
    if (slice == 0 && valid) {
        double total = part[0][lane];
        for (int s = 1; s < kSlices; ++s) total = total + part[s][lane];
        const float value = static_cast<float>(total);
        if (i < L.in)
            grads[L.w_dst + static_cast<size_t>(row) * L.in + i] = value;
        else
            grads[L.b_dst + row] = value;
    }
}

int phase_entries(const mz::FcPhase* list, int n) {
    int total = 0;
    for (int i = 0; i < n; ++i) total += (list[i].total_out + 4 * kGroup - 1) / (4 * kGroup) * 4 * kGroup;
    return total;
}

int refuse(const std::string& msg) { return fail(nullptr, MZMCTS_ERR_INVALID, msg); }

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

}  // namespace

struct mztrain_fc {
    FcNet net;           // build_fc_net's, every hidden layer on a scratch region of its own
    fcb::Net rule;
    WgPlan plan;
    const float* weights;
    float* grads;
    int32_t max_batch, max_steps, device, support;
    int32_t fwd_rows, bwd_rows;
    size_t fwd_lds, bwd_lds;
    int32_t wgrad_blocks;
    uint8_t* workspace;
    size_t workspace_bytes;
    float *value_logits, *reward_logits, *policy_logits, *grad_value, *grad_reward, *grad_policy, *act, *del;
};

namespace {

// Give every hidden layer its own scratch region (build_fc_net lets the layers of a head take turns on two), so that a
// position's scratch holds all of its layers' inputs at once.  The jobs are visited in the order build_fc_net made them.
void keep_every_activation(FcNet* net) {
    auto pad4 = [](int v) { return (v + 3) / 4 * 4; };
    int off = net->off_policy + pad4(net->A);
    const mz::FcMlp* mlps[5] = {&net->repr, &net->dyn, &net->reward, &net->policy, &net->value};
    int hidden[5][mz::kFcMaxLayers] = {};
    for (int m = 0; m < 5; ++m)
        for (int l = 0; l + 1 < mlps[m]->n_layers; ++l) {
            hidden[m][l] = off;
            off += pad4(mlps[m]->layer[l].out);
        }
    net->scratch_floats = std::max(off, 64);
    auto place = [&](mz::FcJob* jb, int m, int l, int x_first, int y_last) {
        jb->x_off = (l == 0) ? x_first : hidden[m][l - 1];
        jb->y_off = (l == mlps[m]->n_layers - 1) ? y_last : hidden[m][l];
    };
    struct Head {
        int m, x_first, y_last;
    };
    auto chain = [&](mz::FcPhase* phases, int m) {
        for (int l = 0; l < mlps[m]->n_layers; ++l) place(&phases[l].job[0], m, l, 0, net->off_raw);
    };
    auto heads = [&](mz::FcPhase* phases, int depth, std::initializer_list<Head> hs) {
        for (int l = 0; l < depth; ++l) {
            int at = 0;
            for (const Head& h : hs)
                if (l < mlps[h.m]->n_layers) place(&phases[l].job[at++], h.m, l, h.x_first, h.y_last);
        }
    };
    chain(net->init_pre, 0);
    heads(net->init_post, net->n_init_post, {{3, net->off_norm, net->off_policy}, {4, net->off_norm, net->off_value}});
    chain(net->rec_pre, 1);
    heads(net->rec_post, net->n_rec_post,
          {{2, net->off_raw, net->off_reward}, {3, net->off_norm, net->off_policy}, {4, net->off_norm, net->off_value}});
}

// The backward's view of the same network: weights in the staged (padded) layout, vectors at their record offsets.
void describe_rule(const FcNet& net, fcb::Net* rule, WgPlan* plan) {
    auto pad4 = [](int v) { return (v + 3) / 4 * 4; };
    const mz::FcMlp* mlps[5] = {&net.repr, &net.dyn, &net.reward, &net.policy, &net.value};
    fcb::Mlp* out[5] = {&rule->repr, &rule->dyn, &rule->reward, &rule->policy, &rule->value};
    const mz::FcPhase* phases[5] = {net.init_pre, net.rec_pre, net.rec_post, net.rec_post, net.rec_post};
    const int steps[5] = {fcb::kStepZero, fcb::kStepsAfterZero, fcb::kStepsAfterZero, fcb::kStepsAll, fcb::kStepsAll};
    rule->obs = net.obs;
    rule->enc = net.enc;
    rule->A = net.A;
    rule->F = net.F;
    rule->off_raw = net.off_raw;
    rule->off_norm = net.off_norm;
    rule->off_stats = net.scratch_floats;
    rule->record_floats = net.scratch_floats + 4;
    int width = std::max({net.obs, net.enc + net.A, net.F});
    plan->n_layers = 0;
    for (int m = 0; m < 5; ++m) {
        out[m]->n_layers = mlps[m]->n_layers;
        for (int l = 0; l < mlps[m]->n_layers; ++l) {
            const mz::FcLayer& L = mlps[m]->layer[l];
            // the job of (m, l): the chains hold one job per phase; in rec_post the heads present at depth l come in the
            // order reward, policy, value
            int at = 0;
            if (m >= 2)
                for (int before = 2; before < m; ++before) at += (l < mlps[before]->n_layers) ? 1 : 0;
            const mz::FcJob& jb = phases[m][l].job[at];
            fcb::Layer& R = out[m]->layer[l];
            R.in = L.in;
            R.out = L.out;
            R.ld = L.in_pad;
            R.w = L.w_lds;
            R.b = L.b_lds;
            R.x_off = jb.x_off;
            R.y_off = jb.y_off;
            width = std::max({width, static_cast<int>(L.in), static_cast<int>(L.out)});
            WgLayer& W = plan->layer[plan->n_layers++];
            W = WgLayer{L.in, L.out, jb.x_off, jb.y_off, L.w_off, L.b_off, steps[m], (L.in + 1 + kGroup - 1) / kGroup};
        }
    }
    rule->width = pad4(width);
}

size_t forward_lds(const FcNet& net, int rows) {
    const int entries = phase_entries(net.init_pre, net.n_init_pre) + phase_entries(net.init_post, net.n_init_post) +
                        phase_entries(net.rec_pre, net.n_rec_pre) + phase_entries(net.rec_post, net.n_rec_post);
    return sizeof(float) * (static_cast<size_t>((net.n_weights_lds + 3) & ~3) + static_cast<size_t>(net.scratch_floats) * rows) +
           sizeof(mz::NeuronDesc) * static_cast<size_t>(entries);
}

size_t backward_lds(const FcNet& net, const fcb::Net& rule, int rows) {
    return sizeof(float) * (static_cast<size_t>((net.n_weights_lds + 3) & ~3) +
                            static_cast<size_t>(rows) * fcb::kBuffers * rule.width);
}

template <class Bytes>
int rows_that_fit(Bytes bytes) {
    for (int rows = kMaxRows; rows >= 4; rows /= 2)
        if (bytes(rows) <= kLdsPerWorkgroup) return rows;
    return 0;
}

}  // namespace

extern "C" {

int mztrain_fc_create(const mzmcts_fc_desc* desc, int32_t actions, int32_t support_size, const float* weights,
                      int64_t n_weights, float* grads, int32_t max_batch, int32_t max_steps, int32_t device,
                      mztrain_fc** out) {
    if (!desc || !weights || !grads || !out) return refuse("mztrain_fc_create: null argument");
    *out = nullptr;
    if (actions <= 0 || max_batch <= 0 || max_steps <= 0)
        return refuse("mztrain_fc_create: actions, max_batch and max_steps must be positive");
    if (support_size < 1 || 2 * static_cast<int64_t>(support_size) + 1 > mz::kFcMaxWidth || actions > mz::kFcMaxWidth)
        return refuse(std::string("mztrain_fc_create: ") + mz::kFcNetSizesMessage);
    mztrain_fc h{};
    const int rc = mz::build_fc_net(desc, actions, support_size, n_weights, &h.net);
    if (rc == mz::kFcNetSizes) return refuse(std::string("mztrain_fc_create: ") + mz::kFcNetSizesMessage);
    if (rc == mz::kFcNetWeightCount) return refuse(std::string("mztrain_fc_create: ") + mz::kFcNetWeightCountMessage);
    keep_every_activation(&h.net);
    describe_rule(h.net, &h.rule, &h.plan);
    h.fwd_rows = rows_that_fit([&](int rows) { return forward_lds(h.net, rows); });
    h.bwd_rows = rows_that_fit([&](int rows) { return backward_lds(h.net, h.rule, rows); });
    if (h.fwd_rows == 0 || h.bwd_rows == 0)
        return refuse("mztrain_fc_create: the network's weights and activations do not fit a workgroup's 160 KB of LDS");
    // the kernels count positions p = b * K1 + k in int32
    if (static_cast<int64_t>(max_batch) * max_steps > INT32_MAX)
        return refuse("mztrain_fc_create: max_batch * max_steps does not fit int32 (positions are counted in int32)");
    h.fwd_lds = forward_lds(h.net, h.fwd_rows);
    h.bwd_lds = backward_lds(h.net, h.rule, h.bwd_rows);
    h.weights = weights;
    h.grads = grads;
    h.max_batch = max_batch;
    h.max_steps = max_steps;
    h.device = device;
    h.support = support_size;
    h.wgrad_blocks = 0;
    for (int l = 0; l < h.plan.n_layers; ++l)
        h.wgrad_blocks = std::max(h.wgrad_blocks, h.plan.layer[l].out * h.plan.layer[l].tiles);
    // one block of device memory: logits and their gradients (step-major), the activation and delta records, each on
    // a 256-byte boundary, between two guard bands
    const size_t positions = static_cast<size_t>(max_batch) * max_steps;
    const size_t sizes[8] = {positions * h.net.F, positions * h.net.F, positions * h.net.A, positions * h.net.F,
                             positions * h.net.F, positions * h.net.A, positions * h.rule.record_floats,
                             positions * h.rule.record_floats};
    constexpr size_t kGuard = 256;   // bytes before and after, left as the 0xff every byte starts with
    size_t offsets[8], total = kGuard;
    for (int i = 0; i < 8; ++i) {
        offsets[i] = total;
        total += round_up(sizes[i] * sizeof(float), 256);
    }
    MZ_HIP(nullptr, hipSetDevice(device));
    MZ_HIP(nullptr, hipFuncSetAttribute(reinterpret_cast<const void*>(fc_train_forward_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsPerWorkgroup)));
    MZ_HIP(nullptr, hipFuncSetAttribute(reinterpret_cast<const void*>(fc_train_backward_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsPerWorkgroup)));
    total += kGuard;
    MZ_HIP(nullptr, hipMalloc(reinterpret_cast<void**>(&h.workspace), total));
    if (hipMemset(h.workspace, 0xff, total) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(h.workspace);
        return fail(nullptr, MZMCTS_ERR_HIP, "mztrain_fc_create: clearing the workspace failed");
    }
    h.workspace_bytes = total;
    float** slots[8] = {&h.value_logits, &h.reward_logits, &h.policy_logits, &h.grad_value,
                        &h.grad_reward,  &h.grad_policy,   &h.act,           &h.del};
    for (int i = 0; i < 8; ++i) *slots[i] = reinterpret_cast<float*>(h.workspace + offsets[i]);
    *out = new mztrain_fc(h);
    return MZMCTS_OK;
}

void mztrain_fc_destroy(mztrain_fc* handle) {
    if (!handle) return;
    if (handle->workspace) (void)hipFree(handle->workspace);
    delete handle;
}

int64_t mztrain_fc_workspace_bytes(const mztrain_fc* handle) {
    return handle ? static_cast<int64_t>(handle->workspace_bytes) : -1;
}

int mztrain_fc_logits(const mztrain_fc* handle, const float** value_logits, const float** reward_logits,
                      const float** policy_logits) {
    if (!handle || !value_logits || !reward_logits || !policy_logits) return refuse("mztrain_fc_logits: null argument");
    *value_logits = handle->value_logits;
    *reward_logits = handle->reward_logits;
    *policy_logits = handle->policy_logits;
    return MZMCTS_OK;
}

int mztrain_fc_step(mztrain_fc* h, const mztrain_fc_args* a, void* stream_) {
    if (!a) return refuse("mztrain_fc_step: null args");
    if (!a->observations || !a->actions || !a->target_value || !a->target_reward || !a->target_policy || !a->gradient_scale ||
        !a->sample_loss || !a->head_sums || !a->priorities)
        return refuse("mztrain_fc_step: null pointer in args (weight alone may be null)");
    if (a->batch <= 0 || a->steps <= 0) return refuse("mztrain_fc_step: batch and steps must be positive");
    if (!h) return refuse("mztrain_fc_step: null handle");
    if (a->batch > h->max_batch || a->steps > h->max_steps)
        return refuse("mztrain_fc_step: batch or steps above the maxima the handle was created with");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int B = a->batch, K1 = a->steps;
    fc_train_forward_kernel<<<dim3((B + h->fwd_rows - 1) / h->fwd_rows), dim3(h->fwd_rows * kGroup), h->fwd_lds, stream>>>(
        h->net, h->fwd_rows, B, K1, h->weights, a->observations, a->actions, h->value_logits, h->reward_logits,
        h->policy_logits, h->act, h->rule.record_floats);
    MZ_HIP(nullptr, hipGetLastError());
    mztrain_loss_args loss{};
    loss.value_logits = h->value_logits;
    loss.reward_logits = h->reward_logits;
    loss.policy_logits = h->policy_logits;
    loss.target_value = a->target_value;
    loss.target_reward = a->target_reward;
    loss.target_policy = a->target_policy;
    loss.gradient_scale = a->gradient_scale;
    loss.weight = a->weight;
    loss.batch = B;
    loss.steps = K1;
    loss.support_size = h->support;
    loss.actions = h->net.A;
    loss.value_loss_weight = a->value_loss_weight;
    loss.per_alpha = a->per_alpha;
    loss.sample_loss = a->sample_loss;
    loss.head_sums = a->head_sums;
    loss.priorities = a->priorities;
    loss.grad_value = h->grad_value;
    loss.grad_reward = h->grad_reward;
    loss.grad_policy = h->grad_policy;
    const int rc = mztrain_unroll_loss(&loss, stream_);
    if (rc != MZMCTS_OK) return fail(nullptr, rc, "mztrain_fc_step: the loss launch failed");
    fc_train_backward_kernel<<<dim3((B + h->bwd_rows - 1) / h->bwd_rows), dim3(h->bwd_rows * kGroup), h->bwd_lds, stream>>>(
        h->net, h->rule, h->bwd_rows, B, K1, h->weights, h->act, h->del, h->grad_value, h->grad_reward, h->grad_policy,
        1.0f / static_cast<float>(B));
    MZ_HIP(nullptr, hipGetLastError());
    fc_train_wgrad_kernel<<<dim3(h->wgrad_blocks, h->plan.n_layers), dim3(kGroup * kSlices), 0, stream>>>(
        h->plan, h->rule.record_floats, B, K1, h->act, h->del, h->grads);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

}  // extern "C"
