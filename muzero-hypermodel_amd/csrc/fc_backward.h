// fc_backward.h -- the backward rule of one training step of a MuZeroFullyConnectedNetwork (Trainer._unroll, the loss
// wrapper and loss.mean() are the specification), written once for the HIP kernels of fc_train.hip and for a host
// compiler (tests/fc_backward_check.cpp).  No HIP include: the lane group is a policy object (lane, width, fence, sum), a
// host build walks everything with the one-lane Serial group.
//
// A POSITION is one (sample b, unroll step k); position p = b * K1 + k owns one record of `record_floats` floats in the
// activation workspace and one in the delta workspace, both in the forward's scratch layout:
//   activations  every layer's input vector at x_off (the ELU output of the layer before, the observation, the hidden state
//                and one-hot action, the normalised / raw state), the raw state at off_raw, the normalised one at
//                off_norm, and at off_stats the rescale's min index, max index and scale
//   deltas       the gradient of every layer's pre-activation at that layer's y_off
// The rule, per position, k = K1-1 .. 0:
//   delta at the logits = the loss launch's gradient * (1 / B)                       (loss.mean(); `gv * g` in the wrapper)
//   Linear: g_x[i] = sum_j W[j][i] delta[j], j ascending; ELU' = 1 for y > 0, else y + 1 with y the saved expf(x) - 1
//   policy and value read the normalised state, the reward head the raw one
//   the hidden state of a recurrent step passes on HALF of its whole gradient (policy + value heads of the step, dynamics
//   of the next step); the initial hidden state has no hook
//   rescale norm = (raw - min) / scale, scale = max - min (+ 1e-5 below 1e-5: the addition passes the gradient through):
//   g_raw[i] = g[i] / scale, the first index attaining max gets d_scale = -sum(g * norm) / scale, the first attaining min
//   -sum(g) / scale - d_scale; the same index for both: the scale terms cancel
//   the dynamics' input gradient (first `enc` inputs) is what the position before receives; the one-hot part is dropped
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
namespace fcb {

constexpr int kMaxLayers = 4;    // Linear layers per MLP (fc_net_device.h kFcMaxLayers)
constexpr int kBuffers = 6;      // temporaries of `width` floats a group needs (Buffers below)

struct Layer {
    int32_t in, out;
    int32_t ld;            // floats between two weight rows in the array the walk reads
    int32_t w, b;          // offsets of the weight rows / the bias in that array
    int32_t x_off, y_off;  // record offsets of the input vector / of the pre-activation's delta
};
struct Mlp {
    int32_t n_layers;
    Layer layer[kMaxLayers];
};
struct Net {
    int32_t obs, enc, A, F;
    int32_t off_raw, off_norm, off_stats;   // record offsets; stats = {min index, max index, scale} as floats
    int32_t record_floats;
    int32_t width;                          // widest vector of the network, rounded up to 4
    Mlp repr, dyn, reward, policy, value;
};

struct Serial {
    MZ_HD int lane() const { return 0; }
    MZ_HD int width() const { return 1; }
    MZ_HD void fence() const {}
    MZ_HD float sum(float v) const { return v; }
};

struct Buffers {
    float *t0, *t1;     // delta of the layer being walked, and of the one below
    float *g_policy;    // input gradients of the heads (enc)
    float *g_value;
    float *g_reward;
    float *g_hidden;    // gradient the next position's dynamics sent to this position's hidden state (enc)
};

MZ_HD inline float elu_slope(float y) { return y > 0.f ? 1.f : y + 1.f; }

// g_x[i] = sum_j W[j][i] * delta[j] for the first `count` inputs of a layer, one lane per input, j ascending
template <class Group>
MZ_HD inline void linear_input_grad(const Group& g, const Layer& L, const float* w, const float* delta, float* gx, int count) {
    for (int i = g.lane(); i < count; i += g.width()) {
        const float* column = w + L.w + i;
        float acc = 0.f;
        for (int j = 0; j < L.out; ++j) acc = acc + column[static_cast<size_t>(j) * L.ld] * delta[j];
        gx[i] = acc;
    }
}

// `cur` holds the delta of the MLP's last layer.  Leaves every layer's delta in the record `del`; with gin_count > 0 the
// gradient of the first gin_count inputs of the MLP in `gin`.  cur / nxt are clobbered.
template <class Group>
MZ_HD inline void mlp_backward(const Group& g, const Mlp& m, const float* w, const float* act, float* del, float* cur,
                               float* nxt, float* gin, int gin_count) {
    for (int l = m.n_layers - 1; l >= 0; --l) {
        const Layer& L = m.layer[l];
        for (int i = g.lane(); i < L.out; i += g.width()) del[L.y_off + i] = cur[i];
        if (l == 0) {
            if (gin_count > 0) linear_input_grad(g, L, w, cur, gin, gin_count);
            g.fence();
            return;
        }
        linear_input_grad(g, L, w, cur, nxt, L.in);
        for (int i = g.lane(); i < L.in; i += g.width()) nxt[i] = nxt[i] * elu_slope(act[L.x_off + i]);
        g.fence();
        float* swap = cur;
        cur = nxt;
        nxt = swap;
    }
}

template <class Group>
MZ_HD inline void scaled_copy(const Group& g, const float* src, float factor, float* dst, int n) {
    for (int i = g.lane(); i < n; i += g.width()) dst[i] = src[i] * factor;
    g.fence();
}

// One position.  gv / gr / gp: the loss launch's gradient rows of this position (gr unread for k == 0).  has_next: a
// later position exists, and u.g_hidden holds what its dynamics sent back; on exit (k > 0) u.g_hidden holds what this
// position's dynamics sends to position k - 1.
template <class Group>
MZ_HD inline void position_backward(const Group& g, const Net& n, const float* w, int k, bool has_next, const float* act,
                                    float* del, const float* gv, const float* gr, const float* gp, float inv_batch,
                                    const Buffers& u) {
    scaled_copy(g, gp, inv_batch, u.t0, n.A);
    mlp_backward(g, n.policy, w, act, del, u.t0, u.t1, u.g_policy, n.enc);
    scaled_copy(g, gv, inv_batch, u.t0, n.F);
    mlp_backward(g, n.value, w, act, del, u.t0, u.t1, u.g_value, n.enc);
    if (k > 0) {
        scaled_copy(g, gr, inv_batch, u.t0, n.F);
        mlp_backward(g, n.reward, w, act, del, u.t0, u.t1, u.g_reward, n.enc);
    }
    // the whole gradient of the normalised state; a recurrent step's hidden state passes half of it on
    float s1 = 0.f, s2 = 0.f;
    for (int i = g.lane(); i < n.enc; i += g.width()) {
        float t = u.g_policy[i] + u.g_value[i];
        if (has_next) t = t + u.g_hidden[i];
        if (k > 0) t = t * 0.5f;
        u.g_policy[i] = t;
        s1 = s1 + t;
        s2 = s2 + t * act[n.off_norm + i];
    }
    s1 = g.sum(s1);
    s2 = g.sum(s2);
    const int imin = static_cast<int>(act[n.off_stats]), imax = static_cast<int>(act[n.off_stats + 1]);
    const float scale = act[n.off_stats + 2];
    const float d_scale = -(s2 / scale);
    const float d_min = -(s1 / scale);
    for (int i = g.lane(); i < n.enc; i += g.width()) {
        float r = u.g_policy[i] / scale;
        if (imin == imax) {
            if (i == imin) r = r + d_min;
        } else {
            if (i == imax) r = r + d_scale;
            if (i == imin) r = r + (d_min - d_scale);
        }
        if (k > 0) r = r + u.g_reward[i];
        u.t0[i] = r;
    }
    g.fence();
    if (k > 0)
        mlp_backward(g, n.dyn, w, act, del, u.t0, u.t1, u.g_hidden, n.enc);
    else
        mlp_backward(g, n.repr, w, act, del, u.t0, u.t1, static_cast<float*>(nullptr), 0);
}

// One sample: positions K1-1 .. 0.  act / del: the workspaces' first records; grad_*: the loss launch's step-major
// gradients [K1][B][F], [K1][B][F], [K1][B][A].
template <class Group>
MZ_HD inline void sample_backward(const Group& g, const Net& n, const float* w, int B, int K1, int b, const float* act,
                                  float* del, const float* grad_value, const float* grad_reward, const float* grad_policy,
                                  float inv_batch, const Buffers& u) {
    for (int k = K1 - 1; k >= 0; --k) {
        const size_t p = static_cast<size_t>(b) * K1 + k, row = static_cast<size_t>(k) * B + b;
        position_backward(g, n, w, k, k < K1 - 1, act + p * n.record_floats, del + p * n.record_floats,
                          grad_value + row * n.F, grad_reward + row * n.F, grad_policy + row * n.A, inv_batch, u);
    }
}

// Which positions a layer's parameters see: the representation step 0 only, dynamics and reward every step but 0.
enum Steps { kStepZero = 0, kStepsAfterZero = 1, kStepsAll = 2 };
MZ_HD inline bool step_counts(int steps, int k) { return steps == kStepsAll || (steps == kStepZero ? k == 0 : k > 0); }

// Part of one weight-gradient entry, dW[y][x] = sum over positions of delta[y] * input[x] (x_idx < 0: the bias, input 1):
// positions [p_begin, p_end) in order, b-major.  The product of two floats is exact in a double.
MZ_HD inline double weight_grad_partial(const float* act, const float* del, int record_floats, int x_idx, int y_idx, int K1,
                                        int steps, int p_begin, int p_end) {
    double sum = 0.0;
    for (int p = p_begin; p < p_end; ++p) {
        if (!step_counts(steps, p % K1)) continue;
        const size_t at = static_cast<size_t>(p) * record_floats;
        const double x = x_idx >= 0 ? static_cast<double>(act[at + x_idx]) : 1.0;
        sum = sum + static_cast<double>(del[at + y_idx]) * x;
    }
    return sum;
}

}  // namespace fcb
}  // namespace mz
