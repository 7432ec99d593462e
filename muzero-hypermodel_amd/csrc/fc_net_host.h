// fc_net_host.h -- host side of fc_net_device.h: a MuZeroFullyConnectedNetwork's layer description (include/mzmcts.h
// mzmcts_fc_desc) turned into the FcNet the device functions walk -- weight offsets in the flat state_dict-order buffer,
// the padded on-chip layout, the scratch regions and the phase lists.  One function for every caller that evaluates the
// network in a kernel: the search engine (mzmcts_fc_configure) and the replay store's Reanalyse pass
// (mzreplay_reanalyse_fc_configure).
#pragma once
#include <algorithm>
#include <initializer_list>

#include "../../include/mzmcts.h"
#include "fc_net_device.h"

namespace mz {

enum FcNetError { kFcNetOk = 0, kFcNetSizes = 1, kFcNetWeightCount = 2 };
constexpr const char* kFcNetSizesMessage = "layer sizes outside the supported range (<= 3 hidden layers per MLP, widths <= 256)";
constexpr const char* kFcNetWeightCountMessage = "n_weights does not match the layer description";

inline int bind_mlp(FcMlp* m, int in, const int32_t* hidden, int n_hidden, int out, int* cursor, int* lds_cursor,
                    int* max_hidden) {
    if (n_hidden < 0 || n_hidden > kFcMaxLayers - 1) return -1;
    int widths[kFcMaxLayers + 1];
    widths[0] = in;
    for (int i = 0; i < n_hidden; ++i) widths[i + 1] = hidden[i];
    widths[n_hidden + 1] = out;
    m->n_layers = n_hidden + 1;
    for (int l = 0; l < m->n_layers; ++l) {
        if (widths[l] <= 0 || widths[l + 1] <= 0 || widths[l] > kFcMaxWidth || widths[l + 1] > kFcMaxWidth) return -1;
        m->layer[l].in = widths[l];
        m->layer[l].out = widths[l + 1];
        m->layer[l].w_off = *cursor;
        *cursor += widths[l] * widths[l + 1];
        m->layer[l].b_off = *cursor;
        *cursor += widths[l + 1];
        m->layer[l].in_pad = (widths[l] + 3) / 4 * 4;
        m->layer[l].w_lds = *lds_cursor;
        *lds_cursor += m->layer[l].in_pad * widths[l + 1];
        m->layer[l].b_lds = *lds_cursor;
        *lds_cursor += (widths[l + 1] + 3) / 4 * 4;
        if (l < m->n_layers - 1 && widths[l + 1] > *max_hidden) *max_hidden = widths[l + 1];
    }
    return 0;
}

// d: the layer description; A actions, support_size s (F = 2 s + 1 logits per value / reward head); n_weights: floats of
// the flat buffer.  Returns kFcNetOk and fills *out, or says which check failed (the caller words the message).
inline int build_fc_net(const mzmcts_fc_desc* d, int A, int support, int64_t n_weights, FcNet* out) {
    FcNet net{};
    net.obs = d->observation_floats;
    net.enc = d->encoding_size;
    net.A = A;
    net.F = 2 * support + 1;
    net.support = support;
    int cursor = 0, lds_cursor = 0, max_hidden = 1;
    int rc = 0;
    rc |= bind_mlp(&net.repr, net.obs, d->hidden[0], d->n_hidden[0], net.enc, &cursor, &lds_cursor, &max_hidden);
    rc |= bind_mlp(&net.dyn, net.enc + net.A, d->hidden[1], d->n_hidden[1], net.enc, &cursor, &lds_cursor, &max_hidden);
    rc |= bind_mlp(&net.reward, net.enc, d->hidden[2], d->n_hidden[2], net.F, &cursor, &lds_cursor, &max_hidden);
    rc |= bind_mlp(&net.policy, net.enc, d->hidden[3], d->n_hidden[3], net.A, &cursor, &lds_cursor, &max_hidden);
    rc |= bind_mlp(&net.value, net.enc, d->hidden[4], d->n_hidden[4], net.F, &cursor, &lds_cursor, &max_hidden);
    if (rc != 0 || net.obs <= 0 || net.obs > kFcMaxWidth) return kFcNetSizes;
    if (cursor != n_weights) return kFcNetWeightCount;
    net.n_weights = cursor;
    net.n_weights_lds = lds_cursor;
    // scratch regions (floats, 16-byte aligned): x_in | raw | norm | reward | value | policy | 3 heads x 2 temps
    auto pad4 = [](int v) { return (v + 3) / 4 * 4; };
    int off = pad4(std::max(net.obs, net.enc + net.A));
    net.off_raw = off;
    off += pad4(net.enc);
    net.off_norm = off;
    off += pad4(net.enc);
    net.off_reward = off;
    off += pad4(net.F);
    net.off_value = off;
    off += pad4(net.F);
    net.off_policy = off;
    off += pad4(net.A);
    int temp[3][2];
    for (int h = 0; h < 3; ++h)
        for (int t = 0; t < 2; ++t) {
            temp[h][t] = off;
            off += pad4(max_hidden);
        }
    net.scratch_floats = std::max(off, 64);  // >= 256 B: the fused kernel's backup borrows it (tree_device.h)
    auto job_of = [&](const FcMlp& m, int l, int x_first, int y_last, int head) {
        FcJob jb{};
        const FcLayer& L = m.layer[l];
        jb.in_pad = L.in_pad;
        jb.out = L.out;
        jb.w_lds = L.w_lds;
        jb.b_lds = L.b_lds;
        jb.x_off = (l == 0) ? x_first : temp[head][(l - 1) & 1];
        jb.y_off = (l == m.n_layers - 1) ? y_last : temp[head][l & 1];
        jb.elu = (l == m.n_layers - 1) ? 0 : 1;
        return jb;
    };
    auto chain = [&](const FcMlp& m, int x_first, int y_last, FcPhase* phases, int32_t* count) {
        *count = m.n_layers;
        for (int l = 0; l < m.n_layers; ++l) {
            phases[l].n_jobs = 1;
            phases[l].job[0] = job_of(m, l, x_first, y_last, 0);
            phases[l].total_out = phases[l].job[0].out;
        }
    };
    struct Head {
        const FcMlp* mlp;
        int x_first, y_last;
    };
    auto heads = [&](std::initializer_list<Head> hs, FcPhase* phases, int32_t* count) {
        int depth = 0;
        for (const Head& h : hs) depth = std::max(depth, static_cast<int>(h.mlp->n_layers));
        *count = depth;
        for (int l = 0; l < depth; ++l) {
            phases[l].n_jobs = 0;
            phases[l].total_out = 0;
            int head_index = 0;
            for (const Head& h : hs) {
                if (l < h.mlp->n_layers) {
                    phases[l].job[phases[l].n_jobs] = job_of(*h.mlp, l, h.x_first, h.y_last, head_index);
                    phases[l].total_out += h.mlp->layer[l].out;
                    phases[l].n_jobs += 1;
                }
                ++head_index;
            }
        }
    };
    chain(net.repr, 0, net.off_raw, net.init_pre, &net.n_init_pre);
    heads({{&net.policy, net.off_norm, net.off_policy}, {&net.value, net.off_norm, net.off_value}}, net.init_post,
          &net.n_init_post);
    chain(net.dyn, 0, net.off_raw, net.rec_pre, &net.n_rec_pre);
    heads({{&net.reward, net.off_raw, net.off_reward},
           {&net.policy, net.off_norm, net.off_policy},
           {&net.value, net.off_norm, net.off_value}},
          net.rec_post, &net.n_rec_post);
    *out = net;
    return kFcNetOk;
}

}  // namespace mz
