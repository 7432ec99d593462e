// fc_backward_check.cpp -- csrc/fc_backward.h built for the host: the backward rule and the weight-gradient sum of the HIP
// training step in float32 on a case written by tests/test_fc_backward_cpu.py (the float64 yardstick's activations and logit
// gradients, rounded to float32), one lane (fcb::Serial).  Every array is a heap block of its exact size, so the address
// sanitizer sees any index outside a record, a weight row or a gradient.
//   in:  int32 B, K1, n_weights, n_plan | fcb::Net as int32 | n_plan x {in, out, x_off, y_off, w_dst, b_dst, steps}
//        | f32 weights | act [B][K1][record] | grad_value [K1][B][F] | grad_reward [K1][B][F] | grad_policy [K1][B][A]
//   out: f32 del [B][K1][record] | grads [n_weights]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fc_backward.h"

namespace fcb = mz::fcb;

static void read_exact(void* dst, size_t bytes, FILE* f) {
    if (bytes && fread(dst, 1, bytes, f) != bytes) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[4];
    read_exact(head, sizeof head, in);
    const int B = head[0], K1 = head[1], n_weights = head[2], n_plan = head[3];
    fcb::Net net;
    static_assert(sizeof(fcb::Net) == 4 * (9 + 5 * (1 + fcb::kMaxLayers * 7)), "fcb::Net is plain int32 words");
    read_exact(&net, sizeof net, in);
    std::vector<int32_t> plan(static_cast<size_t>(n_plan) * 7);
    read_exact(plan.data(), plan.size() * 4, in);
    const size_t P = static_cast<size_t>(B) * K1, R = net.record_floats;
    std::vector<float> weights(n_weights), act(P * R), gv(P * net.F), gr(P * net.F), gp(P * net.A);
    read_exact(weights.data(), weights.size() * 4, in);
    read_exact(act.data(), act.size() * 4, in);
    read_exact(gv.data(), gv.size() * 4, in);
    read_exact(gr.data(), gr.size() * 4, in);
    read_exact(gp.data(), gp.size() * 4, in);
    fclose(in);

    std::vector<float> del(P * R, 0.f), grads(n_weights, -12345.f);
    std::vector<std::vector<float>> temp(fcb::kBuffers, std::vector<float>(net.width));
    fcb::Buffers u{temp[0].data(), temp[1].data(), temp[2].data(), temp[3].data(), temp[4].data(), temp[5].data()};
    const float inv_batch = 1.0f / static_cast<float>(B);
    for (int b = 0; b < B; ++b)
        fcb::sample_backward(fcb::Serial{}, net, weights.data(), B, K1, b, act.data(), del.data(), gv.data(), gr.data(),
                             gp.data(), inv_batch, u);
    for (int l = 0; l < n_plan; ++l) {
        const int32_t* L = &plan[static_cast<size_t>(l) * 7];
        const int in_w = L[0], out_w = L[1], x_off = L[2], y_off = L[3], w_dst = L[4], b_dst = L[5], steps = L[6];
        for (int j = 0; j < out_w; ++j)
            for (int i = 0; i <= in_w; ++i) {
                const double sum = fcb::weight_grad_partial(act.data(), del.data(), net.record_floats, i < in_w ? x_off + i : -1,
                                                            y_off + j, K1, steps, 0, static_cast<int>(P));
                if (i < in_w)
                    grads[static_cast<size_t>(w_dst) + static_cast<size_t>(j) * in_w + i] = static_cast<float>(sum);
                else
                    grads[static_cast<size_t>(b_dst) + j] = static_cast<float>(sum);
            }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(del.data(), 4, del.size(), out);
    fwrite(grads.data(), 4, grads.size(), out);
    fclose(out);
    return 0;
}
