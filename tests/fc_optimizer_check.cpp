// fc_optimizer_check.cpp -- csrc/fc_optimizer.h built for the host by g++ under the address and undefined-behaviour
// sanitizers: the optimizer's steps on a case written by tests/test_fc_optimizer_cpu.py.  Every array is a heap block of its
// exact size (a buffer the kind does not use is not allocated at all), so the address sanitizer sees any index outside
// [0, n) and any touch of a moment the kind must leave alone.
//   in:  int32 kind, steps | int64 n, start | f64 beta1, beta2, eps, weight_decay, momentum | f64 lr[steps]
//        | f32 weights[n] | f32 grads[steps][n]
//   out: f32 weights[n] | f32 moment1[n] (zeros when unused) | f32 moment2[n] (zeros when unused)
//        | f64 bc1, bc2, step_size, bc2s of the last step (Adam; zeros for SGD)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fc_optimizer.h"

namespace fco = mz::fco;

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
    int32_t head[2];
    int64_t sizes[2];
    double hyper[5];
    read_exact(head, sizeof head, in);
    read_exact(sizes, sizeof sizes, in);
    read_exact(hyper, sizeof hyper, in);
    const int kind = head[0], steps = head[1];
    const int64_t n = sizes[0], start = sizes[1];
    if ((kind != fco::kAdam && kind != fco::kSgd) || steps < 0 || n <= 0) return 2;
    std::vector<double> lr(steps);
    read_exact(lr.data(), lr.size() * sizeof(double), in);
    std::vector<float> weights(n);
    read_exact(weights.data(), weights.size() * 4, in);
    std::vector<std::vector<float>> grads(steps);
    for (auto& g : grads) {
        g.resize(n);
        read_exact(g.data(), g.size() * 4, in);
    }
    fclose(in);

    const bool adam = kind == fco::kAdam, with_buffer = adam || hyper[4] != 0.0;
    std::vector<float> moment1(with_buffer ? n : 0, 0.f), moment2(adam ? n : 0, 0.f);
    fco::AdamScalars64 last{};
    for (int k = 0; k < steps; ++k) {
        const int64_t t = start + k + 1;
        fco::reference_step(kind, n, weights.data(), grads[k].data(), with_buffer ? moment1.data() : nullptr,
                            adam ? moment2.data() : nullptr, lr[k], t, hyper[0], hyper[1], hyper[2], hyper[3], hyper[4]);
        if (adam) last = fco::adam_scalars(lr[k], hyper[0], hyper[1], t);
    }
    moment1.resize(n, 0.f);
    moment2.resize(n, 0.f);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(weights.data(), 4, weights.size(), out);
    fwrite(moment1.data(), 4, moment1.size(), out);
    fwrite(moment2.data(), 4, moment2.size(), out);
    const double scalars[4] = {last.bc1, last.bc2, last.step_size, last.bc2s};
    fwrite(scalars, sizeof(double), 4, out);
    fclose(out);
    return 0;
}
