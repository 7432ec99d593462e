// bn_epilogue_check.cpp -- csrc/bn_epilogue.h built for the host by g++ under the address and undefined-behaviour
// sanitizers: forward and backward of one case written by tests/test_bn_epilogue_cpu.py.  Every array is a heap block of its
// exact size (the residual and its gradient are not allocated at all without a residual), so the address sanitizer sees any
// index outside a tensor.
//   in:  int64 batch | int32 channels, hw, with_residual, pad | f64 eps, momentum | f32 x[n] | f32 residual[n] (if any)
//        | f32 gamma[c], beta[c], running_mean[c], running_var[c] | f32 dy[n]            (n = batch * channels * hw)
//   out: f32 out[n] | f32 dx[n] | f32 dresidual[n] (if any) | f32 mean[c], invstd[c], running_mean[c], running_var[c],
//        dgamma[c], dbeta[c]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bn_epilogue.h"

namespace bne = mz::bne;

static void read_exact(void* dst, size_t bytes, FILE* f) {
    if (bytes && fread(dst, 1, bytes, f) != bytes) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

static std::vector<float> read_floats(size_t count, FILE* f) {
    std::vector<float> v(count);
    read_exact(v.data(), count * 4, f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t batch;
    int32_t head[4];
    double hyper[2];
    read_exact(&batch, sizeof batch, in);
    read_exact(head, sizeof head, in);
    read_exact(hyper, sizeof hyper, in);
    const int32_t channels = head[0], hw = head[1];
    const bool with_residual = head[2] != 0;
    if (batch < 1 || channels < 1 || hw < 1 || batch * hw < 2) return 2;
    const size_t n = static_cast<size_t>(batch) * channels * hw, c = channels;
    const std::vector<float> x = read_floats(n, in);
    const std::vector<float> residual = read_floats(with_residual ? n : 0, in);
    const std::vector<float> gamma = read_floats(c, in), beta = read_floats(c, in);
    std::vector<float> running_mean = read_floats(c, in), running_var = read_floats(c, in);
    const std::vector<float> dy = read_floats(n, in);
    fclose(in);

    const bne::Shape shape{batch, channels, hw};
    std::vector<float> out(n), dx(n), dresidual(with_residual ? n : 0), mean(c), invstd(c), dgamma(c), dbeta(c);
    bne::reference_forward(shape, x.data(), with_residual ? residual.data() : nullptr, gamma.data(), beta.data(),
                           running_mean.data(), running_var.data(), hyper[0], hyper[1], out.data(), mean.data(),
                           invstd.data());
    bne::reference_backward(shape, dy.data(), x.data(), out.data(), gamma.data(), mean.data(), invstd.data(), dx.data(),
                            with_residual ? dresidual.data() : nullptr, dgamma.data(), dbeta.data());

    FILE* result = fopen(argv[2], "wb");
    if (!result) return 2;
    for (const std::vector<float>* v : {&out, &dx, &dresidual, &mean, &invstd, &running_mean, &running_var, &dgamma, &dbeta})
        if (!v->empty()) fwrite(v->data(), 4, v->size(), result);
    fclose(result);
    return 0;
}
