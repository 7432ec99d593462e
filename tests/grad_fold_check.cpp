// grad_fold_check.cpp -- csrc/grad_fold.h built for the host by g++ under the address and undefined-behaviour sanitizers: the
// fold-and-update steps on a case written by tests/test_grad_fold_cpu.py.  Every array is a heap block of its exact size (a
// moment the kind does not use is not allocated at all), so the address sanitizer sees any index outside the flat buffers or
// the staging buffer and any touch of a moment the kind must leave alone.  The plan is walked too: every chunk must lie in
// its segment.
//   in:  int32 kind, steps, n_segments, pad | int64 n, staging_floats | f64 beta1, beta2, eps, weight_decay, momentum
//        | f64 lr[steps] | Segment[n_segments] | int32 uses[n_segments] | f32 weights[n] | f32 grads[n] | f32 moment1[n]
//        | f32 moment2[n] | f32 staging[steps][staging_floats]
//   out: f32 weights[n] | f32 grads[n] | f32 moment1[n] | f32 moment2[n]      (a moment the kind does not use: as read)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grad_fold.h"

namespace fco = mz::fco;
namespace gfold = mz::gfold;

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
    int64_t sizes[2];
    double hyper[5];
    read_exact(head, sizeof head, in);
    read_exact(sizes, sizeof sizes, in);
    read_exact(hyper, sizeof hyper, in);
    const int kind = head[0], steps = head[1], n_segments = head[2];
    const int64_t n = sizes[0], staging_floats = sizes[1];
    if ((kind != fco::kAdam && kind != fco::kSgd) || steps < 0 || n_segments <= 0 || n <= 0 || staging_floats <= 0) return 2;
    std::vector<double> lr(steps);
    read_exact(lr.data(), lr.size() * sizeof(double), in);
    std::vector<gfold::Segment> segments(n_segments);
    read_exact(segments.data(), segments.size() * sizeof(gfold::Segment), in);
    std::vector<int32_t> uses(n_segments);
    read_exact(uses.data(), uses.size() * 4, in);
    std::vector<float> weights(n), grads(n), kept1(n), kept2(n);
    read_exact(weights.data(), n * 4, in);
    read_exact(grads.data(), n * 4, in);
    read_exact(kept1.data(), n * 4, in);
    read_exact(kept2.data(), n * 4, in);
    std::vector<std::vector<float>> staging(steps);
    for (auto& s : staging) {
        s.resize(staging_floats);
        read_exact(s.data(), s.size() * 4, in);
    }
    fclose(in);

    int32_t at = -1;
    if (const char* why = gfold::check_segments(segments.data(), n_segments, n, staging_floats, &at)) {
        fprintf(stderr, "%s (segment %d)\n", why, at);
        return 3;
    }
    if (const char* why = gfold::check_uses(segments.data(), uses.data(), n_segments, &at)) {
        fprintf(stderr, "%s (segment %d)\n", why, at);
        return 3;
    }
    const gfold::FoldPlan plan = gfold::plan_fold(segments.data(), n_segments);
    std::vector<gfold::Chunk> chunks(plan.chunks);
    gfold::fill_chunks(segments.data(), n_segments, chunks.data());
    for (const gfold::Chunk& c : chunks)
        if (c.segment < 0 || c.segment >= n_segments || c.first < 0 || c.count < 1 || c.count > gfold::kChunk ||
            c.first + c.count > segments[c.segment].count)
            return 4;

    const bool adam = kind == fco::kAdam, with_buffer = adam || hyper[4] != 0.0;
    std::vector<float> moment1, moment2;
    if (with_buffer) moment1 = kept1;
    if (adam) moment2 = kept2;
    for (int k = 0; k < steps; ++k)
        gfold::reference_step(kind, segments.data(), uses.data(), n_segments, staging[k].data(), weights.data(), grads.data(),
                              with_buffer ? moment1.data() : nullptr, adam ? moment2.data() : nullptr, lr[k], k + 1, hyper[0],
                              hyper[1], hyper[2], hyper[3], hyper[4]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(weights.data(), 4, n, out);
    fwrite(grads.data(), 4, n, out);
    fwrite(with_buffer ? moment1.data() : kept1.data(), 4, n, out);
    fwrite(adam ? moment2.data() : kept2.data(), 4, n, out);
    fclose(out);
    return 0;
}
