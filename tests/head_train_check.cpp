// head_train_check.cpp -- csrc/head_train.h as a stand-alone host program (g++, address and undefined-behaviour sanitizers):
// tests/test_head_train_cpu.py feeds it a case and compares what it writes with the library's host entries, bit for bit.
//
//   head_train_check <case file> <result file>
// case:   int64 batch, int32 channels, plane, n_heads, then per head int32 reduced, hidden, outputs; then x [B][C][P] and per
//         head conv_w, conv_b, fc1_w, fc1_b, fc2_w, fc2_b, dlogits [B][O]
// result: per head logits, flat, pre, dpre, dflat, dconv_w, dconv_b, dfc1_w, dfc1_b, dfc2_w, dfc2_b; then dx
#include <cstdint>
#include <cstdio>
#include <vector>

#include "head_train.h"

namespace hdt = mz::hdt;

static bool read_floats(std::FILE* f, std::vector<float>* v, size_t n) {
    v->resize(n);
    return std::fread(v->data(), sizeof(float), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t batch = 0;
    int32_t dims[3] = {0, 0, 0};
    if (std::fread(&batch, sizeof(batch), 1, in) != 1 || std::fread(dims, sizeof(int32_t), 3, in) != 3) return 4;
    const int C = dims[0], P = dims[1], n_heads = dims[2];
    if (n_heads < 1 || n_heads > hdt::kMaxHeads || batch < 1 || batch > hdt::kMaxBatch) return 5;
    int32_t sizes[hdt::kMaxHeads][3] = {};
    for (int h = 0; h < n_heads; ++h) {
        if (std::fread(sizes[h], sizeof(int32_t), 3, in) != 3) return 4;
        if (hdt::refusal(C, P, sizes[h][0], sizes[h][1], sizes[h][2], n_heads)) return 5;
    }
    std::vector<float> x, param[hdt::kMaxHeads][6], dlogits[hdt::kMaxHeads];
    if (!read_floats(in, &x, batch * C * P)) return 7;
    for (int h = 0; h < n_heads; ++h) {
        const size_t R = sizes[h][0], Hd = sizes[h][1], O = sizes[h][2];
        const size_t counts[6] = {R * C, R, Hd * R * P, Hd, O * Hd, O};
        for (int i = 0; i < 6; ++i)
            if (!read_floats(in, &param[h][i], counts[i])) return 7;
        if (!read_floats(in, &dlogits[h], batch * O)) return 7;
    }
    std::fclose(in);

    // outputs: logits, flat, pre, dpre, dflat, then the six gradients
    std::vector<float> out[hdt::kMaxHeads][11], dx(batch * C * P);
    hdt::Head heads[hdt::kMaxHeads] = {};
    hdt::ReduceHead red[hdt::kMaxHeads] = {};
    float *logits[hdt::kMaxHeads] = {}, *flat[hdt::kMaxHeads] = {}, *pre[hdt::kMaxHeads] = {}, *dpre[hdt::kMaxHeads] = {},
          *dflat[hdt::kMaxHeads] = {};
    for (int h = 0; h < n_heads; ++h) {
        const size_t R = sizes[h][0], Hd = sizes[h][1], O = sizes[h][2];
        const size_t counts[11] = {batch * O, batch * R * P, batch * Hd, batch * Hd, batch * R * P,
                                   R * C,     R,             Hd * R * P, Hd,         O * Hd,        O};
        for (int i = 0; i < 11; ++i) out[h][i].assign(counts[i], -1.f);
        heads[h] = hdt::Head{param[h][0].data(), param[h][1].data(), param[h][2].data(), param[h][3].data(),
                             param[h][4].data(), param[h][5].data(), sizes[h][0],        sizes[h][1],        sizes[h][2]};
        logits[h] = out[h][0].data(), flat[h] = out[h][1].data(), pre[h] = out[h][2].data();
        dpre[h] = out[h][3].data(), dflat[h] = out[h][4].data();
        red[h] = hdt::ReduceHead{x.data(), flat[h], pre[h], dlogits[h].data(), dpre[h], dflat[h],
                                 {out[h][5].data(), out[h][6].data(), out[h][7].data(), out[h][8].data(), out[h][9].data(),
                                  out[h][10].data()},
                                 sizes[h][0], sizes[h][1], sizes[h][2]};
    }
    hdt::reference_forward(x.data(), heads, n_heads, logits, flat, pre, batch, C, P);
    hdt::reference_backward(heads, red, n_heads, dpre, dflat, dx.data(), batch, C, P);

    std::FILE* result = std::fopen(argv[2], "wb");
    if (!result) return 8;
    for (int h = 0; h < n_heads; ++h)
        for (int i = 0; i < 11; ++i)
            if (std::fwrite(out[h][i].data(), sizeof(float), out[h][i].size(), result) != out[h][i].size()) return 9;
    if (std::fwrite(dx.data(), sizeof(float), dx.size(), result) != dx.size()) return 9;
    return std::fclose(result) == 0 ? 0 : 10;
}
