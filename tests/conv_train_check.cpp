// conv_train_check.cpp -- csrc/conv_train.h as a stand-alone host program (g++, address and undefined-behaviour sanitizers):
// tests/test_conv_train_cpu.py feeds it a case and compares what it writes with the library's host entries, bit for bit.
//
//   conv_train_check <case file> <result file>
// case:   int64 batch, int32 cin, cout, height, width, dx_planes, then x [B][cin][P], w [cout][cin][9], dy [B][cout][P]
// result: y [B][cout][P], dx [B][dx_planes][P] (nothing for dx_planes 0), dw [cout][cin][9], the forward packing, the
//         data-gradient packing (nothing for dx_planes 0), then the plan {grid, block, lds, slices, rounds} as five floats
#include <cstdint>
#include <cstdio>
#include <vector>

#include "conv_train.h"

namespace cvt = mz::cvt;

static bool read_floats(std::FILE* f, std::vector<float>* v, size_t n) {
    v->resize(n);
    return std::fread(v->data(), sizeof(float), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t batch = 0;
    int32_t dims[5] = {0, 0, 0, 0, 0};
    if (std::fread(&batch, sizeof(batch), 1, in) != 1 || std::fread(dims, sizeof(int32_t), 5, in) != 5) return 4;
    const int cin = dims[0], cout = dims[1], height = dims[2], width = dims[3], dx_planes = dims[4];
    if (!cvt::conv_supported(cin, cout, height, width, dx_planes)) return 5;
    cvt::WgradPlan plan;
    if (cvt::plan_conv_wgrad(batch, cin, cout, height, width, &plan) != MZMCTS_OK) return 6;
    const size_t P = static_cast<size_t>(height) * width;
    std::vector<float> x, w, dy;
    if (!read_floats(in, &x, batch * cin * P) || !read_floats(in, &w, static_cast<size_t>(cout) * cin * 9) ||
        !read_floats(in, &dy, batch * cout * P))
        return 7;
    std::fclose(in);

    std::vector<float> y(batch * cout * P), dx(batch * dx_planes * P), dw(static_cast<size_t>(cout) * cin * 9);
    cvt::reference_forward(x.data(), w.data(), y.data(), batch, cin, cout, height, width);
    if (dx_planes > 0) cvt::reference_dgrad(dy.data(), w.data(), dx.data(), batch, cin, cout, height, width, dx_planes);
    cvt::reference_wgrad(x.data(), dy.data(), dw.data(), batch, cin, cout, height, width);
    std::vector<float> packed(mz::conv_packed_floats(cin, cout)), packed_dx(dx_planes > 0 ? mz::conv_packed_floats(cout, dx_planes) : 0);
    for (size_t i = 0; i < packed.size(); ++i) packed[i] = cvt::pack_forward_value(w.data(), cin, cout, static_cast<int>(i));
    for (size_t i = 0; i < packed_dx.size(); ++i)
        packed_dx[i] = cvt::pack_dgrad_value(w.data(), cin, cout, dx_planes, static_cast<int>(i));
    const float plan_out[5] = {static_cast<float>(plan.grid), static_cast<float>(plan.block), static_cast<float>(plan.lds),
                               static_cast<float>(plan.slices), static_cast<float>(plan.rounds)};

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 8;
    for (const std::vector<float>* v : {&y, &dx, &dw, &packed, &packed_dx})
        if (!v->empty() && std::fwrite(v->data(), sizeof(float), v->size(), out) != v->size()) return 9;
    if (std::fwrite(plan_out, sizeof(float), 5, out) != 5) return 9;
    return std::fclose(out) == 0 ? 0 : 10;
}
