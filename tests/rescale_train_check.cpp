// rescale_train_check.cpp -- csrc/rescale_train.h as a stand-alone host program (g++, address and undefined-behaviour
// sanitizers): tests/test_rescale_train_cpu.py feeds it a case and compares what it writes with the library's host entry, bit
// for bit.
//
//   rescale_train_check <case file> <result file>
// case:   int64 rows, int32 row_len, then x [rows][row_len] and g [rows][row_len]
// result: dx [rows][row_len], then the plan as int64 {grid, block, rows per workgroup, row stride, LDS bytes}
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rescale_train.h"

namespace rst = mz::rst;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int64_t rows = 0;
    int32_t row_len = 0;
    if (std::fread(&rows, sizeof(rows), 1, in) != 1 || std::fread(&row_len, sizeof(row_len), 1, in) != 1) return 4;
    if (rst::refusal(rows, row_len)) return 5;
    const size_t n = static_cast<size_t>(rows) * static_cast<size_t>(row_len);
    std::vector<float> x(n), g(n), dx(n, -1.f);
    if (std::fread(x.data(), sizeof(float), n, in) != n || std::fread(g.data(), sizeof(float), n, in) != n) return 7;
    std::fclose(in);

    rst::reference_backward(x.data(), g.data(), dx.data(), rows, row_len);
    rst::Plan plan;
    if (!rst::plan_rescale_backward(rows, row_len, &plan)) return 6;
    const int64_t planned[5] = {plan.grid, plan.block, plan.rows_per_group, plan.row_stride, static_cast<int64_t>(plan.lds)};

    std::FILE* result = std::fopen(argv[2], "wb");
    if (!result) return 8;
    if (std::fwrite(dx.data(), sizeof(float), n, result) != n || std::fwrite(planned, sizeof(int64_t), 5, result) != 5) return 9;
    return std::fclose(result) == 0 ? 0 : 10;
}
