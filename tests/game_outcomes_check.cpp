// game_outcomes_check.cpp -- csrc/game_outcomes.h as a stand-alone host program (tests/test_game_outcomes_cpu.py builds it
// with -fsanitize=address,undefined and compares its output with the library's host entry, bit for bit).
//   game_outcomes_check <cases> <result>
// <cases>: i32 count, then per case i32 n, rewards f64[n + 1], to_play i8[n + 1], root_values f64[n]
// <result>: one 40-byte Outcome per case
// Every array is a heap block of its exact size, so that a read or write past a row's end is an error the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "game_outcomes.h"

static_assert(sizeof(mz::outcomes::Outcome) == 40, "40 bytes per game");

template <typename T>
static std::unique_ptr<T[]> read_block(std::FILE* f, size_t count) {
    std::unique_ptr<T[]> block(new T[count]);
    if (std::fread(block.get(), sizeof(T), count, f) != count) {
        std::fprintf(stderr, "game_outcomes_check: the case file is short\n");
        std::exit(2);
    }
    return block;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: game_outcomes_check <cases> <result>\n");
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "game_outcomes_check: cannot open the files\n");
        return 2;
    }
    const int32_t count = *read_block<int32_t>(in, 1).get();
    for (int32_t c = 0; c < count; ++c) {
        const int32_t n = *read_block<int32_t>(in, 1).get();
        if (n < 1) {
            std::fprintf(stderr, "game_outcomes_check: a game has at least one move\n");
            return 2;
        }
        const auto rewards = read_block<double>(in, static_cast<size_t>(n) + 1);
        const auto to_play = read_block<int8_t>(in, static_cast<size_t>(n) + 1);
        const auto root_values = read_block<double>(in, static_cast<size_t>(n));
        std::unique_ptr<double[]> packed(new double[n]);
        mz::outcomes::Outcome o;
        std::memset(&o, 0, sizeof(o));
        o = mz::outcomes::game_outcome(rewards.get(), to_play.get(), root_values.get(), n, packed.get());
        // the sum once more the way a wavefront takes it (leaves named without a stack, summed in place, then walked)
        mz::outcomes::WalkStack stack;
        const double again = mz::outcomes::pairwise_sum_by_leaves(stack, packed.get(), o.value_count);
        if (std::memcmp(&again, &o.value_sum, sizeof(double)) != 0 && !(again != again && o.value_sum != o.value_sum)) {
            std::fprintf(stderr, "game_outcomes_check: case %d: the sum by leaves differs from the walk's\n", c);
            return 3;
        }
        if (std::fwrite(&o, sizeof(o), 1, out) != 1) return 2;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
