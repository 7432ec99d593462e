// Host-side check of csrc/reanalyse_plan.h (the plan of a batched Reanalyse pass, as the kernels of mzreplay.hip compute
// it), built and driven by tests/test_reanalyse_plan_cpu.py:
//     g++ -O2 -std=c++17 -ffp-contract=off reanalyse_plan_check.cpp
// Inputs are little-endian binary files written by the test; one JSON object on the last line.
//
//   reanalyse_plan_check draws FILE   u32 seed; i32 n_stored; i32 count; i32 passes: `passes` passes of `count` draws each
//                                     on numpy.random.seed(seed) -> indices, the stream's key and position afterwards
//   reanalyse_plan_check plan FILE    i32 n_games, n_stored, capacity; i64 oldest_id; i32 length[capacity] (by slot);
//                                     i64 ids[n_games]: plan_serial on given ids -> slots, row_start, and for every row
//                                     the draw draw_of_row finds
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reanalyse_plan.h"

namespace {

struct Reader {
    std::vector<unsigned char> data;
    size_t at = 0;
    explicit Reader(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) {
            std::perror(path);
            std::exit(2);
        }
        unsigned char buf[65536];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + got);
        std::fclose(f);
    }
    template <typename T>
    T one() {
        T v;
        if (at + sizeof(T) > data.size()) std::exit(3);
        std::memcpy(&v, data.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <typename T>
    std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (at + sizeof(T) * n > data.size()) std::exit(3);
        if (n) std::memcpy(v.data(), data.data() + at, sizeof(T) * n);
        at += sizeof(T) * n;
        return v;
    }
};

template <typename T>
void print_list(const char* name, const std::vector<T>& v, bool last = false) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", static_cast<long long>(v[i]));
    std::printf("]%s", last ? "" : ", ");
}

int draws(Reader& in) {
    const uint32_t seed = in.one<uint32_t>();
    const int32_t n_stored = in.one<int32_t>(), count = in.one<int32_t>(), passes = in.one<int32_t>();
    std::vector<uint32_t> key(mz::kMtN);
    int32_t pos = 0;
    mz::mt_seed(key.data(), &pos, seed);
    std::vector<int64_t> index;
    const std::vector<int32_t> length(1, 1);
    for (int pass = 0; pass < passes; ++pass) {
        // through plan_serial, with one slot per game so that the ids are the indices
        std::vector<int64_t> ids(count);
        std::vector<int32_t> slots(count), row_start(count + 1);
        std::vector<int32_t> lengths(static_cast<size_t>(n_stored), 1);
        mz::reanalyse::plan_serial(key.data(), &pos, count, 0, n_stored, n_stored, nullptr, lengths.data(), ids.data(),
                                   slots.data(), row_start.data());
        index.insert(index.end(), ids.begin(), ids.end());
    }
    std::printf("{");
    print_list("index", index);
    print_list("key", std::vector<int64_t>(key.begin(), key.end()));
    std::printf("\"pos\": %d}\n", pos);
    return 0;
}

int plan(Reader& in) {
    const int32_t n_games = in.one<int32_t>(), n_stored = in.one<int32_t>(), capacity = in.one<int32_t>();
    const int64_t oldest = in.one<int64_t>();
    const std::vector<int32_t> length = in.many<int32_t>(static_cast<size_t>(capacity));
    const std::vector<int64_t> given = in.many<int64_t>(static_cast<size_t>(n_games));
    std::vector<int64_t> ids(n_games);
    std::vector<int32_t> slots(n_games), row_start(n_games + 1);
    uint32_t key[mz::kMtN];
    int32_t pos = 0;
    mz::mt_seed(key, &pos, 0);
    const int32_t rows = mz::reanalyse::plan_serial(key, &pos, n_games, oldest, n_stored, capacity, given.data(), length.data(),
                                                    ids.data(), slots.data(), row_start.data());
    std::vector<int32_t> draw_of(static_cast<size_t>(rows));
    for (int32_t r = 0; r < rows; ++r)
        draw_of[r] = mz::reanalyse::draw_of_row([&](int i) { return row_start[i]; }, n_games, r);
    std::printf("{");
    print_list("game_ids", ids);
    print_list("slots", slots);
    print_list("row_start", row_start);
    print_list("draw_of_row", draw_of);
    std::printf("\"pos\": %d, \"fits\": [%d, %d]}\n", pos, mz::reanalyse::rows_fit(4096, 524287) ? 1 : 0,
                mz::reanalyse::rows_fit(4096, 524288) ? 1 : 0);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    Reader in(argv[2]);
    if (!std::strcmp(argv[1], "draws")) return draws(in);
    if (!std::strcmp(argv[1], "plan")) return plan(in);
    return 1;
}
