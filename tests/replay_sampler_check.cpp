// Host-side check of csrc/replay_sampler.h (the arithmetic the device sampler of the replay store runs), built and
// driven by tests/test_replay_sampler_cpu.py:
//     g++ -O2 -std=c++17 -ffp-contract=off replay_sampler_check.cpp
// Inputs are little-endian binary files written by the test; every answer is printed as integers (float32 values as
// their bit patterns), one JSON object on the last line.
//
//   replay_sampler_check sum FILE      i32 count, then per array i32 n, f32[n]: numpy_sum_f32 of each
//   replay_sampler_check batch FILE    i32 n_games, stride, unroll, actions, per, batch; u32 seed; i64 total_samples;
//                                      f32 game_priority[n_games]; i32 length[n_games]; f32 priorities[n_games][stride]:
//                                      one get_batch on numpy.random.seed(seed) by sample_batch_serial
//   replay_sampler_check update FILE   i32 n_games, stride, steps, batch; i64 oldest_id; i32 length[n_games];
//                                      f32 priorities[n_games][stride]; i64 game_ids[batch]; i32 positions[batch];
//                                      f32 fresh[batch][steps]: update_priorities_serial
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "replay_sampler.h"

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

uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

template <typename T, typename F>
void print_list(const char* name, const std::vector<T>& v, F as_integer, bool last = false) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", static_cast<long long>(as_integer(v[i])));
    std::printf("]%s", last ? "" : ", ");
}

int run_sum(Reader& in) {
    const int count = in.one<int32_t>();
    std::vector<float> out;
    for (int k = 0; k < count; ++k) {
        const int n = in.one<int32_t>();
        const std::vector<float> a = in.many<float>(static_cast<size_t>(n));
        out.push_back(mz::replay::numpy_sum_f32([&](int i) { return a[i]; }, n));
    }
    std::printf("{");
    print_list("sums", out, bits, true);
    std::printf("}\n");
    return 0;
}

int run_batch(Reader& in) {
    mz::replay::BatchView v{};
    v.n_games = in.one<int32_t>();
    v.stride = in.one<int32_t>();
    v.unroll = in.one<int32_t>();
    v.num_actions = in.one<int32_t>();
    const int per = in.one<int32_t>();
    const int batch = in.one<int32_t>();
    const uint32_t seed = in.one<uint32_t>();
    v.total_samples = in.one<int64_t>();
    const std::vector<float> game_priority = in.many<float>(static_cast<size_t>(v.n_games));
    const std::vector<int32_t> length = in.many<int32_t>(static_cast<size_t>(v.n_games));
    const std::vector<float> priorities = in.many<float>(static_cast<size_t>(v.n_games) * v.stride);
    v.game_priority = game_priority.data();
    v.length = length.data();
    v.priorities = priorities.data();
    std::vector<uint32_t> key(mz::kMtN);
    int32_t pos;
    mz::mt_seed(key.data(), &pos, seed);
    uint64_t words = 0;
    const size_t U1 = static_cast<size_t>(v.unroll) + 1;
    std::vector<int32_t> game_index(batch), position(batch), absorbing(batch * U1);
    std::vector<float> weight(batch), probs(v.n_games);
    std::vector<double> cdf(static_cast<size_t>(v.n_games > v.stride ? v.n_games : v.stride));
    mz::replay::sample_batch_serial(v, per != 0, batch, key.data(), &pos, &words, game_index.data(), position.data(),
                                    absorbing.data(), weight.data(), probs.data(), cdf.data());
    auto same = [](auto x) { return x; };
    std::printf("{");
    print_list("game_index", game_index, same);
    print_list("position", position, same);
    print_list("absorbing", absorbing, same);
    print_list("weight", weight, bits);
    print_list("key", key, same);
    std::printf("\"pos\": %d, \"words\": %llu}\n", pos, static_cast<unsigned long long>(words));
    return 0;
}

int run_update(Reader& in) {
    const int n_games = in.one<int32_t>();
    const int stride = in.one<int32_t>();
    const int steps = in.one<int32_t>();
    const int batch = in.one<int32_t>();
    const int64_t oldest = in.one<int64_t>();
    const std::vector<int32_t> length = in.many<int32_t>(static_cast<size_t>(n_games));
    std::vector<float> priorities = in.many<float>(static_cast<size_t>(n_games) * stride);
    const std::vector<int64_t> game_ids = in.many<int64_t>(static_cast<size_t>(batch));
    const std::vector<int32_t> positions = in.many<int32_t>(static_cast<size_t>(batch));
    const std::vector<float> fresh = in.many<float>(static_cast<size_t>(batch) * steps);
    std::vector<float> game_priority(n_games, -1.f);
    mz::replay::update_priorities_serial(batch, steps, game_ids.data(), positions.data(), fresh.data(), oldest, n_games,
                                         length.data(), priorities.data(), stride, game_priority.data());
    std::printf("{");
    print_list("priorities", priorities, bits);
    print_list("game_priority", game_priority, bits, true);
    std::printf("}\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: replay_sampler_check sum|batch|update FILE\n");
        return 2;
    }
    Reader in(argv[2]);
    const std::string mode = argv[1];
    if (mode == "sum") return run_sum(in);
    if (mode == "batch") return run_batch(in);
    if (mode == "update") return run_update(in);
    return 2;
}
