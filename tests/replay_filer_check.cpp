// Host-side check of csrc/replay_filer.h (the index arithmetic the device filer of the replay store runs), built and
// driven by tests/test_replay_filer_cpu.py:
//     g++ -O2 -std=c++17 replay_filer_check.cpp
// One call of the filer, stated serially in the order of its launches (count per env, chunked exclusive scan, the call's
// plan and the evicted games' lengths, the walk per env, the counters), from a little-endian binary file:
//     i32 E, M, capacity, max_moves, scan_chunk; i64 counters[4] (next id, stored, total_samples, steps);
//     i32 running_length[E]; i32 slot_length[capacity]; i32 actions[M][E]; u8 done[M][E]
// Answer: one JSON object on the last line -- played[E], finished games in filing order (env, length, id, slot, stored),
// counters[4], running_length[E] afterwards.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "replay_filer.h"

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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader in(argv[1]);
    const int E = in.one<int32_t>(), M = in.one<int32_t>(), G = in.one<int32_t>(), L = in.one<int32_t>();
    const int chunk = in.one<int32_t>();
    mz::filer::Counters before;
    before.next_game_id = in.one<int64_t>();
    before.games_stored = in.one<int64_t>();
    before.total_samples = in.one<int64_t>();
    before.steps_played = in.one<int64_t>();
    std::vector<int32_t> running = in.many<int32_t>(E);
    const std::vector<int32_t> slot_length = in.many<int32_t>(G);
    const std::vector<int32_t> actions = in.many<int32_t>(static_cast<size_t>(M) * E);
    const std::vector<uint8_t> done = in.many<uint8_t>(static_cast<size_t>(M) * E);

    // launch 1: a thread per env
    std::vector<int32_t> played(E), count(E);
    bool overflow = false;
    for (int e = 0; e < E; ++e) {
        played[e] = mz::filer::prefix_length(M, [&](int m) { return actions[static_cast<size_t>(m) * E + e]; });
        int len = running[e];
        count[e] = mz::filer::count_finished(&len, played[e], L, [&](int m) { return done[static_cast<size_t>(m) * E + e] != 0; },
                                             &overflow);
    }
    // launch 2: the scan, the plan, the evicted games
    std::vector<int64_t> offset(E);
    const int64_t n_new = mz::filer::exclusive_scan_chunked(E, chunk, [&](int e) { return count[e]; },
                                                            [&](int e, int64_t v) { offset[e] = v; });
    const mz::filer::Call call = mz::filer::plan_call(before, n_new, G, 0, overflow);
    int64_t evicted_lengths = 0;
    const int64_t evicted = mz::filer::evicted_old(before, call.n_new, G);
    for (int64_t j = 0; j < evicted; ++j)
        evicted_lengths += slot_length[mz::filer::slot_of(mz::filer::first_evicted_id(before) + j, G)];
    // launch 3: a wavefront per env walks its moves
    std::vector<int64_t> g_env(call.n_new), g_len(call.n_new), g_id(call.n_new), g_slot(call.n_new), g_stored(call.n_new);
    int64_t all_lengths = 0, survivor_lengths = 0;
    for (int e = 0; e < E && !call.refused; ++e) {
        int len = running[e];
        int64_t rank = offset[e];
        for (int m = 0; m < played[e]; ++m) {
            ++len;
            if (done[static_cast<size_t>(m) * E + e]) {
                const int j = static_cast<int>(rank++);
                g_env[j] = e;
                g_len[j] = len;
                g_id[j] = mz::filer::game_id(call, j);
                g_slot[j] = mz::filer::slot_of(g_id[j], G);
                g_stored[j] = mz::filer::survives(call, j) ? 1 : 0;
                all_lengths += len;
                if (mz::filer::survives(call, j)) survivor_lengths += len;
                len = 0;
            }
        }
        running[e] = len;
    }
    const mz::filer::Counters after =
        mz::filer::counters_after(before, call.n_new, G, all_lengths, survivor_lengths, evicted_lengths);
    std::printf("{\"refused\": %d, ", call.refused);
    print_list("played", played);
    print_list("env", g_env);
    print_list("length", g_len);
    print_list("id", g_id);
    print_list("slot", g_slot);
    print_list("stored", g_stored);
    print_list("running", running);
    print_list("counters", std::vector<int64_t>{after.next_game_id, after.games_stored, after.total_samples, after.steps_played}, true);
    std::printf("}\n");
    return 0;
}
