// Host-side check of select_action.h (the sampler the GPU runs for temperatures that need pow: glibc's pow restated,
// csrc/glibc_libm.h) against HostStream::select_action (the same rule on this machine's libm, pinned to the reference by
// fixture G8).  Built and run by tests/test_select_action.py:
//     g++ -O2 -std=c++17 -ffp-contract=off -mfma select_action_check.cpp -lm
//
//   select_action_check sweep < rows     every row of stdin ("n v0 v1 ...", one per line) plus generated rows of 2, 4, 7,
//                                        9, 121 and 256 children, at every temperature of the list below, some hundred
//                                        seeds each, three draws per seed: same slot, word count, stream position and
//                                        key block as the host sampler; then visit_weight == std::pow for every visit
//                                        count 0..32767 at those exponents.  Prints one JSON line.
//   select_action_check rows < rows      every line "seed temperature draws n v0 v1 ...": prints the chosen slots of
//                                        `draws` consecutive samples on numpy.random.seed(seed), then the words consumed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include <iostream>

#include "select_action.h"

namespace {

struct Row {
    std::vector<int32_t> visits;
};

// xorshift: the rows only have to be varied, not numpy's
uint32_t next(uint32_t& s) {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}

// rows of n children that sum to `total`: kind 0 spread, 1 many zeros, 2 ties, 3 one dominant child
Row make_row(int n, int total, int kind, uint32_t& s) {
    Row r;
    r.visits.assign(static_cast<size_t>(n), 0);
    if (kind == 2) {
        for (int i = 0; i < total; ++i) r.visits[static_cast<size_t>(i % n)] += 1;
        return r;
    }
    if (kind == 3) {
        const int big = static_cast<int>(next(s) % static_cast<uint32_t>(n));
        const int rest = total / 10;
        r.visits[static_cast<size_t>(big)] = total - rest;
        for (int i = 0; i < rest; ++i) r.visits[next(s) % static_cast<uint32_t>(n)] += 1;
        return r;
    }
    const uint32_t live = static_cast<uint32_t>(kind == 1 ? (n + 3) / 4 : n), stride = static_cast<uint32_t>(n) / live;
    for (int i = 0; i < total; ++i) r.visits[(next(s) % live) * stride] += 1;
    return r;
}

bool same_draws(const Row& row, double temperature, uint32_t seed, int draws) {
    const int n = static_cast<int>(row.visits.size());
    mz::HostStream host;
    host.seed(seed);
    uint32_t key[mz::kMtN];
    std::memcpy(key, host.key, sizeof(key));
    int32_t pos = host.pos;
    std::vector<double> weights(static_cast<size_t>(n));
    for (int d = 0; d < draws; ++d) {
        const uint64_t before = host.words;
        const int want = host.select_action(row.visits.data(), n, temperature);
        uint32_t used = 0;
        const int got = mz::select_action_any([&](int i) { return row.visits[static_cast<size_t>(i)]; }, n, temperature,
                                              weights.data(), key, &pos, &used);
        if (got != want || used != host.words - before || pos != host.pos || std::memcmp(key, host.key, sizeof(key)) != 0)
            return false;
    }
    return true;
}

std::vector<Row> read_rows(std::istream& in) {
    std::vector<Row> rows;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        int n;
        if (!(ss >> n) || n <= 0) continue;
        Row r;
        for (int i = 0, v; i < n && (ss >> v); ++i) r.visits.push_back(v);
        if (static_cast<int>(r.visits.size()) == n) rows.push_back(r);
    }
    return rows;
}

int sweep() {
    // 0.25 leaves the exact path at 32767 visits only (32767 ** 4 > 9e15); 1e25: an exponent below glibc_pow's range
    static const double temperatures[] = {0.35, 0.7, 1.0 / 3.0, 0.2, 0.125, 3.0, 17.5, 0.25, 1e25, 0.5, 1.0, 0.0, INFINITY};
    static const int lengths[] = {2, 4, 7, 9, 121, 256};
    std::vector<Row> rows = read_rows(std::cin);
    const size_t given = rows.size();
    uint32_t s = 2463534242u;
    for (int n : lengths)
        for (int kind = 0; kind < 4; ++kind)
            for (int total : {50, 400, 32767}) rows.push_back(make_row(n, total, kind, s));
    long cases = 0, bad = 0, general = 0;
    for (size_t r = 0; r < rows.size(); ++r) {
        double sum = 0.0;
        for (int32_t v : rows[r].visits) sum += v;
        for (double t : temperatures) {
            // (a power that overflows is refused before any kernel runs: not a case)
            if (!mz::temperature_samplable(t, static_cast<int>(rows[r].visits.size()), sum)) continue;
            const bool is_general = mz::general_temperature(t, sum);
            for (uint32_t seed = 0; seed < 200; ++seed) {
                ++cases;
                general += is_general ? 1 : 0;
                if (!same_draws(rows[r], t, seed * 2654435761u + static_cast<uint32_t>(r), 3)) {
                    if (bad < 5) std::printf("row %zu temperature %g seed %u differs\n", r, t, seed);
                    ++bad;
                }
            }
        }
    }
    // the 1 / k temperature whose powers leave the exact integers must have taken the pow path, the others not
    const bool routed = mz::general_temperature(0.25, 32767.0) && !mz::general_temperature(0.25, 9740.0) &&
                        !mz::general_temperature(0.5, 32767.0) && mz::general_temperature(0.2, 2.0) &&
                        !mz::general_temperature(0.0, 50.0) && !mz::general_temperature(INFINITY, 50.0);
    long powers = 0, pow_bad = 0;
    for (double t : temperatures) {
        if (t == 0.0 || std::isinf(t)) continue;
        const double inv = 1 / t;
        for (int v = 0; v <= 32767; ++v) {
            const double got = mz::visit_weight(v, inv), want = std::pow(static_cast<double>(v), inv);
            ++powers;
            if (std::memcmp(&got, &want, sizeof(double)) != 0) {
                if (pow_bad < 5) std::printf("pow(%d, 1 / %g): %a, libm %a\n", v, t, got, want);
                ++pow_bad;
            }
        }
    }
    // what the move batches refuse: NaN, negative, powers that overflow (50 ** 1e4)
    const bool refused = !mz::temperature_samplable(std::nan(""), 2, 50.0) && !mz::temperature_samplable(-1.0, 2, 50.0) &&
                         !mz::temperature_samplable(1e-4, 2, 50.0) && !mz::temperature_samplable(1e-300, 2, 50.0) &&
                         mz::temperature_samplable(0.35, 121, 400.0) && mz::temperature_samplable(1e300, 2, 50.0);
    std::printf("{\"given_rows\": %zu, \"rows\": %zu, \"cases\": %ld, \"general_cases\": %ld, \"mismatches\": %ld, "
                "\"powers\": %ld, \"pow_mismatches\": %ld, \"routed\": %s, \"refused\": %s}\n",
                given, rows.size(), cases, general, bad, powers, pow_bad, routed ? "true" : "false", refused ? "true" : "false");
    return (bad || pow_bad || !routed || !refused) ? 1 : 0;
}

int replay_rows() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        unsigned long seed;
        std::string temperature;
        int draws, n;
        if (!(ss >> seed >> temperature >> draws >> n)) continue;
        std::vector<int32_t> visits(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) ss >> visits[static_cast<size_t>(i)];
        const double t = std::strtod(temperature.c_str(), nullptr);   // (reads "inf")
        uint32_t key[mz::kMtN];
        int32_t pos;
        mz::mt_seed(key, &pos, static_cast<uint32_t>(seed));
        std::vector<double> weights(static_cast<size_t>(n));
        uint32_t used = 0;
        for (int d = 0; d < draws; ++d)
            std::printf("%d ", mz::select_action_any([&](int i) { return visits[static_cast<size_t>(i)]; }, n, t, weights.data(),
                                                     key, &pos, &used));
        std::printf("%u\n", used);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "rows") == 0) return replay_rows();
    std::fprintf(stderr, "usage: select_action_check sweep|rows < rows\n");
    return 2;
}
