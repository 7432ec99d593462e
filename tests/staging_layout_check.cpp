// Host build of csrc/staging_layout.h for tests/test_staging_layout_cpu.py (g++ -Wall -Werror; once more under ASan + UBSan).
//   staging_layout_check offsets            "E A M" triples on stdin -> one line of numbers per triple: every offset, size and
//                                           stride of the five layouts, the offsets taken from the typed pointers views() hands out
//   staging_layout_check roundtrip E A M    a distinct value through every typed pointer of every block into plain byte vectors
//                                           of exactly the layouts' sizes, then all of them read back
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "staging_layout.h"

namespace mz {
struct MinMax {
    double minimum, maximum;
};
static_assert(sizeof(MinMax) == kMinMaxBytes, "MinMax");
}  // namespace mz

static uint8_t* const kBase = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);   // (never dereferenced: offsets only)
template <typename T>
static size_t at(const T* p) { return static_cast<size_t>(reinterpret_cast<const uint8_t*>(p) - kBase); }
template <typename T>
static void put(const T* p) { std::printf(" %zu", at(p)); }
static void put(size_t v) { std::printf(" %zu", v); }

static int offsets() {
    size_t E, A, M;
    while (std::scanf("%zu %zu %zu", &E, &A, &M) == 3) {
        std::printf("%zu %zu %zu", E, A, M);
        const mz::UploadLayout up(E, A);
        const mz::UploadBlock u = up.views(kBase);
        put(u.legal), put(u.num_legal), put(u.to_play), put(u.rng_skip), put(u.noise), put(up.bytes), put(up.bytes_no_noise());
        const mz::DownloadLayout down(E);
        const mz::DownloadBlock d = down.views(kBase);
        put(d.root_value_sum), put(d.min_max), put(d.depth_sum), put(d.root_predicted), put(d.max_depth), put(d.tie_words);
        put(d.noise_words), put(d.error_flag), put(down.bytes);
        const mz::MoveControlLayout ctl(E, A, M);
        const mz::MoveControlBlock c = ctl.views(kBase);
        put(c.noise), put(c.rng_skip), put(c.temperature), put(c.move_limit), put(c.expected_ties), put(ctl.bytes);
        const mz::MoveOutputLayout out(E, A);
        const mz::MoveOutputBlock o = out.views(kBase, 0), o2 = out.views(kBase, M - 1);
        put(o.actions), put(o.visits), put(o.root_value_sum), put(o.root_predicted), put(o.max_depth), put(o.tie_words);
        put(o.sample_words), put(o.depth_sum), put(out.stride);
        const mz::MoveInputsLayout in(E, A);
        const mz::MoveInputsBlock i = in.views(kBase, 0), i2 = in.views(kBase, M - 1);
        put(i.num_legal), put(i.to_play), put(i.noise_words), put(i.legal), put(in.stride);
        std::printf("\n");
        // the members are what views() uses, and move m's block starts m strides on
        const bool same = at(u.noise) == up.noise && at(d.error_flag) == down.error_flag && at(c.expected_ties) == ctl.expected_ties &&
                          at(o2.depth_sum) == out.stride * (M - 1) + out.depth_sum && at(o2.actions) == out.stride * (M - 1) &&
                          at(i2.legal) == in.stride * (M - 1) + in.legal;
        if (!same) return std::fprintf(stderr, "views() and the layout's members disagree at %zu %zu %zu\n", E, A, M), 1;
    }
    return 0;
}

// field `id` of a block: element i holds a value no other element of the block holds
static int g_bad = 0;
template <typename T>
static T value(int id, size_t i) { return static_cast<T>(id * 100000 + static_cast<int>(i)); }
template <>
mz::MinMax value<mz::MinMax>(int id, size_t i) { return {value<double>(id, i), -value<double>(id, i)}; }
template <typename T>
static void fill(T* p, size_t n, int id) {
    for (size_t i = 0; i < n; ++i) p[i] = value<T>(id, i);
}
template <typename T>
static void expect(const T* p, size_t n, int id) {
    for (size_t i = 0; i < n; ++i) {
        const T want = value<T>(id, i);
        if (std::memcmp(&p[i], &want, sizeof(T)) != 0) ++g_bad;
    }
}
static int roundtrip(size_t E, size_t A, size_t M) {
    const mz::UploadLayout up(E, A);
    const mz::DownloadLayout down(E);
    const mz::MoveControlLayout ctl(E, A, M);
    const mz::MoveOutputLayout out(E, A);
    const mz::MoveInputsLayout in(E, A);
    std::vector<uint8_t> b_up(up.bytes), b_down(down.bytes), b_ctl(ctl.bytes), b_out(out.stride * M), b_in(in.stride * M);
    auto each_field = [&](auto f) {
        const mz::UploadBlock u = up.views(b_up.data());
        f(u.legal, E * A, 1), f(u.num_legal, E, 2), f(u.to_play, E, 3), f(u.rng_skip, E, 4), f(u.noise, E * A, 5);
        const mz::DownloadBlock d = down.views(b_down.data());
        f(d.root_value_sum, E, 1), f(d.min_max, E, 2), f(d.depth_sum, E, 3), f(d.root_predicted, E, 4), f(d.max_depth, E, 5);
        f(d.tie_words, E, 6), f(d.noise_words, E, 7), f(d.error_flag, 4, 8);
        const mz::MoveControlBlock c = ctl.views(b_ctl.data());
        f(c.noise, M * E * A, 1), f(c.rng_skip, M * E, 2), f(c.temperature, E, 3), f(c.move_limit, E, 4), f(c.expected_ties, E, 5);
        for (size_t m = 0; m < M; ++m) {
            const int k = static_cast<int>(10 * (m + 1));
            const mz::MoveOutputBlock o = out.views(b_out.data(), m);
            f(o.actions, E, k + 1), f(o.visits, E * A, k + 2), f(o.root_value_sum, E, k + 3), f(o.root_predicted, E, k + 4);
            f(o.max_depth, E, k + 5), f(o.tie_words, E, k + 6), f(o.sample_words, E, k + 7), f(o.depth_sum, E, k + 8);
            const mz::MoveInputsBlock i = in.views(b_in.data(), m);
            f(i.num_legal, E, k + 1), f(i.to_play, E, k + 2), f(i.noise_words, E, k + 3), f(i.legal, E * A, k + 4);
        }
    };
    each_field([](auto* p, size_t n, int id) { fill(p, n, id); });
    each_field([](auto* p, size_t n, int id) { expect(p, n, id); });
    std::printf("{\"fields\": %zu, \"bad\": %d}\n", 18 + 12 * M, g_bad);
    return g_bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "offsets")) return offsets();
    if (argc == 5 && !std::strcmp(argv[1], "roundtrip"))
        return roundtrip(std::strtoul(argv[2], nullptr, 10), std::strtoul(argv[3], nullptr, 10), std::strtoul(argv[4], nullptr, 10));
    std::fprintf(stderr, "usage: staging_layout_check offsets < shapes | roundtrip E A M\n");
    return 2;
}
