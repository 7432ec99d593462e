// Host-side check of np_legacy_rng.h DeviceStream (the Dirichlet sampler the GPU runs: glibc's log / pow restated,
// csrc/glibc_libm.h) against HostStream (the same sampler on this machine's libm, pinned to numpy by fixture G7):
// identical rows, word counts and stream positions over many seeds, shapes and row lengths.  Built and run by
// tests/test_glibc_libm.py:  g++ -O2 -std=c++17 -ffp-contract=off -mfma device_stream_check.cpp -lm
//
// `device_stream_check windows` (tests/test_device_stream_cpu.py) holds the WINDOWED form to the window-less one -- the form
// root_noise_kernel and move_inputs_kernel (csrc/mcts_kernels.hip) draw through: a copy of the untempered words
// key[pos, pos + ahead) in fast memory, ahead clipped to the block.  stdin:
//     alpha k n_lengths length...            (one line)
//     pos key[0] ... key[623]                (one stream state per line, key words in hex)
// Every state is drawn from with a window of every given length (clipped to 624 - pos as the kernels clip it; the array
// is allocated at exactly that length, so that a sanitizer sees an index outside it), with no window, and on HostStream;
// rows (bits), pos, words and the key block afterwards must agree.  stdout, per state: pos, words, the row's bits and
// the key block after the draw through the LAST length's window, for the caller to hold against numpy; then the counts.
#include <cstdio>
#include <cstring>
#include <vector>

#include "np_legacy_rng.h"

namespace {

constexpr int kMaxRow = 256;

// what the kernels stage: `ahead` words, never past the block's end
int staged_words(int pos, int length) { return mz::kMtN - pos < length ? mz::kMtN - pos : length; }

struct Drawn {
    std::vector<uint32_t> key;
    int32_t pos;
    uint32_t words;
    double row[kMaxRow];
    bool same(const Drawn& o, int k) const {
        return std::memcmp(row, o.row, sizeof(double) * k) == 0 && pos == o.pos && words == o.words && key == o.key;
    }
};

// length < 0: no window at all (device_dirichlet_kernel's form)
void draw_device(const std::vector<uint32_t>& key, int pos, double alpha, int k, int length, Drawn* out) {
    out->key = key;                                               // (heap, exactly 624 words)
    std::memset(out->row, 0, sizeof(out->row));
    if (length < 0) {
        mz::DeviceStream stream{out->key.data(), pos, 0u, nullptr, 0, 0};
        stream.dirichlet(alpha, k, out->row);
        out->pos = stream.pos;
        out->words = stream.words;
        return;
    }
    const int ahead = staged_words(pos, length);
    uint32_t* window = new uint32_t[ahead > 0 ? ahead : 0];
    for (int i = 0; i < ahead; ++i) window[i] = out->key[pos + i];
    mz::DeviceStream stream{out->key.data(), pos, 0u, window, pos, pos + (ahead > 0 ? ahead : 0)};
    stream.dirichlet(alpha, k, out->row);
    out->pos = stream.pos;
    out->words = stream.words;
    delete[] window;
}

int check_windows() {
    double alpha;
    int k, n_lengths;
    if (std::scanf("%lf %d %d", &alpha, &k, &n_lengths) != 3 || k < 1 || k > kMaxRow || n_lengths < 1) return 2;
    std::vector<int> lengths(n_lengths);
    for (int& v : lengths)
        if (std::scanf("%d", &v) != 1 || v < 0) return 2;
    long states = 0, draws = 0, bad_window = 0, bad_host = 0;
    int pos;
    std::vector<uint32_t> key(mz::kMtN);
    Drawn plain, windowed;
    while (std::scanf("%d", &pos) == 1) {
        if (pos < 0 || pos > mz::kMtN) return 2;
        for (uint32_t& w : key)
            if (std::scanf("%x", &w) != 1) return 2;
        draw_device(key, pos, alpha, k, -1, &plain);
        mz::HostStream host;
        std::memcpy(host.key, key.data(), sizeof(host.key));
        host.pos = pos;
        double want[kMaxRow];
        host.dirichlet(alpha, k, want);
        if (std::memcmp(want, plain.row, sizeof(double) * k) != 0 || host.pos != plain.pos || host.words != plain.words ||
            std::memcmp(host.key, plain.key.data(), sizeof(host.key)) != 0) {
            if (bad_host < 5) std::fprintf(stderr, "pos %d: window-less DeviceStream differs from HostStream\n", pos);
            ++bad_host;
        }
        for (int length : lengths) {
            draw_device(key, pos, alpha, k, length, &windowed);
            ++draws;
            if (!windowed.same(plain, k)) {
                if (bad_window < 5) std::fprintf(stderr, "pos %d window %d: differs from the window-less draw\n", pos, length);
                ++bad_window;
            }
        }
        std::printf("%d %u", windowed.pos, windowed.words);
        for (int j = 0; j < k; ++j) {
            uint64_t bits;
            std::memcpy(&bits, &windowed.row[j], sizeof(bits));
            std::printf(" %llx", static_cast<unsigned long long>(bits));
        }
        for (uint32_t w : windowed.key) std::printf(" %x", w);
        std::printf("\n");
        ++states;
    }
    std::printf("{\"states\": %ld, \"window_draws\": %ld, \"window_mismatches\": %ld, \"host_mismatches\": %ld}\n", states, draws,
                bad_window, bad_host);
    return (bad_window || bad_host) ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "windows") == 0) return check_windows();
    static const double alphas[] = {0.25, 0.1, 0.3, 0.03, 0.5, 0.9, 1.0};
    static const int lengths[] = {2, 4, 7, 9, 18, 121};
    long rows = 0, bad = 0;
    for (unsigned seed = 0; seed < 400; ++seed) {
        for (double alpha : alphas) {
            for (int k : lengths) {
                mz::HostStream host;
                host.seed(seed * 2654435761u + 17u);
                uint32_t key[mz::kMtN];
                std::memcpy(key, host.key, sizeof(key));
                mz::DeviceStream dev{key, host.pos, 0u, nullptr, 0, 0};
                double want[121], got[121];
                for (int draw = 0; draw < 3; ++draw) {                 // (three draws: the 624-word block is regenerated on the way)
                    const uint64_t before = host.words;
                    host.dirichlet(alpha, k, want);
                    const uint32_t dev_before = dev.words;
                    dev.dirichlet(alpha, k, got);
                    ++rows;
                    if (std::memcmp(want, got, sizeof(double) * k) != 0 || host.words - before != dev.words - dev_before ||
                        host.pos != dev.pos || std::memcmp(host.key, key, sizeof(key)) != 0) {
                        if (bad < 5) std::printf("seed %u alpha %g k %d draw %d differs\n", seed, alpha, k, draw);
                        ++bad;
                    }
                }
            }
        }
    }
    std::printf("{\"rows\": %ld, \"mismatches\": %ld}\n", rows, bad);
    return bad ? 1 : 0;
}
