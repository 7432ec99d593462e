// Host-side check of csrc/gomoku_rules.h and the Gomoku opponent of csrc/board_rules.h (the text the environment
// kernels compile): for every position read from stdin
//     seed finished(0|1) n_legal  121 x stone  n_legal x cell
// gmk_finished must equal `finished`, gmk_legal must return the listed cells, and the random opponent on a stream
// seeded `seed` must play legal[choice(n_legal)] with the words consumed, the stream position and the key block equal
// to HostStream's for choice(n_legal) (HostStream is pinned to numpy by fixture G7).  A full board has no move: -1,
// nothing drawn.  The per-stone test is also run on the bordered board the kernels stage in LDS: the stones that start
// a five are counted and printed, so that the caller can compare them with its own count.  With the argument --picks
// every row also prints a line "pick <move> <words> <stream position>": what the opponent did, for a caller that holds
// numpy's own record of the draw.
// Built and run by tests/test_gomoku_cpu.py and tests/test_gomoku_rules_cpu.py:   g++ -O2 -std=c++17 -ffp-contract=off gomoku_rules_check.cpp -lm
#include <cstdio>
#include <cstring>

#include "board_rules.h"

int main(int argc, char** argv) {
    const bool print_picks = argc > 1 && std::strcmp(argv[1], "--picks") == 0;
    long rows = 0, bad_finished = 0, bad_legal = 0, bad_random = 0, bad_stream = 0, bad_full = 0, full_boards = 0, starts = 0;
    unsigned seed;
    int finished, n_want;
    while (std::scanf("%u %d %d", &seed, &finished, &n_want) == 3) {
        int8_t board[mz::kGmkCells];
        for (int i = 0; i < mz::kGmkCells; ++i) {
            int v;
            if (std::scanf("%d", &v) != 1) return 2;
            board[i] = static_cast<int8_t>(v);
        }
        int32_t want[mz::kGmkCells], legal[mz::kGmkCells];
        for (int i = 0; i < n_want; ++i)
            if (std::scanf("%d", &want[i]) != 1) return 2;
        if (mz::gmk_finished(board) != (finished != 0)) ++bad_finished;
        const int n = mz::gmk_legal(board, legal);
        if (n != n_want || std::memcmp(legal, want, sizeof(int32_t) * n) != 0) ++bad_legal;
        int8_t padded[mz::kGmkPadded];
        mz::gmk_pad(board, padded);
        for (int i = 0; i < mz::kGmkCells; ++i) starts += mz::gmk_five_from(padded, mz::gmk_padded_index(i));
        mz::HostStream host;
        host.seed(seed);
        uint32_t key[mz::kMtN];
        std::memcpy(key, host.key, sizeof(key));
        int32_t pos = host.pos;
        uint32_t words = 0;
        const int got = mz::gmk_opponent_action(board, key, &pos, &words);
        if (print_picks) std::printf("pick %d %u %d\n", got, words, pos);
        if (n == 0) {
            ++full_boards;
            if (got != -1 || words != 0 || pos != host.pos || std::memcmp(key, host.key, sizeof(key)) != 0) ++bad_full;
        } else {
            const uint32_t drawn = host.below(static_cast<uint32_t>(n));
            if (words != host.words || pos != host.pos || std::memcmp(key, host.key, sizeof(key)) != 0) ++bad_stream;
            if (got != legal[drawn]) ++bad_random;
        }
        ++rows;
    }
    std::printf("{\"rows\": %ld, \"finished_mismatches\": %ld, \"legal_mismatches\": %ld, \"random_mismatches\": %ld, "
                "\"stream_mismatches\": %ld, \"full_boards\": %ld, \"full_board_mismatches\": %ld, \"five_starts\": %ld}\n",
                rows, bad_finished, bad_legal, bad_random, bad_stream, full_boards, bad_full, starts);
    return (bad_finished || bad_legal || bad_random || bad_stream || bad_full) ? 1 : 0;
}
