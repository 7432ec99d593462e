// Host-side check of csrc/board_rules.h (the text the environment kernels compile): for every position read from stdin
//     game(1|2) player(+1|-1) seed expected_action cells x stone
// the scripted expert's move on a stream seeded `seed` must equal expected_action, and the words consumed and the
// stream position must be HostStream's for choice(n_legal) (HostStream is pinned to numpy by fixture G7); the random
// opponent must pick legal[choice(n_legal)].  Built and run by tests/test_opponent_cpu.py:
//     g++ -O2 -std=c++17 -ffp-contract=off board_rules_check.cpp -lm
#include <cstdio>
#include <cstring>

#include "board_rules.h"

int main() {
    long rows = 0, bad_expert = 0, bad_stream = 0, bad_random = 0;
    int game, player, want;
    unsigned seed;
    while (std::scanf("%d %d %u %d", &game, &player, &seed, &want) == 4) {
        const int cells = game == 1 ? 9 : 42;
        int8_t board[42];
        for (int i = 0; i < cells; ++i) {
            int v;
            if (std::scanf("%d", &v) != 1) return 2;
            board[i] = static_cast<int8_t>(v);
        }
        int32_t legal[9];
        const int n = game == 1 ? mz::ttt_legal(board, legal) : mz::c4_legal(board, legal);
        mz::HostStream host;
        host.seed(seed);
        uint32_t key[mz::kMtN];
        for (int kind = mz::kOpponentExpert; kind <= mz::kOpponentRandom; ++kind) {
            host.seed(seed);
            std::memcpy(key, host.key, sizeof(key));
            int32_t pos = host.pos;
            uint32_t words = 0;
            const int got = mz::opponent_action(game, kind, board, player, key, &pos, &words);
            const uint32_t drawn = host.below(static_cast<uint32_t>(n));
            if (words != host.words || pos != host.pos || std::memcmp(key, host.key, sizeof(key)) != 0) ++bad_stream;
            if (kind == mz::kOpponentExpert && got != want) ++bad_expert;
            if (kind == mz::kOpponentRandom && got != legal[drawn]) ++bad_random;
        }
        ++rows;
    }
    // a full board has no move: -1, no word drawn, the stream untouched (both games, both kinds)
    long bad_full = 0;
    for (int full_game = 1; full_game <= 2; ++full_game)
        for (int kind = mz::kOpponentExpert; kind <= mz::kOpponentRandom; ++kind) {
            int8_t board[42];
            for (int i = 0; i < 42; ++i) board[i] = static_cast<int8_t>((i / 2) % 2 ? 1 : -1);
            mz::HostStream host;
            host.seed(5);
            uint32_t key[mz::kMtN];
            std::memcpy(key, host.key, sizeof(key));
            int32_t pos = host.pos;
            uint32_t words = 0;
            if (mz::opponent_action(full_game, kind, board, 1, key, &pos, &words) != -1 || words != 0 || pos != host.pos ||
                std::memcmp(key, host.key, sizeof(key)) != 0)
                ++bad_full;
        }
    std::printf("{\"rows\": %ld, \"expert_mismatches\": %ld, \"stream_mismatches\": %ld, \"random_mismatches\": %ld, "
                "\"full_board_mismatches\": %ld}\n", rows, bad_expert, bad_stream, bad_random, bad_full);
    return (bad_expert || bad_stream || bad_random || bad_full) ? 1 : 0;
}
