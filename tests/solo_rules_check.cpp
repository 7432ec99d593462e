// Host-side run of csrc/solo_rules.h (the text the environment kernels compile for TwentyOne and SimpleGrid).  Every
// line of stdin is one env played the way mzenv_advance plays it -- ply, reset of a finished game --:
//     T seed max_moves n  a_0 .. a_{n-1}      TwentyOne(seed): constructor, reset(), then n plies
//     G max_moves n  a_0 .. a_{n-1}           SimpleGrid from (0, 0)
// and is answered by one line of integers:
//     T:  ctor_player ctor_dealer ctor_words ctor_pos  first_player first_dealer first_words first_pos, then per ply
//         player dealer reward done words pos ply  next_player next_dealer reset_words next_pos
//     G:  per ply  row col reward done ply  next_row next_col
// (hands / position after the ply, words the ply drew and the stream position after it, the ply's number in its game,
// then the state, the reset's words and the position after the reset that follows a finished game).  An action below
// zero leaves the env alone, as the kernels do: the line repeats the state, with 0 words and the ply count unchanged.
// max_moves as in mzenv_set_max_moves (0 = none).  The caller compares with fixture G23 and with the host plugins.
// Built and run by tests/test_solo_games_cpu.py:   g++ -O2 -std=c++17 -ffp-contract=off solo_rules_check.cpp -lm
// Stand-alone: it can be built once more with -fsanitize=address,undefined and run by hand on the same input.
#include <cstdio>
#include <vector>

#include "solo_rules.h"

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind != 'T' && kind != 'G') return 2;
        const int game = kind == 'T' ? mz::kGameTwentyOne : mz::kGameSimpleGrid;
        unsigned seed = 0;
        int max_moves, n;
        if (kind == 'T' && std::scanf("%u", &seed) != 1) return 2;
        if (std::scanf("%d %d", &max_moves, &n) != 2 || n < 0) return 2;
        std::vector<int> actions(n);
        for (int& a : actions)
            if (std::scanf("%d", &a) != 1) return 2;
        std::vector<uint32_t> key(mz::kMtN, 0u);
        int32_t pos = 0, state[mz::kSoloState] = {0, 0};
        uint32_t words = 0;
        if (kind == 'T') {
            mz::t21_construct(state, key.data(), &pos, seed, &words);
            std::printf("%d %d %u %d ", state[0], state[1], words, pos);
        }
        words = 0;
        mz::solo_reset(game, state, key.data(), &pos, &words);
        if (kind == 'T') std::printf("%d %d %u %d ", state[0], state[1], words, pos);
        int steps = 0;
        for (int a : actions) {
            int reward = 0;
            bool done = false;
            words = 0;
            if (a >= 0) {
                ++steps;
                done = mz::solo_ply(game, state, a, steps, max_moves, key.data(), &pos, &words, &reward);
            }
            if (kind == 'T')
                std::printf("%d %d %d %d %u %d %d ", state[0], state[1], reward, done ? 1 : 0, words, pos, steps);
            else
                std::printf("%d %d %d %d %d ", state[0], state[1], reward, done ? 1 : 0, steps);
            words = 0;
            if (done) {
                mz::solo_reset(game, state, key.data(), &pos, &words);
                steps = 0;
            }
            if (kind == 'T')
                std::printf("%d %d %u %d ", state[0], state[1], words, pos);
            else
                std::printf("%d %d ", state[0], state[1]);
        }
        std::printf("\n");
    }
    return 0;
}
