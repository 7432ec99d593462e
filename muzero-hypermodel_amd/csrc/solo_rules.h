// solo_rules.h -- the two one-player games that need nothing but numpy: TwentyOne and SimpleGrid.
//
// Rules restated from the behaviour of the reference's games/twentyone.py:227-299 and games/simple_grid.py:190-227,
// with the Game wrappers' reward scaling (x10 in both).  Host and device compile this text: env_kernels.hip runs it one
// thread per env, tests/solo_rules_check.cpp replays fixture G23 through it with g++.  No HIP include.
//
// TwentyOne is the one game whose transition is stochastic: a card is `RandomState.randint(1, 13)` on the env's own
// MT19937 stream, which is 1 + mt_below(key, pos, 12, words) -- one 32-bit word per attempt, `word & 15`, accepted at
// 11 or less -- so a ply consumes a variable number of words (a hit: one card; a stand: as many as the dealer needs).
#pragma once
#include <cstdint>

#include "np_legacy_rng.h"

namespace mz {

constexpr int kGameTwentyOne = 5;   // include/mzenv.h MZENV_TWENTYONE
constexpr int kGameSimpleGrid = 6;  // include/mzenv.h MZENV_SIMPLEGRID
constexpr int kSoloState = 2;       // TwentyOne: player_hand, dealer_hand;  SimpleGrid: row, col
constexpr int kGridSize = 3;

MZ_HD inline bool solo_game(int game) { return game == kGameTwentyOne || game == kGameSimpleGrid; }

// ---- TwentyOne ------------------------------------------------------------------------------------------------------
// deal_card_value: cards 1..12, the three highest count 10 (an ace is always 1)
MZ_HD inline int t21_card(uint32_t* key, int32_t* pos, uint32_t* words) {
    const int card = 1 + static_cast<int>(mt_below(key, pos, 12u, words));
    return card >= 10 ? 10 : card;
}

// TwentyOne(seed): seeds the stream and deals two cards that reset() then replaces -- two DRAWS (with their
// rejections), not two words
MZ_HD inline void t21_construct(int32_t* hands, uint32_t* key, int32_t* pos, uint32_t seed, uint32_t* words) {
    mt_seed(key, pos, seed);
    hands[0] = t21_card(key, pos, words);
    hands[1] = t21_card(key, pos, words);
}

// reset(): the player's card first, then the dealer's
MZ_HD inline void t21_reset(int32_t* hands, uint32_t* key, int32_t* pos, uint32_t* words) {
    hands[0] = t21_card(key, pos, words);
    hands[1] = t21_card(key, pos, words);
}

// Game.step(a): a == 0 hits, a == 1 stands.  Returns done; *reward is the wrapper's (x10).
MZ_HD inline bool t21_step(int32_t* hands, int a, uint32_t* key, int32_t* pos, uint32_t* words, int* reward) {
    if (a == 0) hands[0] += t21_card(key, pos, words);
    const bool busted = hands[0] > 21;
    const bool done = busted || a == 1 || hands[0] == 21;
    *reward = 0;
    if (!done) return false;
    if (!busted)
        while (hands[1] <= 16) hands[1] += t21_card(key, pos, words);
    const int player = hands[0], dealer = hands[1];
    if (busted)
        *reward = -10;
    else if (dealer < player || dealer > 21)
        *reward = 10;
    else if (dealer == player)
        *reward = 0;
    else
        *reward = -10;
    return true;
}

// observation (3,3,3): a plane of player_hand, a plane of dealer_hand, a plane of zeros
MZ_HD inline void t21_observe(const int32_t* hands, float* o) {
    for (int i = 0; i < 9; ++i) {
        o[i] = static_cast<float>(hands[0]);
        o[9 + i] = static_cast<float>(hands[1]);
        o[18 + i] = 0.f;
    }
}

// ---- SimpleGrid -----------------------------------------------------------------------------------------------------
MZ_HD inline void grid_reset(int32_t* rc) { rc[0] = rc[1] = 0; }

// a == 0 moves down, a == 1 right; a move GridEnv.legal_actions() does not allow (or any other action) moves nothing
MZ_HD inline bool grid_step(int32_t* rc, int a, int* reward) {
    if (a == 0 && rc[0] != kGridSize - 1)
        ++rc[0];
    else if (a == 1 && rc[1] != kGridSize - 1)
        ++rc[1];
    const bool goal = rc[0] == kGridSize - 1 && rc[1] == kGridSize - 1;
    *reward = goal ? 10 : 0;
    return goal;
}

// observation (1,1,9): one-hot of 3 * row + col
MZ_HD inline void grid_observe(const int32_t* rc, float* o) {
    const int at = kGridSize * rc[0] + rc[1];
    for (int i = 0; i < kGridSize * kGridSize; ++i) o[i] = i == at ? 1.f : 0.f;
}

// ---- one ply of either game, the move limit included -----------------------------------------------------
// `steps` is the env's ply count with this ply in it.  The limit decides only whether the GAME is over: a TwentyOne hit
// that it ends without bust or 21 is no stand -- the dealer does not play, no word is drawn, the reward stays 0 (the
// reference's limit lives in play_game's loop, which never tells the game).
MZ_HD inline bool solo_ply(int game, int32_t* state, int a, int steps, int max_moves, uint32_t* key, int32_t* pos,
                           uint32_t* words, int* reward) {
    const bool done = game == kGameTwentyOne ? t21_step(state, a, key, pos, words, reward) : grid_step(state, a, reward);
    return done || (max_moves > 0 && steps >= max_moves);
}

MZ_HD inline void solo_reset(int game, int32_t* state, uint32_t* key, int32_t* pos, uint32_t* words) {
    if (game == kGameTwentyOne)
        t21_reset(state, key, pos, words);
    else
        grid_reset(state);
}

MZ_HD inline void solo_observe(int game, const int32_t* state, float* o) {
    if (game == kGameTwentyOne)
        t21_observe(state, o);
    else
        grid_observe(state, o);
}

}  // namespace mz
