// board_rules.h -- the rules of the two board games as __host__ __device__ functions: winner test, legal actions
// and the scripted opponents of evaluation games.  The environment kernels (env_kernels.hip) and a CPU check
// (tests/board_rules_check.cpp) compile this same text.
//
// Boards are int8[cells], 0 empty, +1 first player, -1 second player; tic-tac-toe cell = 3 * row + column,
// connect four cell = 7 * row + column with row 0 at the bottom.  The rules restate this package's host plugins
// (games/tictactoe.py, games/connect4.py), which fixture G11 pins to the reference move by move.  Gomoku's rules
// (11 x 11, cell = 11 * row + column; fixture G18) live in gomoku_rules.h; its scripted opponent is below.
#pragma once
#include <cstdint>

#include "gomoku_rules.h"
#include "np_legacy_rng.h"

namespace mz {

enum OpponentKind : int32_t { kOpponentSelf = 0, kOpponentExpert = 1, kOpponentRandom = 2 };

// ---- tic-tac-toe ------------------------------------------------------------------------------------
MZ_HD inline bool ttt_winner(const int8_t* b, int p) {
    const int t = 3 * p;
    for (int i = 0; i < 3; ++i) {
        if (b[3 * i] + b[3 * i + 1] + b[3 * i + 2] == t) return true;
        if (b[i] + b[i + 3] + b[i + 6] == t) return true;
    }
    return (b[0] + b[4] + b[8] == t) || (b[2] + b[4] + b[6] == t);
}

MZ_HD inline int ttt_legal(const int8_t* b, int32_t* legal) {
    int n = 0;
    for (int i = 0; i < 9; ++i)
        if (b[i] == 0) legal[n++] = i;
    return n;
}

// ---- connect four (row 0 = bottom) ---------------------------------------------------------------------
MZ_HD inline bool c4_winner(const int8_t* b, int p) {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 7; ++c) {
            if (b[r * 7 + c] != p) continue;
            if (c + 3 < 7 && b[r * 7 + c + 1] == p && b[r * 7 + c + 2] == p && b[r * 7 + c + 3] == p) return true;
            if (r + 3 < 6 && b[(r + 1) * 7 + c] == p && b[(r + 2) * 7 + c] == p && b[(r + 3) * 7 + c] == p) return true;
            if (r + 3 < 6 && c + 3 < 7 && b[(r + 1) * 7 + c + 1] == p && b[(r + 2) * 7 + c + 2] == p &&
                b[(r + 3) * 7 + c + 3] == p)
                return true;
            if (r - 3 >= 0 && c + 3 < 7 && b[(r - 1) * 7 + c + 1] == p && b[(r - 2) * 7 + c + 2] == p &&
                b[(r - 3) * 7 + c + 3] == p)
                return true;
        }
    return false;
}

MZ_HD inline int c4_legal(const int8_t* b, int32_t* legal) {
    int n = 0;
    for (int c = 0; c < 7; ++c)
        if (b[35 + c] == 0) legal[n++] = c;
    return n;
}

// numpy.random.choice(legal) on the stream key/pos: one bounded draw (none for a single legal action).  n >= 1.
MZ_HD inline int random_legal_action(const int32_t* legal, int n, uint32_t* key, int32_t* pos, uint32_t* words) {
    return legal[mt_below(key, pos, static_cast<uint32_t>(n), words)];
}

// games/tictactoe.py expert_action: a random legal move first (always drawn), then the eight lines in the order
// row i, column i (i = 0..2), diagonal, anti-diagonal: a line holding two equal stones and a gap names the gap; the
// player's own line wins and returns at once, the other side's is a block that a later line may override.
MZ_HD inline int ttt_expert(const int8_t* b, int player, const int32_t* legal, int n, uint32_t* key, int32_t* pos,
                            uint32_t* words) {
    int action = random_legal_action(legal, n, key, pos, words);
    for (int l = 0; l < 8; ++l) {
        int c0, step;
        if (l < 6) {
            const int i = l >> 1;
            c0 = (l & 1) ? i : 3 * i;
            step = (l & 1) ? 3 : 1;
        } else {
            c0 = (l == 6) ? 0 : 2;
            step = (l == 6) ? 4 : 2;
        }
        const int total = b[c0] + b[c0 + step] + b[c0 + 2 * step];
        if (total != 2 && total != -2) continue;
        for (int i = 0; i < 3; ++i)
            if (b[c0 + i * step] == 0) {
                action = c0 + i * step;
                break;
            }
        if (player * total > 0) return action;
    }
    return action;
}

// stones in column c
MZ_HD inline int c4_height(const int8_t* b, int c) {
    int h = 0;
    for (int r = 0; r < 6; ++r) h += b[r * 7 + c] != 0;
    return h;
}

// games/connect4.py expert_action: a random legal move first (always drawn), then every 4 x 4 window (bottom row k,
// left column l) in the order k = 0..2, l = 0..3; inside a window row i and column i interleaved (i = 0..3), then
// the diagonal and the anti-diagonal.  Three equal stones and a gap: a row or diagonal gap counts only when the
// stone would land there (column height equals the gap's row), a column gap always; the player's own line wins and
// returns at once, the other side's is a block that later lines may override.
MZ_HD inline int c4_expert(const int8_t* b, int player, const int32_t* legal, int n, uint32_t* key, int32_t* pos,
                           uint32_t* words) {
    int action = random_legal_action(legal, n, key, pos, words);
    auto at = [&](int r, int c) { return static_cast<int>(b[r * 7 + c]); };
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 4; ++l) {
            for (int i = 0; i < 4; ++i) {
                const int row_sum = at(k + i, l) + at(k + i, l + 1) + at(k + i, l + 2) + at(k + i, l + 3);
                if (row_sum == 3 || row_sum == -3) {
                    int ind = 0;
                    while (at(k + i, l + ind) != 0) ++ind;
                    if (c4_height(b, ind + l) == i + k) {
                        action = ind + l;
                        if (player * row_sum > 0) return action;
                    }
                }
                const int col_sum = at(k, l + i) + at(k + 1, l + i) + at(k + 2, l + i) + at(k + 3, l + i);
                if (col_sum == 3 || col_sum == -3) {
                    action = i + l;
                    if (player * col_sum > 0) return action;
                }
            }
            const int diag_sum = at(k, l) + at(k + 1, l + 1) + at(k + 2, l + 2) + at(k + 3, l + 3);
            if (diag_sum == 3 || diag_sum == -3) {
                int ind = 0;
                while (at(k + ind, l + ind) != 0) ++ind;
                if (c4_height(b, ind + l) == ind + k) {
                    action = ind + l;
                    if (player * diag_sum > 0) return action;
                }
            }
            const int anti_sum = at(k, l + 3) + at(k + 1, l + 2) + at(k + 2, l + 1) + at(k + 3, l);
            if (anti_sum == 3 || anti_sum == -3) {
                int ind = 0;
                while (at(k + ind, l + 3 - ind) != 0) ++ind;
                if (c4_height(b, 3 - ind + l) == ind + k) {
                    action = 3 - ind + l;
                    if (player * anti_sum > 0) return action;
                }
            }
        }
    return action;
}

// The opponent's move in a position of `game` (1 tic-tac-toe, 2 connect four) with `player` (+1 / -1) to move, drawn
// from the stream key/pos; *words counts the 32-bit words consumed.  A full board has no move: -1, nothing drawn
// (a bounded draw over zero entries would index with a raw 32-bit word).  A position that is won but not full is
// played on like any other: callers reset finished games first.
MZ_HD inline int opponent_action(int game, int kind, const int8_t* b, int player, uint32_t* key, int32_t* pos,
                                 uint32_t* words) {
    int32_t legal[9];
    const int n = (game == 1) ? ttt_legal(b, legal) : c4_legal(b, legal);
    if (n == 0) return -1;
    if (kind == kOpponentRandom) return random_legal_action(legal, n, key, pos, words);
    return (game == 1) ? ttt_expert(b, player, legal, n, key, pos, words) : c4_expert(b, player, legal, n, key, pos, words);
}

// The scripted opponent's move on a Gomoku board, drawn from the stream key/pos.  The reference's Gomoku has no
// expert_agent (AbstractGame.expert_agent raises), so there is one kind: numpy.random.choice over the legal cells, up
// to 121 of them (one legal cell draws no word).  A full board has no move: -1, nothing drawn.
MZ_HD inline int gmk_opponent_action(const int8_t* b, uint32_t* key, int32_t* pos, uint32_t* words) {
    int32_t legal[kGmkCells];
    const int n = gmk_legal(b, legal);
    if (n == 0) return -1;
    return random_legal_action(legal, n, key, pos, words);
}

}  // namespace mz
