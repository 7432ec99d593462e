// Host-side check of csrc/paired_moves.h (the slot rule the environment kernels compile): seeded evaluation games of
// tic-tac-toe and connect four are replayed twice -- one twin through paired_move, one through three single-ply calls
// (MuZero's action, then twice "no action", which on MuZero's turn leaves the env alone and on the opponent's plays the
// opponent: what mzenv_advance_opponent does) -- and compared after every move: board, side to move, ply counter, stream
// key and position, and each slot's record against the corresponding call's.  After every paired move MuZero must be to
// move.  The plies are a host restatement over csrc/board_rules.h; the check is of the slot loop, not of the rules.
// Built and run by tests/test_paired_moves_cpu.py:
//     g++ -O2 -std=c++17 -ffp-contract=off paired_moves_check.cpp
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "board_rules.h"
#include "paired_moves.h"

namespace {

struct Record {
    int played = -1, done = 0;
    float reward = 0.f;
    uint32_t words = 0;
    int8_t after[42] = {};  // the position the slot's observation shows
    int after_player = 0;
    bool operator==(const Record& o) const {
        return played == o.played && done == o.done && reward == o.reward && words == o.words &&
               std::memcmp(after, o.after, sizeof(after)) == 0 && after_player == o.after_player;
    }
};

struct Env {
    int game = 1, kind = mz::kOpponentExpert, muzero = 0, max_moves = 0;
    int8_t board[42] = {};
    int player = 1, steps = 0;
    uint32_t key[mz::kMtN];
    int32_t pos = 0;

    int cells() const { return game == 1 ? 9 : 42; }
    bool opponent_to_move() const { return (player == 1 ? 0 : 1) != muzero; }
    int legal(int32_t* out) const { return game == 1 ? mz::ttt_legal(board, out) : mz::c4_legal(board, out); }
    void reset() {
        std::memset(board, 0, sizeof(board));
        player = 1;
        steps = 0;
    }
    // a single-ply call: step (the opponent chooses on its turn; a < 0 on MuZero's leaves the env alone), the position
    // reached, reset if the game is over
    Record ply(int a) {
        Record r;
        if (opponent_to_move()) a = mz::opponent_action(game, kind, board, player, key, &pos, &r.words);
        bool done = false;
        if (a >= 0) {
            r.played = a;
            ++steps;
            bool won, full = true;
            if (game == 1) {
                board[a] = static_cast<int8_t>(player);
                won = mz::ttt_winner(board, player);
                for (int i = 0; i < 9; ++i) full = full && board[i] != 0;
                r.reward = won ? 20.f : 0.f;
            } else {
                for (int row = 0; row < 6; ++row)
                    if (board[row * 7 + a] == 0) {
                        board[row * 7 + a] = static_cast<int8_t>(player);
                        break;
                    }
                won = mz::c4_winner(board, player);
                for (int c = 0; c < 7; ++c) full = full && board[35 + c] != 0;
                r.reward = won ? 10.f : 0.f;
            }
            done = won || full || (max_moves > 0 && steps >= max_moves);
            player = -player;
        }
        r.done = done ? 1 : 0;
        std::memcpy(r.after, board, sizeof(board));
        r.after_player = player;
        if (done) reset();
        return r;
    }
    bool same_state(const Env& o) const {
        return std::memcmp(board, o.board, sizeof(board)) == 0 && player == o.player && steps == o.steps && pos == o.pos &&
               std::memcmp(key, o.key, sizeof(key)) == 0;
    }
};

struct HostOps {
    Env& env;
    Record slots[mz::kPairedSlots];
    bool opponent_to_move() { return env.opponent_to_move(); }
    void slot(int s, bool play, int a) {
        if (play) {
            slots[s] = env.ply(a);
        } else {
            slots[s] = Record();
            std::memcpy(slots[s].after, env.board, sizeof(env.board));
            slots[s].after_player = env.player;
        }
    }
};

}  // namespace

int main() {
    long moves = 0, plies = 0, bad_state = 0, bad_slot = 0, bad_invariant = 0, slot2_plies = 0, skipped = 0, games = 0;
    for (int game = 1; game <= 2; ++game)
        for (int kind = mz::kOpponentExpert; kind <= mz::kOpponentRandom; ++kind)
            for (int muzero = 0; muzero <= 1; ++muzero)
                for (int limit : {0, 2, 3, 5})
                    for (unsigned seed = 0; seed < 12; ++seed) {
                        Env a;
                        a.game = game, a.kind = kind, a.muzero = muzero, a.max_moves = limit;
                        mz::mt_seed(a.key, &a.pos, 977u * seed + 13u * game + kind);
                        Env b = a;
                        mz::HostStream picks;  // MuZero's own choices: a stream of the check's, not the env's
                        picks.seed(4242u + seed);
                        // the settle call: only the opponent's pending plies
                        {
                            HostOps ops{a};
                            mz::paired_move(ops, -1);
                            Record first = b.ply(-1);
                            if (ops.slots[0].played != -1 || ops.slots[2].played != -1 || !(ops.slots[1] == first) ||
                                (first.played >= 0) != (muzero == 1))
                                ++bad_slot;
                            if (!a.same_state(b)) ++bad_state;
                        }
                        for (int m = 0; m < 60; ++m) {
                            if (a.opponent_to_move()) ++bad_invariant;
                            int32_t legal[9];
                            const int n = a.legal(legal);
                            int action = legal[picks.below(static_cast<uint32_t>(n))];
                            if (picks.below(8u) == 0) action = -1, ++skipped;  // an env left alone, in mid-game too
                            HostOps ops{a};
                            mz::paired_move(ops, action);
                            for (int s = 0; s < mz::kPairedSlots; ++s) {
                                const Record single = b.ply(s == 0 ? action : -1);
                                if (!(ops.slots[s] == single)) ++bad_slot;
                                plies += single.played >= 0;
                                games += single.done;
                            }
                            slot2_plies += ops.slots[2].played >= 0;
                            if (!a.same_state(b)) ++bad_state;
                            ++moves;
                        }
                        if (a.opponent_to_move()) ++bad_invariant;
                    }
    std::printf("{\"moves\": %ld, \"plies\": %ld, \"games\": %ld, \"skipped\": %ld, \"slot2_plies\": %ld, "
                "\"state_mismatches\": %ld, \"slot_mismatches\": %ld, \"invariant_breaks\": %ld}\n",
                moves, plies, games, skipped, slot2_plies, bad_state, bad_slot, bad_invariant);
    return (bad_state || bad_slot || bad_invariant) ? 1 : 0;
}
