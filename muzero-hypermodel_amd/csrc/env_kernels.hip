// env_kernels.hip -- device-resident batched game environments (include/mzenv.h).
//
// One thread per env: a move is a handful of byte operations per game, far below any roofline that
// matters; what these kernels buy is that E games advance without E host-side Python calls per move.
// Gomoku's 121 cells do not fit that shape: its kernels (further down) give an env a wavefront and a lane two cells.
// TwentyOne and SimpleGrid (solo_rules.h, shared with a CPU check) take the same shape; TwentyOne's plies draw cards from the env's stream.
// Rules restate the reference's in-repo envs (games/tictactoe.py:242-305, games/connect4.py:219-304)
// with the Game wrappers' reward scaling; CartPole restates the classic-control equations (pinned to them bit for bit but for sin / cos: include/mzenv.h).  The board rules
// and the scripted opponents of evaluation games live in board_rules.h (also compiled for the host by a CPU check).
// Paired moves (mzenv_advance_paired: MuZero's ply and the opponent's replies in one launch) wrap the same ply functions in
// the slot loop of paired_moves.h, one wrapper per kernel form.
#include <hip/hip_runtime.h>

#include "board_rules.h"
#include "env_layout.h"
#include "np_legacy_rng.h"
#include "paired_moves.h"
#include "solo_rules.h"

namespace mz {

// games 1..3 keep a board and a player to move (and can face a scripted opponent); 0, 5 and 6 are one-player games
// with a state of their own (4 is no game: include/mzenv.h)
__device__ __forceinline__ bool board_game(int game) { return game >= 1 && game <= 3; }

__device__ __forceinline__ double mt_uniform(uint32_t* key, int32_t* pos) {
    const int32_t a = static_cast<int32_t>(mt_next(key, pos) >> 5);
    const int32_t b = static_cast<int32_t>(mt_next(key, pos) >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

__device__ __forceinline__ void env_reset_one(const EnvParams& p, int e) {
    if (p.game == 0) {
        // numpy RandomState(seed).uniform(-0.05, 0.05, size=4): low + (high - low) * random_sample()
        uint32_t* key = p.mt_key + static_cast<size_t>(e) * kMtN;
        int32_t pos = p.mt_pos[e];
        for (int i = 0; i < 4; ++i) p.state[4 * e + i] = -0.05 + (0.05 - -0.05) * mt_uniform(key, &pos);
        p.mt_pos[e] = pos;
    } else if (solo_game(p.game)) {
        // TwentyOne.reset() deals two fresh cards from the env's stream; GridEnv.reset() goes back to (0, 0)
        int32_t pos = p.game == kGameTwentyOne ? p.mt_pos[e] : 0;
        uint32_t words = 0;
        solo_reset(p.game, p.solo + kSoloState * e, p.mt_key + static_cast<size_t>(e) * kMtN, &pos, &words);
        if (words) p.mt_pos[e] = pos;
    } else {
        int8_t* b = p.board + static_cast<size_t>(e) * p.cells;
        for (int i = 0; i < p.cells; ++i) b[i] = 0;
        p.player[e] = 1;
    }
    p.steps[e] = 0;
}

// Opponent mode (mzenv_set_opponent): is the side to move in env e the scripted opponent's?
__device__ __forceinline__ bool opponent_to_move(const EnvParams& p, int e) {
    return p.opp_kind != kOpponentSelf && (p.player[e] == 1 ? 0 : 1) != p.opp_player;
}

// One move of env e; returns whether the game ended: by its own rules, or (mzenv_set_max_moves) because this was the
// last ply the move limit allows -- reward and position are the ply's own either way.  a < 0: the env is left alone
// this move (e.g. its search was not run) -- nothing happened, no ply is counted.  On the opponent's turn the incoming action is ignored: the opponent chooses,
// drawing from env e's stream (select_opponent_action, self_play.py:189-221).  played_out / words_out (null outside
// opponent mode): the action actually played (-1: none) and the stream words the choice consumed.
__device__ __forceinline__ bool env_step_one(const EnvParams& p, int e, int a, float* __restrict__ reward_out,
                                             uint8_t* __restrict__ done_out, int32_t* __restrict__ played_out = nullptr,
                                             uint32_t* __restrict__ words_out = nullptr) {
    uint32_t words = 0;
    if (board_game(p.game) && opponent_to_move(p, e)) {
        int32_t pos = p.opp_pos[e];
        a = opponent_action(p.game, p.opp_kind, p.board + static_cast<size_t>(e) * p.cells, p.player[e],
                            p.opp_key + static_cast<size_t>(e) * kMtN, &pos, &words);
        if (words) p.opp_pos[e] = pos;
    }
    if (played_out) played_out[e] = a < 0 ? -1 : a;
    if (words_out) words_out[e] = words;
    if (a < 0) {
        reward_out[e] = 0.f;
        done_out[e] = 0;
        return false;
    }
    float reward = 0.f;
    bool done = false;
    const int steps = ++p.steps[e];  // an opponent's ply counts like MuZero's (len(action_history), self_play.py:129-131)
    if (p.game == 0) {
        // classic-control cart-pole, Euler step (games/cartpole.py CartPolePhysics on the host)
        const double gravity = 9.8, mass_cart = 1.0, mass_pole = 0.1, half_length = 0.5, force_mag = 10.0, tau = 0.02;
        double* s = p.state + 4 * e;
        const double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
        const double force = (a == 1) ? force_mag : -force_mag;
        const double total_mass = mass_cart + mass_pole;
        const double pole_ml = mass_pole * half_length;
        const double cos_t = cos(theta), sin_t = sin(theta);
        const double temp = (force + pole_ml * (theta_dot * theta_dot) * sin_t) / total_mass;
        const double theta_acc =
            (gravity * sin_t - cos_t * temp) / (half_length * (4.0 / 3.0 - mass_pole * (cos_t * cos_t) / total_mass));
        const double x_acc = temp - pole_ml * theta_acc * cos_t / total_mass;
        s[0] = x + tau * x_dot;
        s[1] = x_dot + tau * x_acc;
        s[2] = theta + tau * theta_dot;
        s[3] = theta_dot + tau * theta_acc;
        const double theta_limit = 12 * 2 * 3.141592653589793 / 360;
        done = fabs(s[0]) > 2.4 || fabs(s[2]) > theta_limit || steps >= 500;
        reward = 1.0f;
    } else if (solo_game(p.game)) {
        // (a ply draws zero or more cards from the env's stream: the position is stored only when words were consumed)
        int32_t pos = p.game == kGameTwentyOne ? p.mt_pos[e] : 0;
        uint32_t drawn = 0;
        int r = 0;
        done = solo_ply(p.game, p.solo + kSoloState * e, a, steps, p.max_moves, p.mt_key + static_cast<size_t>(e) * kMtN,
                        &pos, &drawn, &r);
        if (drawn) p.mt_pos[e] = pos;
        reward = static_cast<float>(r);
    } else {
        int8_t* b = p.board + static_cast<size_t>(e) * p.cells;
        const int pl = p.player[e];
        bool won, full = true;
        if (p.game == 1) {
            b[a] = static_cast<int8_t>(pl);
            won = ttt_winner(b, pl);
            for (int i = 0; i < 9; ++i) full = full && b[i] != 0;
            reward = won ? 20.f : 0.f;  // Game.step: reward * 20
        } else {
            for (int r = 0; r < 6; ++r)
                if (b[r * 7 + a] == 0) {
                    b[r * 7 + a] = static_cast<int8_t>(pl);
                    break;
                }
            won = c4_winner(b, pl);
            for (int c = 0; c < 7; ++c) full = full && b[35 + c] != 0;
            reward = won ? 10.f : 0.f;  // Game.step: reward * 10
        }
        done = won || full;
        p.player[e] = static_cast<int8_t>(-pl);
    }
    done = done || (p.max_moves > 0 && steps >= p.max_moves);
    reward_out[e] = reward;
    done_out[e] = done ? 1 : 0;
    return done;
}

__device__ __forceinline__ void env_observe_one(const EnvParams& p, int e, float* __restrict__ obs,
                                                int32_t* __restrict__ legal, int32_t* __restrict__ num_legal,
                                                int32_t* __restrict__ to_play) {
    float* o = obs + static_cast<size_t>(e) * p.obs_floats;
    int32_t* l = legal + static_cast<size_t>(e) * p.A;
    if (p.game == 0) {
        for (int i = 0; i < 4; ++i) o[i] = static_cast<float>(p.state[4 * e + i]);
        l[0] = 0;
        l[1] = 1;
        num_legal[e] = 2;
        to_play[e] = 0;
        return;
    }
    if (solo_game(p.game)) {
        solo_observe(p.game, p.solo + kSoloState * e, o);
        l[0] = 0;  // Game.legal_actions() is [0, 1] in every state of both games
        l[1] = 1;
        num_legal[e] = 2;
        to_play[e] = 0;
        return;
    }
    const int8_t* b = p.board + static_cast<size_t>(e) * p.cells;
    const int pl = p.player[e];
    for (int i = 0; i < p.cells; ++i) {
        o[i] = b[i] == 1 ? 1.f : 0.f;
        o[p.cells + i] = b[i] == -1 ? 1.f : 0.f;
        o[2 * p.cells + i] = static_cast<float>(pl);
    }
    const int n = (p.game == 1) ? ttt_legal(b, l) : c4_legal(b, l);
    // opponent mode: an empty legal set is the engine's "this env sits the search out" (the row stays filled)
    num_legal[e] = opponent_to_move(p, e) ? 0 : n;
    to_play[e] = pl == 1 ? 0 : 1;
}

__global__ __launch_bounds__(256) void env_reset_kernel(EnvParams p, const uint8_t* __restrict__ mask) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E || (mask && !mask[e])) return;
    env_reset_one(p, e);
}

// TwentyOne(seeds[e]): the constructor seeds env e's stream and deals two cards (mzenv_create; Game.reset() follows)
__global__ __launch_bounds__(256) void env_construct_kernel(EnvParams p, const uint32_t* __restrict__ seeds) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    int32_t pos = 0;
    uint32_t words = 0;
    t21_construct(p.solo + kSoloState * e, p.mt_key + static_cast<size_t>(e) * kMtN, &pos, seeds[e], &words);
    p.mt_pos[e] = pos;
}

__global__ __launch_bounds__(256) void env_step_kernel(EnvParams p, const int32_t* __restrict__ actions,
                                                       float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                       int32_t* __restrict__ played_out, uint32_t* __restrict__ words_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    env_step_one(p, e, actions[e], reward_out, done_out, played_out, words_out);
}

__global__ __launch_bounds__(256) void env_observe_kernel(EnvParams p, float* __restrict__ obs, int32_t* __restrict__ legal,
                                                          int32_t* __restrict__ num_legal, int32_t* __restrict__ to_play) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    env_observe_one(p, e, obs, legal, num_legal, to_play);
}

// step, observation of the position reached, reset of the envs whose game ended, observation to search next:
// the four steps of one self-play move in one launch (envs are independent: one thread runs all four for its env).
__global__ __launch_bounds__(256) void env_advance_kernel(EnvParams p, const int32_t* __restrict__ actions,
                                                          float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                                          float* __restrict__ obs_after, float* __restrict__ obs_next,
                                                          int32_t* __restrict__ legal, int32_t* __restrict__ num_legal,
                                                          int32_t* __restrict__ to_play, int32_t* __restrict__ played_out,
                                                          uint32_t* __restrict__ words_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    const bool done = env_step_one(p, e, actions[e], reward_out, done_out, played_out, words_out);
    env_observe_one(p, e, obs_after, legal, num_legal, to_play);
    if (done) env_reset_one(p, e);
    env_observe_one(p, e, obs_next, legal, num_legal, to_play);
}

// ---- paired moves (mzenv_advance_paired): MuZero's ply and the opponent's replies in one launch ------------------------
// The per-slot outputs of a paired launch: arrays with a leading slot axis, [kPairedSlots][E]...
struct PairedOut {
    float* reward;      // [3][E]
    uint8_t* done;      // [3][E]
    float* obs_after;   // [3][E][obs_floats]  (an empty slot holds the position as it stood)
    int32_t* played;    // [3][E]              -1 = empty slot
    uint32_t* words;    // [3][E]
};

// an empty slot's scalars, as a single-ply launch writes them for an env it leaves untouched
__device__ __forceinline__ void paired_empty_slot(const PairedOut& out, size_t at) {
    out.played[at] = -1;
    out.words[at] = 0;
    out.reward[at] = 0.f;
    out.done[at] = 0;
}

// the plies of paired_move (paired_moves.h) for the one-thread-per-env games: a slot is env_advance_kernel's body
struct EnvPairedOps {
    const EnvParams& p;
    const PairedOut& out;
    int e;
    int32_t *legal, *num_legal, *to_play;
    __device__ bool opponent_to_move() const { return mz::opponent_to_move(p, e); }
    __device__ void slot(int s, bool play, int a) {
        const size_t at = static_cast<size_t>(s) * p.E;
        bool done = false;
        if (play)
            done = env_step_one(p, e, a, out.reward + at, out.done + at, out.played + at, out.words + at);
        else
            paired_empty_slot(out, at + e);
        env_observe_one(p, e, out.obs_after + at * p.obs_floats, legal, num_legal, to_play);
        if (done) env_reset_one(p, e);
    }
};

__global__ __launch_bounds__(256) void env_advance_paired_kernel(EnvParams p, const int32_t* __restrict__ actions,
                                                                 PairedOut out, float* __restrict__ obs_next,
                                                                 int32_t* __restrict__ legal, int32_t* __restrict__ num_legal,
                                                                 int32_t* __restrict__ to_play) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    EnvPairedOps ops{p, out, e, legal, num_legal, to_play};
    paired_move(ops, actions[e]);
    env_observe_one(p, e, obs_next, legal, num_legal, to_play);
}

// ---- Gomoku: a wavefront owns an env, a lane owns cells -------------------------------------------------------------
// An 11 x 11 board does not fit the one-thread-per-env shape above: 363 strided float stores per observation and lane
// (every store instruction of a wavefront touching 64 different cache lines) and a serial 121 x 4 x 5 line scan.  Here
// the 64 lanes of a wavefront share ONE env: lane l holds cells l and 64 + l (the second for l < 57) in registers,
// four envs make a 256-thread workgroup.
//   line scan     the board is staged once in LDS with its zero border (gomoku_rules.h: 15 x 15 bytes), every lane
//                 runs gmk_five_from on its own cells, the verdict is an __any over the wavefront
//   legal list    __ballot of "my cell is empty" per 64-cell half; a lane's slot is the popcount of the mask bits
//                 below it (plus the first half's count): ascending cell order without a serial loop
//   observations  lane l writes floats l and 64 + l of each 121-float plane: consecutive lanes, consecutive addresses
//   opponent      lane 0 draws the slot from env e's Mersenne stream (the stream is serial); the slot reaches the other
//                 lanes by a register broadcast, and the lane holding that slot's cell names the action by a ballot
// Everything an env shares (player, ply counter, outputs per env) is read by all lanes and written by lane 0.
constexpr int kGmkEnvsPerBlock = 4;
enum GmkOp : int { kGmkReset = 0, kGmkStep = 1, kGmkObserve = 2, kGmkAdvance = 3 };

struct GmkCells {
    int b0, b1;  // this lane's cells l and 64 + l (b1 = a stone of nobody's colour, 2, for the lanes that have none)
};

__device__ __forceinline__ uint64_t gmk_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// observation planes [board == 1, board == -1, player to move] of one env, coalesced
__device__ __forceinline__ void gmk_write_obs(float* __restrict__ o, int lane, GmkCells c, int player) {
    const bool second = lane + 64 < kGmkCells;
    const float turn = static_cast<float>(player);
    o[lane] = c.b0 == 1 ? 1.f : 0.f;
    if (second) o[64 + lane] = c.b1 == 1 ? 1.f : 0.f;
    o[kGmkCells + lane] = c.b0 == -1 ? 1.f : 0.f;
    if (second) o[kGmkCells + 64 + lane] = c.b1 == -1 ? 1.f : 0.f;
    o[2 * kGmkCells + lane] = turn;
    if (second) o[2 * kGmkCells + 64 + lane] = turn;
}

// legal list by ordered compaction; returns the number of empty cells.  slot0 / slot1: where this lane's cells stand
// in the list (meaningful for its empty cells only).
__device__ __forceinline__ int gmk_legal_slots(int lane, GmkCells c, int* slot0, int* slot1) {
    const uint64_t m0 = __ballot(c.b0 == 0), m1 = __ballot(c.b1 == 0);
    const int n0 = __popcll(m0);
    *slot0 = __popcll(m0 & gmk_lanes_below(lane));
    *slot1 = n0 + __popcll(m1 & gmk_lanes_below(lane));
    return n0 + __popcll(m1);
}

__device__ __forceinline__ void gmk_write_observation(const EnvParams& p, int e, int lane, GmkCells c, int player,
                                                      float* __restrict__ obs, int32_t* __restrict__ legal,
                                                      int32_t* __restrict__ num_legal, int32_t* __restrict__ to_play) {
    gmk_write_obs(obs + static_cast<size_t>(e) * (3 * kGmkCells), lane, c, player);
    int slot0, slot1;
    const int n = gmk_legal_slots(lane, c, &slot0, &slot1);
    int32_t* l = legal + static_cast<size_t>(e) * kGmkCells;
    if (c.b0 == 0) l[slot0] = lane;
    if (c.b1 == 0) l[slot1] = 64 + lane;
    if (lane == 0) {
        // opponent mode: an empty legal set is the engine's "this env sits the search out" (the row stays filled)
        const bool opponent = p.opp_kind != kOpponentSelf && (player == 1 ? 0 : 1) != p.opp_player;
        num_legal[e] = opponent ? 0 : n;
        to_play[e] = player == 1 ? 0 : 1;
    }
}

// Game.step of one env by its wavefront; returns whether the game ended (by its rules or by the move limit).  Collective
// over the WORKGROUP: every wavefront of it calls this together (two barriers inside), one without an env or without a
// ply to play with live == false -- it then touches no memory.  c / player: the lanes' cells and the side to move, kept
// up to date in registers.  a < 0 on MuZero's turn: the env is left alone.
__device__ __forceinline__ bool gmk_wave_step(const EnvParams& p, int e, bool live, int lane, int8_t* __restrict__ board,
                                              int8_t* __restrict__ padded, GmkCells& c, int& player, int a,
                                              float* __restrict__ reward_out, uint8_t* __restrict__ done_out,
                                              int32_t* __restrict__ played_out, uint32_t* __restrict__ words_out) {
    const bool second = lane + 64 < kGmkCells;
    uint32_t words = 0;
    if (live && p.opp_kind != kOpponentSelf && (player == 1 ? 0 : 1) != p.opp_player) {
        // the opponent's turn: the incoming action is ignored, numpy.random.choice(legal) decides (random_legal_action's
        // bounded draw; the list it indexes is never written out: entry k is the empty cell whose slot is k)
        int slot0, slot1;
        const int n = gmk_legal_slots(lane, c, &slot0, &slot1);
        int k = -1;
        if (lane == 0 && n > 0) {
            int32_t pos = p.opp_pos[e];
            k = static_cast<int>(mt_below(p.opp_key + static_cast<size_t>(e) * kMtN, &pos, static_cast<uint32_t>(n), &words));
            if (words) p.opp_pos[e] = pos;
        }
        k = __shfl(k, 0);  // (`words` stays lane 0's: lane 0 reports it)
        // the k-th empty cell: at most one lane holds it, in one of its two cells
        const uint64_t hit0 = __ballot(c.b0 == 0 && slot0 == k), hit1 = __ballot(c.b1 == 0 && slot1 == k);
        a = hit0 ? __ffsll(static_cast<unsigned long long>(hit0)) - 1
                 : (hit1 ? 64 + __ffsll(static_cast<unsigned long long>(hit1)) - 1 : -1);  // a full board has no move
    }
    if (live && lane == 0) {
        if (played_out) played_out[e] = a < 0 ? -1 : a;
        if (words_out) words_out[e] = words;
    }
    bool done = false;
    float reward = 0.f;
    const bool moved = live && a >= 0;
    if (moved) {
        // (an action that names no cell owns no lane: no stone is placed and no store leaves the board)
        if (a == lane) {
            c.b0 = player;
            board[lane] = static_cast<int8_t>(player);
        }
        if (second && a == 64 + lane) {
            c.b1 = player;
            board[64 + lane] = static_cast<int8_t>(player);
        }
        // stage the board with its zero border: 256 bytes cleared, then the cells at their padded places
        reinterpret_cast<int32_t*>(padded)[lane] = 0;
    }
    __syncthreads();
    if (moved) {
        padded[gmk_padded_index(lane)] = static_cast<int8_t>(c.b0);
        if (second) padded[gmk_padded_index(64 + lane)] = static_cast<int8_t>(c.b1);
    }
    __syncthreads();
    if (moved) {
        const bool five = gmk_five_from(padded, gmk_padded_index(lane)) ||
                          (second && gmk_five_from(padded, gmk_padded_index(64 + lane)));
        const bool empty = c.b0 == 0 || c.b1 == 0;
        done = __any(five) || !__any(empty);
        reward = done ? 1.f : 0.f;  // the ply that finishes the game, a full-board draw included (no scaling in Game.step)
        const int steps = p.steps[e] + 1;  // an opponent's ply counts like MuZero's (len(action_history))
        done = done || (p.max_moves > 0 && steps >= p.max_moves);
        player = -player;
        if (lane == 0) {
            p.steps[e] = steps;
            p.player[e] = static_cast<int8_t>(player);
        }
    }
    if (live && lane == 0) {
        reward_out[e] = reward;
        done_out[e] = done ? 1 : 0;
    }
    return done;
}

// Game.reset() of one env by its wavefront (cells and side to move in registers follow)
__device__ __forceinline__ void gmk_wave_reset(const EnvParams& p, int e, int lane, int8_t* __restrict__ board, GmkCells& c,
                                               int& player) {
    const bool second = lane + 64 < kGmkCells;
    c.b0 = 0;
    c.b1 = second ? 0 : 2;
    player = 1;
    board[lane] = 0;
    if (second) board[64 + lane] = 0;
    if (lane == 0) {
        p.player[e] = 1;
        p.steps[e] = 0;
    }
}

template <int OP>
__global__ __launch_bounds__(64 * kGmkEnvsPerBlock) void gomoku_env_kernel(
    EnvParams p, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, float* __restrict__ reward_out,
    uint8_t* __restrict__ done_out, float* __restrict__ obs_after, float* __restrict__ obs_next,
    int32_t* __restrict__ legal, int32_t* __restrict__ num_legal, int32_t* __restrict__ to_play,
    int32_t* __restrict__ played_out, uint32_t* __restrict__ words_out) {
    __shared__ __attribute__((aligned(16))) int8_t padded_all[kGmkEnvsPerBlock][256];  // 225 bytes used per env
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    const int e = blockIdx.x * kGmkEnvsPerBlock + group;
    const bool live = e < p.E;  // (a wavefront without an env stays for the workgroup barrier and touches no memory)
    int8_t* padded = padded_all[group];
    const bool second = lane + 64 < kGmkCells;
    int8_t* board = p.board + static_cast<size_t>(live ? e : 0) * kGmkCells;

    if (OP == kGmkReset) {
        if (!live || (mask && !mask[e])) return;
        board[lane] = 0;
        if (second) board[64 + lane] = 0;
        if (lane == 0) {
            p.player[e] = 1;
            p.steps[e] = 0;
        }
        return;
    }

    GmkCells c{2, 2};
    int player = 1;
    if (live) {
        c.b0 = board[lane];
        if (second) c.b1 = board[64 + lane];
        player = p.player[e];
    }
    if (OP == kGmkObserve) {
        if (live) gmk_write_observation(p, e, lane, c, player, obs_after, legal, num_legal, to_play);
        return;
    }

    // ---- Game.step ----
    const bool done = gmk_wave_step(p, e, live, lane, board, padded, c, player, live ? actions[e] : -1, reward_out, done_out,
                                    played_out, words_out);
    if (OP == kGmkStep || !live) return;

    // ---- observation after the move, Game.reset() of a finished env, observation the next search sees ----
    gmk_write_observation(p, e, lane, c, player, obs_after, legal, num_legal, to_play);
    if (done) gmk_wave_reset(p, e, lane, board, c, player);
    gmk_write_observation(p, e, lane, c, player, obs_next, legal, num_legal, to_play);
}

// The same rules with one thread per env, as games 1 and 2 run: kept for measurement and as a cross-check of the
// wavefront form (EnvParams::gomoku_serial, set at mzenv_create from the environment; never the default).
__device__ __forceinline__ void gmk_serial_observe(const EnvParams& p, int e, float* __restrict__ obs,
                                                   int32_t* __restrict__ legal, int32_t* __restrict__ num_legal,
                                                   int32_t* __restrict__ to_play) {
    float* o = obs + static_cast<size_t>(e) * (3 * kGmkCells);
    const int8_t* b = p.board + static_cast<size_t>(e) * kGmkCells;
    const int pl = p.player[e];
    for (int i = 0; i < kGmkCells; ++i) {
        o[i] = b[i] == 1 ? 1.f : 0.f;
        o[kGmkCells + i] = b[i] == -1 ? 1.f : 0.f;
        o[2 * kGmkCells + i] = static_cast<float>(pl);
    }
    const int n = gmk_legal(b, legal + static_cast<size_t>(e) * kGmkCells);
    num_legal[e] = opponent_to_move(p, e) ? 0 : n;
    to_play[e] = pl == 1 ? 0 : 1;
}

__device__ __forceinline__ void gmk_serial_reset(const EnvParams& p, int e) {
    int8_t* b = p.board + static_cast<size_t>(e) * kGmkCells;
    for (int i = 0; i < kGmkCells; ++i) b[i] = 0;
    p.player[e] = 1;
    p.steps[e] = 0;
}

// Game.step of env e by one thread; returns whether the game ended (by its rules or by the move limit)
__device__ __forceinline__ bool gmk_serial_step(const EnvParams& p, int e, int a, float* __restrict__ reward_out,
                                                uint8_t* __restrict__ done_out, int32_t* __restrict__ played_out,
                                                uint32_t* __restrict__ words_out) {
    int8_t* b = p.board + static_cast<size_t>(e) * kGmkCells;
    uint32_t words = 0;
    if (opponent_to_move(p, e)) {
        int32_t pos = p.opp_pos[e];
        a = gmk_opponent_action(b, p.opp_key + static_cast<size_t>(e) * kMtN, &pos, &words);
        if (words) p.opp_pos[e] = pos;
    }
    if (played_out) played_out[e] = a < 0 ? -1 : a;
    if (words_out) words_out[e] = words;
    bool done = false;
    float reward = 0.f;
    if (a >= 0) {
        const int pl = p.player[e];
        if (a < kGmkCells) b[a] = static_cast<int8_t>(pl);
        done = gmk_finished(b);
        reward = done ? 1.f : 0.f;
        const int steps = ++p.steps[e];
        done = done || (p.max_moves > 0 && steps >= p.max_moves);
        p.player[e] = static_cast<int8_t>(-pl);
    }
    reward_out[e] = reward;
    done_out[e] = done ? 1 : 0;
    return done;
}

template <int OP>
__global__ __launch_bounds__(256) void gomoku_env_serial_kernel(
    EnvParams p, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, float* __restrict__ reward_out,
    uint8_t* __restrict__ done_out, float* __restrict__ obs_after, float* __restrict__ obs_next,
    int32_t* __restrict__ legal, int32_t* __restrict__ num_legal, int32_t* __restrict__ to_play,
    int32_t* __restrict__ played_out, uint32_t* __restrict__ words_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    if (OP == kGmkReset) {
        if (!mask || mask[e]) gmk_serial_reset(p, e);
        return;
    }
    if (OP == kGmkObserve) {
        gmk_serial_observe(p, e, obs_after, legal, num_legal, to_play);
        return;
    }
    const bool done = gmk_serial_step(p, e, actions[e], reward_out, done_out, played_out, words_out);
    if (OP == kGmkStep) return;
    gmk_serial_observe(p, e, obs_after, legal, num_legal, to_play);
    if (done) gmk_serial_reset(p, e);
    gmk_serial_observe(p, e, obs_next, legal, num_legal, to_play);
}

// ---- paired moves of Gomoku (mzenv_advance_paired): the slot rule of paired_moves.h over the ply functions above -----
// wavefront form: a slot is collective over the workgroup (gmk_wave_step's barriers), so every wavefront visits every
// slot; the serial part of a move is lane 0's bounded draw, at most once per opponent slot
struct GmkWavePairedOps {
    const EnvParams& p;
    const PairedOut& out;
    int e, lane;
    bool live;
    int8_t *board, *padded;
    GmkCells c;
    int player;
    int32_t *legal, *num_legal, *to_play;
    __device__ bool opponent_to_move() const { return p.opp_kind != kOpponentSelf && (player == 1 ? 0 : 1) != p.opp_player; }
    __device__ void slot(int s, bool play, int a) {
        const size_t at = static_cast<size_t>(s) * p.E;
        const bool done = gmk_wave_step(p, e, live && play, lane, board, padded, c, player, a, out.reward + at, out.done + at,
                                        out.played + at, out.words + at);
        if (!live) return;
        if (!play && lane == 0) paired_empty_slot(out, at + e);
        gmk_write_observation(p, e, lane, c, player, out.obs_after + at * (3 * kGmkCells), legal, num_legal, to_play);
        if (done) gmk_wave_reset(p, e, lane, board, c, player);
    }
};

__global__ __launch_bounds__(64 * kGmkEnvsPerBlock) void gomoku_paired_kernel(EnvParams p, const int32_t* __restrict__ actions,
                                                                              PairedOut out, float* __restrict__ obs_next,
                                                                              int32_t* __restrict__ legal,
                                                                              int32_t* __restrict__ num_legal,
                                                                              int32_t* __restrict__ to_play) {
    __shared__ __attribute__((aligned(16))) int8_t padded_all[kGmkEnvsPerBlock][256];  // 225 bytes used per env
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    const int e = blockIdx.x * kGmkEnvsPerBlock + group;
    const bool live = e < p.E;  // (a wavefront without an env stays for the workgroup barriers and touches no memory)
    int8_t* board = p.board + static_cast<size_t>(live ? e : 0) * kGmkCells;
    GmkWavePairedOps ops{p, out, e, lane, live, board, padded_all[group], GmkCells{2, 2}, 1, legal, num_legal, to_play};
    if (live) {
        ops.c.b0 = board[lane];
        if (lane + 64 < kGmkCells) ops.c.b1 = board[64 + lane];
        ops.player = p.player[e];
    }
    paired_move(ops, live ? actions[e] : -1);
    if (live) gmk_write_observation(p, e, lane, ops.c, ops.player, obs_next, legal, num_legal, to_play);
}

struct GmkSerialPairedOps {
    const EnvParams& p;
    const PairedOut& out;
    int e;
    int32_t *legal, *num_legal, *to_play;
    __device__ bool opponent_to_move() const { return mz::opponent_to_move(p, e); }
    __device__ void slot(int s, bool play, int a) {
        const size_t at = static_cast<size_t>(s) * p.E;
        bool done = false;
        if (play)
            done = gmk_serial_step(p, e, a, out.reward + at, out.done + at, out.played + at, out.words + at);
        else
            paired_empty_slot(out, at + e);
        gmk_serial_observe(p, e, out.obs_after + at * (3 * kGmkCells), legal, num_legal, to_play);
        if (done) gmk_serial_reset(p, e);
    }
};

__global__ __launch_bounds__(256) void gomoku_paired_serial_kernel(EnvParams p, const int32_t* __restrict__ actions,
                                                                   PairedOut out, float* __restrict__ obs_next,
                                                                   int32_t* __restrict__ legal, int32_t* __restrict__ num_legal,
                                                                   int32_t* __restrict__ to_play) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.E) return;
    GmkSerialPairedOps ops{p, out, e, legal, num_legal, to_play};
    paired_move(ops, actions[e]);
    gmk_serial_observe(p, e, obs_next, legal, num_legal, to_play);
}

template <int OP>
hipError_t launch_gomoku(const EnvParams& p, const uint8_t* mask, const int32_t* actions, float* reward, uint8_t* done,
                         float* obs_after, float* obs_next, int32_t* legal, int32_t* num_legal, int32_t* to_play,
                         int32_t* played, uint32_t* words, hipStream_t stream) {
    if (p.gomoku_serial)
        gomoku_env_serial_kernel<OP><<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(
            p, mask, actions, reward, done, obs_after, obs_next, legal, num_legal, to_play, played, words);
    else
        gomoku_env_kernel<OP><<<dim3((p.E + kGmkEnvsPerBlock - 1) / kGmkEnvsPerBlock), dim3(64 * kGmkEnvsPerBlock), 0, stream>>>(
            p, mask, actions, reward, done, obs_after, obs_next, legal, num_legal, to_play, played, words);
    return hipGetLastError();
}

hipError_t launch_env_construct(const EnvParams& p, const uint32_t* seeds, hipStream_t stream) {
    env_construct_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, seeds);
    return hipGetLastError();
}
hipError_t launch_env_reset(const EnvParams& p, const uint8_t* mask, hipStream_t stream) {
    if (p.game == 3)
        return launch_gomoku<kGmkReset>(p, mask, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, stream);
    env_reset_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, mask);
    return hipGetLastError();
}
hipError_t launch_env_step(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done, int32_t* played,
                           uint32_t* words, hipStream_t stream) {
    if (p.game == 3)
        return launch_gomoku<kGmkStep>(p, nullptr, actions, reward, done, nullptr, nullptr, nullptr, nullptr, nullptr, played,
                                       words, stream);
    env_step_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, actions, reward, done, played, words);
    return hipGetLastError();
}
hipError_t launch_env_advance(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done, float* obs_after,
                              float* obs_next, int32_t* legal, int32_t* num_legal, int32_t* to_play, int32_t* played,
                              uint32_t* words, hipStream_t stream) {
    if (p.game == 3)
        return launch_gomoku<kGmkAdvance>(p, nullptr, actions, reward, done, obs_after, obs_next, legal, num_legal, to_play,
                                          played, words, stream);
    env_advance_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, actions, reward, done, obs_after, obs_next, legal,
                                                                          num_legal, to_play, played, words);
    return hipGetLastError();
}
hipError_t launch_env_advance_paired(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done,
                                     float* obs_after, float* obs_next, int32_t* legal, int32_t* num_legal, int32_t* to_play,
                                     int32_t* played, uint32_t* words, hipStream_t stream) {
    const PairedOut out{reward, done, obs_after, played, words};
    if (p.game == 3 && !p.gomoku_serial)
        gomoku_paired_kernel<<<dim3((p.E + kGmkEnvsPerBlock - 1) / kGmkEnvsPerBlock), dim3(64 * kGmkEnvsPerBlock), 0, stream>>>(
            p, actions, out, obs_next, legal, num_legal, to_play);
    else if (p.game == 3)
        gomoku_paired_serial_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, actions, out, obs_next, legal,
                                                                                       num_legal, to_play);
    else
        env_advance_paired_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, actions, out, obs_next, legal, num_legal,
                                                                                     to_play);
    return hipGetLastError();
}
hipError_t launch_env_observe(const EnvParams& p, float* obs, int32_t* legal, int32_t* num_legal, int32_t* to_play,
                              hipStream_t stream) {
    if (p.game == 3)
        return launch_gomoku<kGmkObserve>(p, nullptr, nullptr, nullptr, nullptr, obs, nullptr, legal, num_legal, to_play, nullptr,
                                          nullptr, stream);
    env_observe_kernel<<<dim3((p.E + 255) / 256), dim3(256), 0, stream>>>(p, obs, legal, num_legal, to_play);
    return hipGetLastError();
}

}  // namespace mz
