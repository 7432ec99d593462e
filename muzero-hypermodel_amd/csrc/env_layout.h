// env_layout.h -- device state of the batched environments (env_kernels.hip, mzenv_capi.hip).
#pragma once
#include <cstdint>

namespace mz {

struct EnvParams {
    int32_t game, E, A, cells, obs_floats;
    int8_t* board;     // [E][cells]  tictactoe / connect4 / gomoku: 0 empty, +1 first player, -1 second player
    int8_t* player;    // [E]         +1 / -1: the player to move
    double* state;     // [E][4]      cartpole: x, x_dot, theta, theta_dot
    int32_t* steps;    // [E]         plies played in the env's current game (every game; cartpole's time limit reads it)
    uint32_t* mt_key;  // [E][624]    cartpole reset stream, twentyone card stream (numpy RandomState(seed))
    int32_t* mt_pos;   // [E]
    // opponent mode of the board games (mzenv_set_opponent): kind (board_rules.h OpponentKind), the player MuZero
    // plays, and the caller's per-env streams the opponent draws from (the search engine's: mzmcts_rng_streams)
    int32_t opp_kind, opp_player;
    uint32_t* opp_key;  // [E][624]
    int32_t* opp_pos;   // [E]
    // move limit (mzenv_set_max_moves): > 0 = the ply that brings steps[e] to it ends the game; 0 = the game's own rules only
    int32_t max_moves;
    // Gomoku only: non-zero runs the one-thread-per-env form of its kernels instead of the wavefront-per-env form (a
    // measurement and cross-check switch, read from the environment at mzenv_create; never the default)
    int32_t gomoku_serial;
    int32_t* solo;  // [E][2]      twentyone: player_hand, dealer_hand;  simple_grid: row, col (solo_rules.h)
};

}  // namespace mz
