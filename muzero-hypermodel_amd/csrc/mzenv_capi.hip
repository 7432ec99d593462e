// mzenv_capi.hip -- host side of the device-resident environments (include/mzenv.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mzenv.h"
#include "env_layout.h"
#include "np_legacy_rng.h"

namespace mz {
hipError_t launch_env_reset(const EnvParams& p, const uint8_t* mask, hipStream_t stream);
hipError_t launch_env_step(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done, int32_t* played,
                           uint32_t* words, hipStream_t stream);
hipError_t launch_env_advance(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done, float* obs_after,
                              float* obs_next, int32_t* legal, int32_t* num_legal, int32_t* to_play, int32_t* played,
                              uint32_t* words, hipStream_t stream);
hipError_t launch_env_advance_paired(const EnvParams& p, const int32_t* actions, float* reward, uint8_t* done,
                                     float* obs_after, float* obs_next, int32_t* legal, int32_t* num_legal, int32_t* to_play,
                                     int32_t* played, uint32_t* words, hipStream_t stream);
hipError_t launch_env_observe(const EnvParams& p, float* obs, int32_t* legal, int32_t* num_legal, int32_t* to_play,
                              hipStream_t stream);
hipError_t launch_env_construct(const EnvParams& p, const uint32_t* seeds, hipStream_t stream);
hipError_t launch_seed_streams(uint32_t* keys, int32_t* pos, const uint32_t* seeds, int E, hipStream_t stream);
}  // namespace mz

struct mzenv {
    mz::EnvParams p{};
    int32_t players = 1;
    int32_t shape[3] = {1, 1, 1};
    int32_t device = 0;
    std::string error;
    std::vector<void*> allocs;
};

namespace {
thread_local std::string g_env_error;
int env_fail(mzenv* env, int code, const std::string& msg) {
    if (env) env->error = msg;
    g_env_error = msg;
    return code;
}
#define MZENV_HIP(env, call)                                                                                 \
    do {                                                                                                     \
        hipError_t err__ = (call);                                                                           \
        if (err__ != hipSuccess) return env_fail(env, -2, std::string(#call) + ": " + hipGetErrorString(err__)); \
    } while (0)

template <typename T>
int env_alloc(mzenv* env, T** out, size_t count) {
    void* ptr = nullptr;
    MZENV_HIP(env, hipMalloc(&ptr, count * sizeof(T) ? count * sizeof(T) : 16));
    MZENV_HIP(env, hipMemset(ptr, 0, count * sizeof(T) ? count * sizeof(T) : 16));
    env->allocs.push_back(ptr);
    *out = static_cast<T*>(ptr);
    return 0;
}
}  // namespace

extern "C" {

const char* mzenv_last_error(const mzenv* env) { return env ? env->error.c_str() : g_env_error.c_str(); }

int mzenv_create(int32_t game, int32_t num_envs, int32_t device, const uint32_t* seeds, mzenv** out) {
    if (!out || !seeds || num_envs <= 0 || game < 0 || game > MZENV_SIMPLEGRID || game == 4) return env_fail(nullptr, -1, "mzenv_create: bad argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return env_fail(nullptr, -2, "mzenv_create: no HIP device available; the device environments have no CPU fallback");
    if (device < 0 || device >= n_dev) return env_fail(nullptr, -1, "mzenv_create: bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return env_fail(nullptr, -2, "hipSetDevice failed");
    auto* env = new mzenv();
    env->device = device;
    mz::EnvParams& p = env->p;
    p.game = game;
    p.E = num_envs;
    int rc = 0;
    auto bail = [&](int code) {
        g_env_error = env->error;
        mzenv_destroy(env);
        return code;
    };
    if ((rc = env_alloc(env, &p.steps, num_envs))) return bail(rc);
    if (game == MZENV_CARTPOLE) {
        p.A = 2;
        p.cells = 0;
        p.obs_floats = 4;
        env->players = 1;
        env->shape[0] = 1, env->shape[1] = 1, env->shape[2] = 4;
        if ((rc = env_alloc(env, &p.state, static_cast<size_t>(num_envs) * 4))) return bail(rc);
        if ((rc = env_alloc(env, &p.mt_key, static_cast<size_t>(num_envs) * mz::kMtN))) return bail(rc);
        if ((rc = env_alloc(env, &p.mt_pos, num_envs))) return bail(rc);
        uint32_t* d_seeds = nullptr;
        if ((rc = env_alloc(env, &d_seeds, num_envs))) return bail(rc);
        hipError_t err = hipMemcpy(d_seeds, seeds, sizeof(uint32_t) * num_envs, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = mz::launch_seed_streams(p.mt_key, p.mt_pos, d_seeds, num_envs, nullptr);
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err != hipSuccess) return bail(env_fail(env, -2, std::string("seeding: ") + hipGetErrorString(err)));
    } else if (game == MZENV_TWENTYONE || game == MZENV_SIMPLEGRID) {
        p.A = 2;
        p.cells = 0;
        env->players = 1;
        if (game == MZENV_TWENTYONE)
            env->shape[0] = 3, env->shape[1] = 3, env->shape[2] = 3;
        else
            env->shape[0] = 1, env->shape[1] = 1, env->shape[2] = 9;
        p.obs_floats = env->shape[0] * env->shape[1] * env->shape[2];
        if ((rc = env_alloc(env, &p.solo, static_cast<size_t>(num_envs) * 2))) return bail(rc);  // (zeroed: the grid's start)
        if (game == MZENV_TWENTYONE) {
            // TwentyOne(seeds[e]): seed the card stream and deal the constructor's two cards
            if ((rc = env_alloc(env, &p.mt_key, static_cast<size_t>(num_envs) * mz::kMtN))) return bail(rc);
            if ((rc = env_alloc(env, &p.mt_pos, num_envs))) return bail(rc);
            uint32_t* d_seeds = nullptr;
            if ((rc = env_alloc(env, &d_seeds, num_envs))) return bail(rc);
            hipError_t err = hipMemcpy(d_seeds, seeds, sizeof(uint32_t) * num_envs, hipMemcpyHostToDevice);
            if (err == hipSuccess) err = mz::launch_env_construct(p, d_seeds, nullptr);
            if (err == hipSuccess) err = hipDeviceSynchronize();
            if (err != hipSuccess) return bail(env_fail(env, -2, std::string("seeding: ") + hipGetErrorString(err)));
        }
    } else {
        const int rows = game == MZENV_TICTACTOE ? 3 : (game == MZENV_CONNECT4 ? 6 : 11);
        const int cols = game == MZENV_TICTACTOE ? 3 : (game == MZENV_CONNECT4 ? 7 : 11);
        p.cells = rows * cols;
        p.A = game == MZENV_CONNECT4 ? cols : p.cells;
        p.obs_floats = 3 * p.cells;
        env->players = 2;
        env->shape[0] = 3, env->shape[1] = rows, env->shape[2] = cols;
        if (game == MZENV_GOMOKU) {
            // measurement / cross-check switch: the one-thread-per-env form of the Gomoku kernels (env_kernels.hip)
            const char* serial = std::getenv("MZENV_GOMOKU_SERIAL");
            p.gomoku_serial = (serial && serial[0] && serial[0] != '0') ? 1 : 0;
        }
        if ((rc = env_alloc(env, &p.board, static_cast<size_t>(num_envs) * p.cells))) return bail(rc);
        if ((rc = env_alloc(env, &p.player, num_envs))) return bail(rc);
    }
    *out = env;
    return 0;
}

void mzenv_destroy(mzenv* env) {
    if (!env) return;
    (void)hipSetDevice(env->device);
    (void)hipDeviceSynchronize();
    for (void* ptr : env->allocs) (void)hipFree(ptr);
    delete env;
}

int mzenv_shape(const mzenv* env, int32_t* num_actions, int32_t* num_players, int32_t* obs_shape3) {
    if (!env) return -1;
    if (num_actions) *num_actions = env->p.A;
    if (num_players) *num_players = env->players;
    if (obs_shape3)
        for (int i = 0; i < 3; ++i) obs_shape3[i] = env->shape[i];
    return 0;
}

int mzenv_reset(mzenv* env, const uint8_t* mask, void* stream) {
    if (!env) return -1;
    MZENV_HIP(env, mz::launch_env_reset(env->p, mask, static_cast<hipStream_t>(stream)));
    return 0;
}

int mzenv_set_opponent(mzenv* env, int32_t kind, int32_t muzero_player, uint32_t* mt_key, int32_t* mt_pos) {
    // (the arguments are judged before the handle: a wrong call reads the same with or without a device)
    if (kind != MZENV_OPPONENT_SELF && kind != MZENV_OPPONENT_EXPERT && kind != MZENV_OPPONENT_RANDOM)
        return env_fail(env, -1, "mzenv_set_opponent: unknown opponent kind (self, expert or random)");
    if (kind != MZENV_OPPONENT_SELF && (!mt_key || !mt_pos))
        return env_fail(env, -1, "mzenv_set_opponent: the opponent needs the per-env streams it draws from");
    if (!env) return env_fail(nullptr, -1, "mzenv_set_opponent: null handle");
    if (kind == MZENV_OPPONENT_SELF) {
        env->p.opp_kind = MZENV_OPPONENT_SELF;
        env->p.opp_player = 0;
        env->p.opp_key = nullptr;
        env->p.opp_pos = nullptr;
        return 0;
    }
    if (env->players < 2) return env_fail(env, -1, "mzenv_set_opponent: a one-player game has no opponent");
    if (muzero_player < 0 || muzero_player >= env->players)
        return env_fail(env, -1, "mzenv_set_opponent: muzero_player is not a player of this game");
    if (env->p.game == MZENV_GOMOKU && kind == MZENV_OPPONENT_EXPERT)
        return env_fail(env, -1, "mzenv_set_opponent: gomoku has no expert agent (the reference's games/gomoku.py defines none); "
                                 "its scripted opponent is \"random\"");
    env->p.opp_kind = kind;
    env->p.opp_player = muzero_player;
    env->p.opp_key = mt_key;
    env->p.opp_pos = mt_pos;
    return 0;
}

int mzenv_set_boards(mzenv* env, const int8_t* boards, const int8_t* players) {
    if (!env || !boards || !players) return env_fail(env, -1, "mzenv_set_boards: null argument");
    if (env->players < 2) return env_fail(env, -1, "mzenv_set_boards: not a board game");
    const size_t E = static_cast<size_t>(env->p.E), cells = static_cast<size_t>(env->p.cells);
    std::vector<int32_t> stones(E, 0);  // the game a position came from has played one ply per stone
    for (size_t e = 0; e < E; ++e) {
        if (players[e] != 1 && players[e] != -1) return env_fail(env, -1, "mzenv_set_boards: a player to move is +1 or -1");
        for (size_t i = 0; i < cells; ++i) {
            if (boards[e * cells + i] < -1 || boards[e * cells + i] > 1)
                return env_fail(env, -1, "mzenv_set_boards: a cell is 0, +1 or -1");
            stones[e] += boards[e * cells + i] != 0;
        }
    }
    MZENV_HIP(env, hipSetDevice(env->device));
    MZENV_HIP(env, hipDeviceSynchronize());
    MZENV_HIP(env, hipMemcpy(env->p.board, boards, E * cells, hipMemcpyHostToDevice));
    MZENV_HIP(env, hipMemcpy(env->p.player, players, E, hipMemcpyHostToDevice));
    MZENV_HIP(env, hipMemcpy(env->p.steps, stones.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int mzenv_get_state(mzenv* env, double* state_out, int32_t* steps_out) {
    if (!env || !state_out) return env_fail(env, -1, "mzenv_get_state: null argument");
    if (env->p.game != MZENV_CARTPOLE) return env_fail(env, -1, "mzenv_get_state: only cartpole keeps an fp64 state");
    const size_t E = static_cast<size_t>(env->p.E);
    MZENV_HIP(env, hipSetDevice(env->device));
    MZENV_HIP(env, hipDeviceSynchronize());
    MZENV_HIP(env, hipMemcpy(state_out, env->p.state, E * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (steps_out) MZENV_HIP(env, hipMemcpy(steps_out, env->p.steps, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mzenv_set_state(mzenv* env, const double* state, const int32_t* steps) {
    if (!env || !state) return env_fail(env, -1, "mzenv_set_state: null argument");
    if (env->p.game != MZENV_CARTPOLE) return env_fail(env, -1, "mzenv_set_state: only cartpole keeps an fp64 state");
    const size_t E = static_cast<size_t>(env->p.E);
    if (steps)
        for (size_t e = 0; e < E; ++e)
            if (steps[e] < 0) return env_fail(env, -1, "mzenv_set_state: a step count is a number of plies played (>= 0)");
    MZENV_HIP(env, hipSetDevice(env->device));
    MZENV_HIP(env, hipDeviceSynchronize());
    MZENV_HIP(env, hipMemcpy(env->p.state, state, E * 4 * sizeof(double), hipMemcpyHostToDevice));
    if (steps) MZENV_HIP(env, hipMemcpy(env->p.steps, steps, E * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int mzenv_set_max_moves(mzenv* env, int32_t max_moves) {
    // (the argument is judged before the handle, as in mzenv_set_opponent)
    if (max_moves < 0) return env_fail(env, -1, "mzenv_set_max_moves: the limit is a number of plies (0 = none)");
    if (!env) return env_fail(nullptr, -1, "mzenv_set_max_moves: null handle");
    env->p.max_moves = max_moves;  // (EnvParams travels by value with every launch: nothing on the device to update)
    return 0;
}

int mzenv_game_moves(mzenv* env, int32_t* out_dev, void* stream) {
    if (!env || !out_dev) return env_fail(env, -1, "mzenv_game_moves: null argument");
    MZENV_HIP(env, hipMemcpyAsync(out_dev, env->p.steps, sizeof(int32_t) * env->p.E, hipMemcpyDeviceToDevice,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

int mzenv_step(mzenv* env, const int32_t* actions, float* reward_out, uint8_t* done_out, void* stream) {
    if (!env || !actions || !reward_out || !done_out) return env_fail(env, -1, "mzenv_step: null argument");
    if (env->p.opp_kind != MZENV_OPPONENT_SELF)
        return env_fail(env, -1, "mzenv_step: opponent mode is on; mzenv_step_opponent reports the moves the opponent played");
    MZENV_HIP(env, mz::launch_env_step(env->p, actions, reward_out, done_out, nullptr, nullptr, static_cast<hipStream_t>(stream)));
    return 0;
}

int mzenv_step_opponent(mzenv* env, const int32_t* actions, float* reward_out, uint8_t* done_out, int32_t* played_out,
                        uint32_t* words_out, void* stream) {
    if (!env || !actions || !reward_out || !done_out || !played_out || !words_out)
        return env_fail(env, -1, "mzenv_step_opponent: null argument");
    MZENV_HIP(env, mz::launch_env_step(env->p, actions, reward_out, done_out, played_out, words_out,
                                       static_cast<hipStream_t>(stream)));
    return 0;
}

int mzenv_observe(mzenv* env, float* obs_out, int32_t* legal_out, int32_t* num_legal_out, int32_t* to_play_out,
                  void* stream) {
    if (!env || !obs_out || !legal_out || !num_legal_out || !to_play_out)
        return env_fail(env, -1, "mzenv_observe: null argument");
    MZENV_HIP(env, mz::launch_env_observe(env->p, obs_out, legal_out, num_legal_out, to_play_out,
                                          static_cast<hipStream_t>(stream)));
    return 0;
}

int mzenv_advance(mzenv* env, const int32_t* actions, float* reward_out, uint8_t* done_out, float* obs_after_out,
                  float* obs_next_out, int32_t* legal_out, int32_t* num_legal_out, int32_t* to_play_out, void* stream_) {
    if (!env || !actions || !reward_out || !done_out || !obs_after_out || !obs_next_out || !legal_out || !num_legal_out ||
        !to_play_out)
        return env_fail(env, -1, "mzenv_advance: null argument");
    if (env->p.opp_kind != MZENV_OPPONENT_SELF)
        return env_fail(env, -1, "mzenv_advance: opponent mode is on; mzenv_advance_opponent reports the moves the opponent played");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MZENV_HIP(env, mz::launch_env_advance(env->p, actions, reward_out, done_out, obs_after_out, obs_next_out, legal_out,
                                          num_legal_out, to_play_out, nullptr, nullptr, stream));
    return 0;
}

int mzenv_advance_opponent(mzenv* env, const int32_t* actions, float* reward_out, uint8_t* done_out, float* obs_after_out,
                           float* obs_next_out, int32_t* legal_out, int32_t* num_legal_out, int32_t* to_play_out,
                           int32_t* played_out, uint32_t* words_out, void* stream_) {
    if (!env || !actions || !reward_out || !done_out || !obs_after_out || !obs_next_out || !legal_out || !num_legal_out ||
        !to_play_out || !played_out || !words_out)
        return env_fail(env, -1, "mzenv_advance_opponent: null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MZENV_HIP(env, mz::launch_env_advance(env->p, actions, reward_out, done_out, obs_after_out, obs_next_out, legal_out,
                                          num_legal_out, to_play_out, played_out, words_out, stream));
    return 0;
}

int mzenv_advance_paired(mzenv* env, const int32_t* actions, float* reward_out, uint8_t* done_out, float* obs_after_out,
                         float* obs_next_out, int32_t* legal_out, int32_t* num_legal_out, int32_t* to_play_out,
                         int32_t* played_out, uint32_t* words_out, void* stream_) {
    if (!env || !actions || !reward_out || !done_out || !obs_after_out || !obs_next_out || !legal_out || !num_legal_out ||
        !to_play_out || !played_out || !words_out)
        return env_fail(env, -1, "mzenv_advance_paired: null argument");
    if (env->players < 2) return env_fail(env, -1, "mzenv_advance_paired: a one-player game has no opponent");
    if (env->p.opp_kind == MZENV_OPPONENT_SELF)
        return env_fail(env, -1, "mzenv_advance_paired: no opponent is set (mzenv_set_opponent); self-play moves are mzenv_advance's");
    if (env->p.max_moves == 1 && env->p.opp_player != 0)
        return env_fail(env, -1, "mzenv_advance_paired: with a move limit of 1 and MuZero playing second every game is the "
                                 "opponent's opening alone: MuZero would never come to move");
    MZENV_HIP(env, mz::launch_env_advance_paired(env->p, actions, reward_out, done_out, obs_after_out, obs_next_out, legal_out,
                                                 num_legal_out, to_play_out, played_out, words_out,
                                                 static_cast<hipStream_t>(stream_)));
    return 0;
}

}  // extern "C"
