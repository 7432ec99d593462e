/*
 * mzenv.h -- C ABI of the device-resident batched game environments (part of libmzmcts.so).
 *
 * once the search runs at 10^7..10^8 simulations/s, stepping 4096
 * Python `Game` objects on the host (one `game.step` per env and move) is the bottleneck.  These
 * kernels keep E games of one kind resident on the GPU behind the same plugin semantics as the
 * reference's game files:
 *
 *   MZENV_TICTACTOE  games/tictactoe.py:242-305 (rules), :132-145 (reward x20), observation planes
 *                    [own stones, opponent stones, player to move] as int-valued floats
 *   MZENV_CONNECT4   games/connect4.py:219-304 (rules), :132-143 (reward x10)
 *   MZENV_GOMOKU     games/gomoku.py:219-289 (rules; is_finished :263-291), :236-249 (reward 1 for the ply that ends the game, a full-board
 *                    draw included; no scaling).  11 x 11 board, cell = action = 11 * row + column, A = 121; a game
 *                    ends when any stone of either colour starts five equal stones down-left, down, down-right or
 *                    right (six in a row contains a five; a run does not wrap from column 10 into the next row), or
 *                    when the board is full.  Scripted opponent: "random" only -- the reference defines no expert
 *                    agent for Gomoku and mzenv_set_opponent refuses MZENV_OPPONENT_EXPERT there.  A wavefront per
 *                    env, two cells per lane (csrc/env_kernels.hip); games 0-2 run one thread per env.
 *   MZENV_TWENTYONE  games/twentyone.py:227-299 (rules), :144-155 (reward x10).  One player, actions 0 = hit, 1 = stand,
 *                    both legal in every state.  A card is RandomState(seed).randint(1, 13) on the env's OWN stream
 *                    (10, 11 and 12 count 10): masked rejection, one 32-bit word per attempt, so a ply consumes a variable
 *                    number of words -- a hit one card, a stand (or a hit to exactly 21) as many as bring the dealer
 *                    above 16, a bust none beyond its own card.  `Game(seed)` deals two cards in its constructor, which
 *                    mzenv_create therefore draws and discards; every reset deals the player's card, then the dealer's.
 *                    Reward +10 / 0 / -10 on the ply that ends the game.  Observation (3,3,3): a plane of the player's
 *                    hand, a plane of the dealer's, a plane of zeros.  The game's own length is at most 20 plies.  A hit
 *                    that only the move limit ends is no stand: the dealer does not play and the reward is 0.
 *   MZENV_SIMPLEGRID games/simple_grid.py:190-227 (rules), :132-143 (reward x10).  One player on a 3 x 3 grid from (0, 0);
 *                    0 = down, 1 = right, both legal in every state as far as Game.legal_actions() says; a move off the
 *                    grid moves nothing and still counts as a ply.  Reward 10 and done exactly on reaching (2, 2).
 *                    Observation (1,1,9): one-hot of 3 * row + column.  The game has no length of its own: play that
 *                    dawdles ends at the move limit (mzenv_set_max_moves).
 *                    Neither game has an opponent or a board: mzenv_set_opponent (other than SELF) and mzenv_set_boards
 *                    are errors.  One thread per env (csrc/solo_rules.h, shared with a CPU check).
 *   MZENV_CARTPOLE   games/cartpole.py wraps gym's CartPole-v1; gym is not vendored by the reference, so
 *                    this restates the published classic-control equations (Euler, tau = 0.02) exactly as
 *                    muzero-hypermodel_amd/games/cartpole.py does on the host.  Pinned to the published equations:
 *                    given sin(theta) and cos(theta), a step is IEEE double + - * / in a fixed order and equals a numpy
 *                    float64 restatement bit for bit; sin / cos are the device library's, within L ulps of the true values
 *                    (tests/cartpole_reference.py: L and how it was measured).  Still unpinned against gym itself, which
 *                    is absent here.  mzenv_get_state / mzenv_set_state read and write the fp64 state.
 *
 * The last section is the frame stack (mzenv_stack_*): an object of its own that keeps every env's n previous frames on the
 * GPU and turns these kernels' plain observations into the stacked search input of config.stacked_observations = n.
 *
 * Conventions as in mzmcts.h: raw device / host pointers, hipStream_t as void*, 0 = ok, < 0 = error,
 * mzenv_last_error() for the text.  All launch functions are asynchronous and allocation-free.
 */
#ifndef MZENV_H
#define MZENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZENV_CARTPOLE 0
#define MZENV_TICTACTOE 1
#define MZENV_CONNECT4 2
#define MZENV_GOMOKU 3
/* 4 is no game and stays refused by mzenv_create ("bad argument"): an existing check pins that, so the ids go on at 5 */
#define MZENV_TWENTYONE 5
#define MZENV_SIMPLEGRID 6

typedef struct mzenv mzenv;

/* seeds: host u32[E]; env e behaves like `Game(seeds[e])` of the host plugin.  Blocking. */
int mzenv_create(int32_t game, int32_t num_envs, int32_t device, const uint32_t *seeds, mzenv **out);
void mzenv_destroy(mzenv *env);
const char *mzenv_last_error(const mzenv *env);

/* static shape of the game: actions A, players, observation (C,H,W) */
int mzenv_shape(const mzenv *env, int32_t *num_actions, int32_t *num_players, int32_t *obs_shape3);

/* Game.reset() for every env whose mask byte is non-zero (mask dev u8[E], NULL = all envs). */
int mzenv_reset(mzenv *env, const uint8_t *mask, void *stream);

/* Game.step(action) for every env (envs with action < 0 are left untouched; their reward and done read 0):
 *   actions dev i32[E];  reward_out dev f32[E];  done_out dev u8[E] */
int mzenv_step(mzenv *env, const int32_t *actions, float *reward_out, uint8_t *done_out, void *stream);

/* What the search needs before a move: the observation batch, Game.legal_actions() in the plugin's
 * order, Game.to_play().
 *   obs_out dev f32[E,C,H,W];  legal_out dev i32[E,A] (first num_legal[e] entries valid);
 *   num_legal_out dev i32[E];  to_play_out dev i32[E] */
int mzenv_observe(mzenv *env, float *obs_out, int32_t *legal_out, int32_t *num_legal_out, int32_t *to_play_out,
                  void *stream);

/* One self-play move of every env in a single call (one launch on `stream`): Game.step(actions), the
 * observation after the move (terminal observations included) -> obs_after_out, Game.reset() of the envs that
 * just finished, and the observation the next search sees -> obs_next_out (legal / num_legal / to_play outputs
 * describe that next state). */
int mzenv_advance(mzenv *env, const int32_t *actions, float *reward_out, uint8_t *done_out, float *obs_after_out,
                  float *obs_next_out, int32_t *legal_out, int32_t *num_legal_out, int32_t *to_play_out, void *stream);

/* ---- evaluation games: a scripted opponent plays one side (reference self_play.py:189-221) -----------------------
 * MZENV_OPPONENT_EXPERT  the plugin's expert_agent(): numpy.random.choice over the legal actions (always drawn), then
 *                        the line scan of games/tictactoe.py / games/connect4.py (a winning completion returns at
 *                        once, a block is kept while the scan goes on); not available for MZENV_GOMOKU (error)
 * MZENV_OPPONENT_RANDOM  numpy.random.choice over the legal actions
 * In a reference worker the opponent draws from numpy's global generator, which is also the search's stream: mt_key
 * (dev u32[E][624]) and mt_pos (dev i32[E]) are therefore the SEARCH ENGINE's per-env streams (mzmcts_rng_streams);
 * the words an opponent consumed are reported per env so that the engine's host mirrors can step over them
 * (mzmcts_rng_consumed).  A one-element legal set consumes no word.
 *
 * While the mode is on (kind != MZENV_OPPONENT_SELF), for an env whose side to move is not muzero_player
 *   - mzenv_observe / mzenv_advance_opponent report num_legal = 0 (the engine's "this env sits the search out"; its
 *     stream is left alone); the `legal` row stays filled;
 *   - mzenv_step_opponent / mzenv_advance_opponent ignore the incoming action and play the opponent's move.
 * An env on muzero_player's turn with action < 0 is left untouched as ever; on the opponent's turn "action < 0" no
 * longer protects an env, so finished games are to be reset before the next step (mzenv_advance_opponent does it; after
 * mzenv_step_opponent call mzenv_reset with the done mask).  An env whose board is full has no opponent move: it is left
 * untouched (played_out -1, no word drawn).  A won but not full position that was not reset is played on.  mzenv_step / mzenv_advance refuse to run
 * in opponent mode (nothing would report the opponent's moves).  One-player games have no opponent (error). */
#define MZENV_OPPONENT_SELF 0
#define MZENV_OPPONENT_EXPERT 1
#define MZENV_OPPONENT_RANDOM 2
int mzenv_set_opponent(mzenv *env, int32_t kind, int32_t muzero_player, uint32_t *mt_key, int32_t *mt_pos);

/* mzenv_step / mzenv_advance with two more outputs per env (usable in either mode):
 *   played_out dev i32[E]  the action actually played (the opponent's own on its turn; -1: env left untouched)
 *   words_out  dev u32[E]  32-bit words the opponent's choice consumed from the env's stream (0 elsewhere) */
int mzenv_step_opponent(mzenv *env, const int32_t *actions, float *reward_out, uint8_t *done_out, int32_t *played_out,
                        uint32_t *words_out, void *stream);
int mzenv_advance_opponent(mzenv *env, const int32_t *actions, float *reward_out, uint8_t *done_out, float *obs_after_out,
                           float *obs_next_out, int32_t *legal_out, int32_t *num_legal_out, int32_t *to_play_out,
                           int32_t *played_out, uint32_t *words_out, void *stream);

/* ---- paired moves: the opponent replies inside MuZero's move ---------------------------------------------------------
 * With mzenv_advance_opponent an env on the opponent's turn sits a whole search out.  mzenv_advance_paired plays, in ONE
 * launch and per env, up to MZENV_PAIRED_SLOTS plies (the rule lives once in csrc/paired_moves.h; kernels and a CPU check
 * compile it):
 *   slot 0     MuZero's ply: only if muzero_player is to move and actions[e] >= 0 -- what mzenv_advance_opponent does for
 *              such an env: step, observation of the position reached, reset if the game is over (rules or move limit)
 *   slot 1, 2  while the opponent is to move: its choice from the env's stream exactly as in mzenv_advance_opponent, step,
 *              observation, reset if the game is over.  Slot 1 is the reply, or the opening of the next game when MuZero's
 *              ply ended the game and MuZero plays second; slot 2 can only be such an opening after a reply that ended
 *              the game.
 * Outputs with a leading slot axis: reward_out dev f32[3][E], done_out dev u8[3][E], obs_after_out dev f32[3][E,C,H,W],
 * played_out dev i32[3][E] (-1 = the slot is empty: reward, done and words read 0, obs_after the position as it stood),
 * words_out dev u32[3][E] (the host steps its stream mirrors over the sum of an env's slots).  Once per env, for the
 * position the next search sees: obs_next_out, legal_out, num_legal_out, to_play_out as in mzenv_advance.
 * Afterwards muzero_player is to move in every env and num_legal > 0 (a full board handed in by mzenv_set_boards on the
 * opponent's turn excepted: it has no move).  Every ply counts into the env's ply counter and the move limit applies per
 * ply.  With all actions -1 the launch plays only the opponent's pending plies (the openings after a reset when MuZero
 * plays second): run it once when the mode is taken up.
 * Errors: a one-player game; no opponent set; a move limit of 1 with muzero_player = 1 (opening, limit, reset, opening,
 * ...: MuZero would never move).  mzenv_advance_opponent and mzenv_advance are what they were. */
#define MZENV_PAIRED_SLOTS 3
int mzenv_advance_paired(mzenv *env, const int32_t *actions, float *reward_out, uint8_t *done_out, float *obs_after_out,
                         float *obs_next_out, int32_t *legal_out, int32_t *num_legal_out, int32_t *to_play_out,
                         int32_t *played_out, uint32_t *words_out, void *stream);

/* Put every env of a board game into a given position: boards host i8[E][cells] (0 empty, +1 first player, -1 second;
 * tic-tac-toe cell = 3 * row + column, connect four cell = 7 * row + column with row 0 at the bottom, gomoku cell =
 * 11 * row + column), players host i8[E] (+1 / -1 to move).  Blocking; cell and player values are checked, reachability is not (see above for what a
 * step does with a finished position).  The ply counter of each env (below) becomes the number of stones on its board:
 * a position handed in continues the game it came from. */
int mzenv_set_boards(mzenv *env, const int8_t *boards, const int8_t *players);

/* The fp64 state of every MZENV_CARTPOLE env, in the order x, x_dot, theta, theta_dot, and its ply counter.  Blocking,
 * host arrays, modelled on mzenv_set_boards; every other game is refused with a message.
 *   mzenv_get_state  state_out host f64[E][4]; steps_out host i32[E], may be NULL.
 *   mzenv_set_state  state host f64[E][4], stored as given: non-finite values included (what a step answers on them is
 *                    plain IEEE arithmetic: a NaN compares false at both limits, so such a state is not "fallen");
 *                    steps host i32[E], NULL = leave the counters as they are; a negative count is refused.
 * A handed-in step count is the game's ply counter (below): the state continues a game that has played that many plies.
 * CartPole's own 500-step cap and mzenv_set_max_moves both read it: the next ply brings it to steps + 1 and ends the
 * game when that reaches 500 or the move limit.  The env's stream is untouched: the next reset draws what it would have
 * drawn anyway. */
int mzenv_get_state(mzenv *env, double *state_out, int32_t *steps_out);
int mzenv_set_state(mzenv *env, const double *state, const int32_t *steps);

/* ---- move limit: games end at config.max_moves (reference self_play.py:129-131) ------------------------------------
 * play_game() leaves its loop once len(action_history) exceeds max_moves, whatever the game's own rules say.  Every env
 * counts the plies actually played in its current game -- in opponent mode the opponent's plies too, as
 * len(action_history) does; an env left untouched (action < 0 on muzero_player's turn, a full board on the opponent's:
 * played_out -1) does not count.  Game.reset() zeroes the counter, whether it comes from mzenv_reset (masked envs only)
 * or from inside mzenv_advance / mzenv_advance_opponent.
 *
 * mzenv_set_max_moves: 0 (the value at create) = no limit: every call behaves as it does without this section.
 *   max_moves > 0: the ply that brings an env's counter to max_moves (or beyond it, when the limit was lowered in
 *   mid-game) reports done_out = 1 even if the game's own rules say it goes on, and mzenv_advance /
 *   mzenv_advance_opponent reset that env like any finished one.  reward_out, obs_after_out, played_out and words_out
 *   are what the ply produced; nothing else changes.  WITH A LIMIT SET, done MEANS "THE GAME IS OVER", NOT "THE POSITION
 *   IS TERMINAL".  After mzenv_step / mzenv_step_opponent the caller resets the envs flagged done, as ever.
 *   CartPole's own time limit (500 steps, gym's) is part of the game's rules and independent of this.
 *   The limit travels with every launch: setting it is a host store -- no allocation, no synchronisation -- and is
 *   legal between any two launches; launches already queued keep the limit they were queued with.  Negative: error.
 * mzenv_game_moves: copies the counters to out_dev (dev i32[E]) on `stream`; asynchronous and allocation-free. */
int mzenv_set_max_moves(mzenv *env, int32_t max_moves);
int mzenv_game_moves(mzenv *env, int32_t *out_dev, void *stream);

/* ---- stacked observations: config.stacked_observations = n (reference self_play.py:514-548) -------------------------
 * The search of a position reads GameHistory.get_stacked_observations(-1, n): the current frame (C planes), then the n
 * previous frames newest first, each as its C planes followed by one constant plane holding float(action played from
 * it); positions before the game's start are zeros: (C + n (C + 1)) H W floats per env.  A frame stack keeps, per env,
 * a ring of the n previous frames (stored with the action plane filled, so a frame of the output is one contiguous
 * copy), a head and a count saturating at n, and turns the environment kernels' plain observations into that search
 * input on the device.  It is an object of its own: the env handle, its kernels and their outputs are what they were,
 * and the plain observations stay what is filed and stored (the replay store stacks on its own when it samples).
 * The rule lives once in csrc/obs_stack.h (kernel and CPU check compile it); csrc/obs_stack.hip says how one launch
 * pushes and emits without reading anything it writes.
 *
 * mzenv_stack_create   blocking; the only place that allocates.  n <= 0, a non-positive shape or env count, a null
 *                      `out` and a stacked float count beyond int32 are refused (-1) before any device work; without a
 *                      device a good call returns -2.
 * mzenv_stack_floats   (C + n (C + 1)) H W
 * mzenv_stack_reset    envs whose mask byte is non-zero (mask dev u8[E], NULL = all) forget their frames; obs dev
 *                      f32[E,C,H,W] is every env's current frame; stacked_out dev f32[E, floats] becomes, for EVERY env,
 *                      the current frame followed by the frames it holds, then zeros.
 * mzenv_stack_push     one self-play move of every env, one launch, asynchronous and allocation-free: obs_before dev
 *                      f32[E,C,H,W] the frames the move was played from, actions dev i32[E], done dev u8[E] (the game is
 *                      over: by its rules or by the move limit), obs_next dev f32[E,C,H,W] the observation the next search
 *                      sees (mzenv_advance's obs_next_out).  Per env: actions[e] < 0 = the env was left untouched (a
 *                      stalled env of a pre-drawn batch, a full board on the opponent's turn): nothing is pushed;
 *                      otherwise done[e] != 0: the env forgets its frames; otherwise (obs_before[e], actions[e]) is
 *                      pushed.  In every case stacked_out[e] = [obs_next[e], frames newest to oldest, zeros].
 *                      In opponent mode pass played_out as `actions`: the opponent's plies are plies of the game.
 * Null pointers are refused (-1) before the handle is looked at. */
typedef struct mzenv_stack mzenv_stack;
int mzenv_stack_create(int32_t num_envs, int32_t channels, int32_t height, int32_t width, int32_t n, int32_t device,
                       mzenv_stack **out);
void mzenv_stack_destroy(mzenv_stack *stack);
const char *mzenv_stack_last_error(const mzenv_stack *stack);
int64_t mzenv_stack_floats(const mzenv_stack *stack);
int mzenv_stack_reset(mzenv_stack *stack, const uint8_t *mask, const float *obs, float *stacked_out, void *stream);
int mzenv_stack_push(mzenv_stack *stack, const float *obs_before, const int32_t *actions, const uint8_t *done,
                     const float *obs_next, float *stacked_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MZENV_H */
