/*
 * mzreplay.h -- C ABI of the device-resident replay store (part of libmzmcts.so).
 *
 * SURVEY.md section 8(f) row 2, the direct consumer of the search's output: finished games
 * (GameHistory, reference self_play.py:480-548) are kept on the GPU as packed arrays and turned into
 * training targets there:
 *
 *   mzreplay_add_games      ReplayBuffer.save_game: initial priorities |root_value - target|^alpha and the
 *                           game priority (replay_buffer.py:33-50)
 *   mzreplay_game_observations / mzreplay_set_reanalysed
 *                           the two ends of Reanalyse's per-game step (replay_buffer.py:335-356): the stacked
 *                           observations of every position of a game as one inference batch, and the fresh
 *                           root values (float32) that compute_target_value bootstraps from afterwards
 *   mzreplay_make_batch     ReplayBuffer.make_target / compute_target_value and
 *                           GameHistory.get_stacked_observations for a batch of (game, position) pairs
 *                           (replay_buffer.py:222-295, self_play.py:514-548)
 *
 * Which games and positions go into a batch, and the random actions of absorbing states, are draws from numpy's
 * legacy RandomState in a fixed order (replay_buffer.py:67-195).  By default they are the caller's and this library
 * only evaluates them (mzreplay_make_batch).  After mzreplay_sampler_enable the store also holds the priorities and
 * a numpy stream of its own on the device, and
 *
 *   mzreplay_sample_batch         draws a batch's games, positions, absorbing actions and importance weights there,
 *                                 draw for draw and bit for bit the reference's (csrc/replay_sampler.h)
 *   mzreplay_make_batch_device    builds the targets from those device-resident indices, in the trainer's dtypes
 *   mzreplay_update_priorities    ReplayBuffer.update_priorities (replay_buffer.py:197-220) from device tensors
 *
 *   mzreplay_reanalyse_*          Reanalyse for N games per pass: the games drawn on the device, every position of every
 *                                 drawn game as one inference batch (csrc/reanalyse_plan.h), for fully-connected networks
 *                                 the whole pass in one launch
 *
 *   mzreplay_filer_*              finished self-play games appended straight from the search engine's and the
 *                                 environment kernels' device rings (csrc/replay_filer.h); mzreplay_read_games reads
 *                                 stored games back
 *
 * so that neither a training step nor a self-play batch needs a host round trip through the store.  fp64 sums run in the reference's order with
 * `discount ** i` taken from a table the caller fills with its own libm (Python floats), so values and
 * policies are bit-identical to the reference's; priorities go through the device's pow() and agree to
 * float32 rounding.
 *
 * Conventions as in mzmcts.h: raw host / device pointers, hipStream_t as void*, 0 = ok, < 0 = error.
 */
#ifndef MZREPLAY_H
#define MZREPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mzreplay mzreplay;

typedef struct mzreplay_config {
    int32_t capacity;             /* game slots (config.replay_buffer_size) */
    int32_t max_moves;            /* longest game, in moves */
    int32_t num_actions;
    int32_t obs_channels, obs_height, obs_width;
    int32_t stacked_observations;
    int32_t td_steps, num_unroll_steps;
    int32_t device;
    double per_alpha;
    const double *discount_powers; /* host f64[td_steps + 1]: config.discount ** i, i = 0..td_steps */
} mzreplay_config;

int mzreplay_create(const mzreplay_config *config, mzreplay **out);
void mzreplay_destroy(mzreplay *store);
const char *mzreplay_last_error(const mzreplay *store);

/* Store n games in the given slots (overwriting what was there).  Host arrays, game-major, padded to
 * max_moves: lengths i32[n] (moves), observations f32[n][max_moves+1][C*H*W], actions i32[n][max_moves+1],
 * rewards f64[n][max_moves+1], to_play i32[n][max_moves+1], child_visits f64[n][max_moves][A],
 * root_values f64[n][max_moves].  Outputs (host, may be NULL): priorities f32[n][max_moves],
 * game_priority f32[n].  Blocking. */
int mzreplay_add_games(mzreplay *store, int32_t n, const int32_t *slots, const int32_t *lengths,
                       const float *observations, const int32_t *actions, const double *rewards,
                       const int32_t *to_play, const double *child_visits, const double *root_values,
                       float *priorities, float *game_priority, void *stream);

/* Targets of a batch.  Host inputs: slots i32[B], positions i32[B], absorbing_actions i32[B][U+1] (entry u is
 * used where position + u lies past the end of the game).  Device outputs: observations
 * f32[B][C'][H][W] with C' = C + stacked * (C + 1), actions i64[B][U+1], values / rewards /
 * gradient_scale f64[B][U+1], policies f64[B][U+1][A].  Asynchronous on `stream`. */
int mzreplay_make_batch(mzreplay *store, int32_t batch, const int32_t *slots, const int32_t *positions,
                        const int32_t *absorbing_actions, float *observations, int64_t *actions, double *values,
                        double *rewards, double *policies, double *gradient_scale, void *stream);

/* Stacked observations of positions 0..length-1 of the game in `slot`: observations dev f32[length][C'][H][W].
 * Asynchronous. */
int mzreplay_game_observations(mzreplay *store, int32_t slot, int32_t length, float *observations, void *stream);
/* Reanalyse's values for that game: f32[length], host or device memory.  From now on the game's targets
 * bootstrap from them, accumulating in float32 as the reference does once the values are a numpy float32 array
 * (NumPy >= 2 promotion; recorded in fixture G13).  mzreplay_add_games into the slot forgets them.  Asynchronous. */
int mzreplay_set_reanalysed(mzreplay *store, int32_t slot, const float *values, int32_t length, void *stream);

/* ---- sampling on the device ----------------------------------------------------------------------------------------
 * Switch the sampler on (once per store; calling it again only reseeds): the store then owns, on the device,
 * priorities f32[capacity][max_moves], game_priority f32[capacity], the game id of every slot and an MT19937 stream
 * seeded as numpy.random.seed(seed).  From here on mzreplay_add_games also leaves the initial priorities it computes in
 * those arrays and numbers the games it stores next_game_id, next_game_id + 1, ...  Blocking. */
int mzreplay_sampler_enable(mzreplay *store, uint32_t seed, int64_t next_game_id);
/* The stream as RandomState.get_state() gives it: key u32[624] (host) and the position 0..624.  Blocking. */
int mzreplay_sampler_get_rng(mzreplay *store, uint32_t *key, int32_t *pos);
int mzreplay_sampler_set_rng(mzreplay *store, const uint32_t *key, int32_t pos);
/* Priorities of the game in `slot` given by the caller (a GameHistory that carries its own, a restored buffer):
 * host f32[length]; the game priority becomes their numpy.max, the slot's game id `game_id`.  Blocking. */
int mzreplay_set_priorities(mzreplay *store, int32_t slot, int64_t game_id, const float *priorities, int32_t length,
                            void *stream);
/* Read a slot back (host outputs, each may be NULL): priorities f32[max_moves], game priority, game id (-1: empty).
 * Blocking. */
int mzreplay_get_priorities(mzreplay *store, int32_t slot, float *priorities, float *game_priority, int64_t *game_id,
                            void *stream);
/* ReplayBuffer.get_batch's draws for `batch` samples (1..4096) over the n_games stored games whose ids start at
 * oldest_game_id (slot = id % capacity); total_samples = the sum of their lengths; per != 0: prioritised replay.
 * Device outputs: game_ids i64[B], slots i32[B], positions i32[B], absorbing_actions i32[B][U+1] (the action index
 * drawn for every unrolled step past the end of the game, 0 elsewhere), weights f32[B] (per != 0 only; may be NULL
 * otherwise).  The stream advances by exactly the words the reference would consume.  Asynchronous on `stream`. */
int mzreplay_sample_batch(mzreplay *store, int32_t batch, int64_t oldest_game_id, int32_t n_games, int64_t total_samples,
                          int32_t per, int64_t *game_ids, int32_t *slots, int32_t *positions, int32_t *absorbing_actions,
                          float *weights, void *stream);
/* mzreplay_make_batch with slots / positions / absorbing_actions in device memory, writing the trainer's dtypes:
 * observations f32, actions i64, values / rewards / policies / gradient_scale f32 (the fp64 results of
 * mzreplay_make_batch rounded to nearest at the store).  Needs no sampler.  Asynchronous. */
int mzreplay_make_batch_device(mzreplay *store, int32_t batch, const int32_t *slots, const int32_t *positions,
                               const int32_t *absorbing_actions, float *observations, int64_t *actions, float *values,
                               float *rewards, float *policies, float *gradient_scale, void *stream);
/* ReplayBuffer.update_priorities: device inputs game_ids i64[B], positions i32[B], priorities f32[B][U+1].  Samples are
 * applied in batch order (where two samples of one game overlap, the later one's values stay), rows end at the game's
 * end, a sample whose game id no longer sits in its slot is skipped, and game_priority = max(priorities) of every
 * touched game.  Asynchronous. */
int mzreplay_update_priorities(mzreplay *store, int32_t batch, const int64_t *game_ids, const int32_t *positions,
                               const float *priorities, void *stream);

/* Read stored games back (host outputs in mzreplay_add_games' input layout, each may be NULL): lengths i32[n],
 * observations f32[n][max_moves+1][C*H*W], actions i32[n][max_moves+1], rewards f64[n][max_moves+1], to_play
 * i32[n][max_moves+1], child_visits f64[n][max_moves][A], root_values f64[n][max_moves]; entries past a game's length are
 * zero.  Games filed on the device never existed on the host: this is how a saved buffer or a test sees them.  Blocking. */
int mzreplay_read_games(mzreplay *store, int32_t n, const int32_t *slots, int32_t *lengths, float *observations,
                        int32_t *actions, double *rewards, int32_t *to_play, double *child_visits, double *root_values,
                        void *stream);

/* ---- finished self-play games filed on the device ---------------------------------------------------------------------
 * The producer side of the store without the host: a filer is owned by a store and bound to one actor of E envs; a store
 * may have any number of filers, each with a stream of its own.  A filer keeps, in device memory, one running row per env
 * in the store's own slot layout, its list of filed games and its error word.  The store-wide counters (next game id,
 * games stored, total_samples, steps played) live in one device block of the STORE, which every filer's kernels read and
 * move.  The store numbers games in the order of the mzreplay_filer_file calls made on it, whatever stream each call runs
 * on: a call makes its stream wait for the store's "last filing" event before its first launch and records that event
 * behind its last one, so the calls of all filers run one after the other on the device, in the order the host made them
 * (no host wait, no allocation and no extra launch; one filer on one stream runs as it would without the event; the
 * calls are made from one host thread, or serialised by the caller).  A call may evict games another filer stored.
 * A filer turns a whole move batch -- read where the search engine and the environment kernels left it -- into stored
 * games in three launches with no host decision in between (csrc/replay_filer.h holds the index arithmetic; DESIGN.md
 * sections 7.9 and 7.9.1):
 *   1. per env and move what mzhist_file does: child_visits[len][legal[i]] = double(visits[i]) / S over a zeroed row,
 *      root_values[len] = root_value_sum / S (IEEE fp64 divisions), actions / rewards / observations / to_play[len + 1];
 *      on `done` the row is a finished game of len moves and the next one starts with obs_next, action 0, reward 0 and the
 *      next move's player;
 *   2. an env's played moves are a prefix of the batch, ending at its first move whose action reads < 0;
 *   3. the games a call finishes are numbered env-major, then in move order: id = next id + rank, slot = id % capacity;
 *   4. a finished game is copied into its slot (length set, Reanalyse's values forgotten), its initial priorities and game
 *      priority are computed as mzreplay_add_games computes them (bit for bit) and, with the sampler on, adopted by it;
 *      when a call finishes more games than the store has slots only the last `capacity` are written, and the counters
 *      move as if all had been stored and evicted in turn;
 *   5. nothing read from a ring is used as an index before it was checked: a legal count outside [0, A], a legal action
 *      outside [0, A) or a game longer than max_moves sets a bit in a device error word, NOTHING of that batch is filed,
 *      and the next mzreplay_filer_sync fails with mzhist_file's message (calls after that sync work).
 * A call queued after a refused one and before the sync that reports it is refused too, whatever it holds: the running
 * rows would otherwise have a hole.  The error word stands on the device until that sync (the list's drain inside
 * mzreplay_filer_file leaves it alone).  The games of the calls BEFORE the refused one are not lost: the failing sync keeps
 * them, the following sync hands them out, and the store and the counters are those of a filer that was given only those
 * calls (tests/test_gpu_replay_filer_forms.py).
 * A refusal stays with its filer: the error word refuses that filer's later unsynced calls and no other filer's, and a
 * refused call moves no shared counter, so the other filers' ids stay contiguous around it
 * (tests/test_gpu_replay_filer_shared.py).
 * Errors of these calls are read with mzreplay_last_error(store). */
typedef struct mzreplay_filer mzreplay_filer;

/* The device twin of mzhist_moves: every pointer a DEVICE pointer, per-move blocks `stride` bytes apart (the engine's
 * rings as mzmcts_moves_device_ring / mzmcts_moves_inputs_device_ring report them).  There is no moves_done (rule 2) and
 * no `played` (opponent plies are not filed on the device).  The players to move are given as the searches recorded them:
 * to_play_after of a move is 1 - to_play for two players and 0 for one, to_play_next of a game's last move is the next
 * move's to_play (the batch's last move: to_play_last). */
typedef struct mzreplay_file_moves {
    int32_t n_moves;               /* M */
    int32_t num_simulations;       /* S */
    const void *actions;           /* move m: i32[E] at actions + m * actions_stride */
    int64_t actions_stride;
    const void *visits;            /* move m: i32[E][A], root children by child slot */
    int64_t visits_stride;
    const void *root_value_sum;    /* move m: f64[E] */
    int64_t root_value_sum_stride;
    const void *legal;             /* move m: i32[E][A] child slot -> action; stride 0 = one set for the batch */
    int64_t legal_stride;
    const void *num_legal;         /* move m: i32[E] */
    int64_t num_legal_stride;
    const void *to_play;           /* move m: i32[E] player to move when move m was searched; NULL = player 0 throughout */
    int64_t to_play_stride;
    const int32_t *to_play_last;   /* [E] player to move after the batch's last move (required with to_play) */
    const float *rewards;          /* [M][E] */
    const uint8_t *done;           /* [M][E] game over after this move */
    const float *obs_after;        /* [M][E][obs] observation after the move (terminal one included) */
    const float *obs_next;         /* [M][E][obs] observation the next search sees (reset where done) */
    int32_t players;               /* 1 or 2 */
    int32_t reserved;
} mzreplay_file_moves;

int mzreplay_filer_create(mzreplay *store, int32_t num_envs, mzreplay_filer **out);
void mzreplay_filer_destroy(mzreplay_filer *filer);
/* Every env starts a game: reset observations dev f32[E][obs], to_play dev i32[E] (NULL = player 0).  Asynchronous. */
int mzreplay_filer_begin(mzreplay_filer *filer, const float *first_observations, const int32_t *first_to_play,
                         void *stream);
/* The store-wide counters as the host knows them: counters[4] = next game id, games stored, total_samples, steps played.
 * At the start, and after every mzreplay_add_games into a store that has a filer; through any of the store's filers (the
 * block is the store's).  Waits for the filings queued so far; the values are copied. */
int mzreplay_filer_set_counters(mzreplay_filer *filer, const int64_t *counters, void *stream);
/* File a move batch.  Asynchronous on `stream`: queue it behind the batch's last environment kernel.  The call's games
 * take the ids that follow those of the call made before it on this store, through whichever filer and stream. */
int mzreplay_filer_file(mzreplay_filer *filer, const mzreplay_file_moves *moves, void *stream);
/* The games this filer filed since its last sync, as host arrays (valid until the next call on this filer): 4 bytes per
 * game each for the env and the length, the id the store gave every game (ascending; consecutive only while no other
 * filer's call came in between), the store's counters once every filing queued so far has run (counters[4] as above, may
 * be NULL), and the filer's device error word turned into a message.  The only data that comes back.  Blocking; `stream`
 * waits for the store's last filing, so it need not be the filer's own. */
int mzreplay_filer_sync_ids(mzreplay_filer *filer, int32_t *n_new, const int32_t **env_index, const int32_t **lengths,
                            const int64_t **game_ids, int64_t *counters, void *stream);
/* mzreplay_filer_sync_ids for a store with one filer, whose games are consecutive: the id of the first of them instead
 * of the list.  Fails on a store with more than one filer (use mzreplay_filer_sync_ids). */
int mzreplay_filer_sync(mzreplay_filer *filer, int32_t *n_new, const int32_t **env_index, const int32_t **lengths,
                        int64_t *first_game_id, int64_t *counters, void *stream);
/* Moves played so far in every env's running game: host i32[E] (what mzhist_lengths gives for the host filer).  Blocking. */
int mzreplay_filer_lengths(mzreplay_filer *filer, int32_t *lengths, void *stream);
/* Initial priorities of stored games for a host-side sampler: host f32[n][max_moves] (zero past the length) and f32[n]
 * for the games in `slots` (host i32[n]).  Blocking. */
int mzreplay_filer_priorities(mzreplay_filer *filer, int32_t n, const int32_t *slots, float *priorities,
                              float *game_priority, void *stream);

/* ---- what a finished game reports (csrc/game_outcomes.h) ----------------------------------------
 * The numbers the reference's self-play loop logs per game (self_play.py:65-90), computed where the game lies: the total
 * reward (Python's sum over the reward history, fp64, ascending), the reward earned on each player's moves
 * (reward_of_player[p] = sum of rewards[i], i = 1 .. n, where to_play[i - 1] == p; [1] stays +0.0 in one-player games),
 * and the count and numpy's pairwise fp64 sum of the non-zero root values (a NaN counts, both zeros do not), from which
 * the host takes mean_value = value_sum / value_count = numpy.mean([v for v in root_values if v]), bit for bit.
 * 40 bytes per game. */
typedef struct mzreplay_game_outcome {
    double total_reward;
    double reward_of_player[2];
    double value_sum;
    int32_t value_count;
    int32_t reserved;
} mzreplay_game_outcome;

/* The rule on host arrays, for a game of n >= 1 moves in the store's row layout: rewards f64[n + 1], to_play i8[n + 1],
 * root_values f64[n].  Touches no device (the CPU tests hold it to Python's sum and numpy.mean).  -1 on a null pointer
 * or n < 1 (mzreplay_last_error(NULL)). */
int mzreplay_outcomes_reference(int32_t n, const double *rewards, const int8_t *to_play, const double *root_values,
                                mzreplay_game_outcome *out);
/* The outcomes of stored games, whichever way they were stored (mzreplay_add_games or a filer): `slots` host i32[n],
 * `outcomes` host [n].  One launch, a wavefront per game; an empty slot reports zeros.  Blocking, in the manner of
 * mzreplay_filer_priorities.  Refused on the arguments alone: a null pointer, n < 0, a slot outside the store. */
int mzreplay_game_outcomes(mzreplay *store, int32_t n, const int32_t *slots, mzreplay_game_outcome *outcomes, void *stream);
/* The filer reports the outcome of every game it finishes -- those a call drops because it finished more games than the
 * store has slots included -- in a list parallel to the one mzreplay_filer_sync_ids hands out: filer_append_kernel applies
 * the rule to the complete row where it finishes the game, before the row is reused.  Accepted only before
 * mzreplay_filer_begin (the kernel form and the scratch of max_moves doubles per env are chosen once).  Off by default:
 * the filer's launches then make the memory accesses they made before this switch existed.  A refused batch (rule 5)
 * reports no outcomes, like it reports no games. */
int mzreplay_filer_enable_outcomes(mzreplay_filer *filer, int32_t on);
/* The outcomes of the games the last mzreplay_filer_sync_ids / mzreplay_filer_sync of this filer returned, in that order
 * (a host array, valid until the next call on this filer): 40 bytes per game on top of the sync's 16.  No device work:
 * the sync fetched them.  Fails while the switch is off. */
int mzreplay_filer_sync_outcomes(mzreplay_filer *filer, int32_t *n, const mzreplay_game_outcome **outcomes);

/* ---- Reanalyse in batches (csrc/reanalyse_plan.h) ------------------------------------------------
 * N games per pass, queued on one stream: the games drawn on the device, every position of every drawn game evaluated
 * as one batch, the fresh values written back.  A pass is a PLAN -- device arrays game_ids i64[n], slots i32[n], row_start
 * i32[n + 1] -- and its consumers:
 *   1. draw d = numpy.random.choice(n_stored) from the pass's own MT19937 stream (n_stored == 1 consumes no word),
 *      game_ids[d] = oldest_game_id + index, slot = id % capacity; or the caller's ids, and the stream does not move;
 *   2. a draw whose game is drawn again later in the pass gets no rows: the last occurrence carries them;
 *   3. rows = the game's length for a carrying draw, 0 otherwise; row_start = their exclusive prefix sum and
 *      row_start[n] = R; row r belongs to the draw found by right bisection in row_start, at position r - row_start[d].
 * mzreplay_reanalyse_enable gives the store the stream, seeded as numpy.random.seed(seed) (calling it again reseeds),
 * and the pass's scratch.  Blocking, like _get_rng / _set_rng (RandomState.get_state() form: key u32[624], pos 0..624). */
struct mzmcts_fc_desc;   /* include/mzmcts.h */
int mzreplay_reanalyse_enable(mzreplay *store, uint32_t seed);
int mzreplay_reanalyse_get_rng(mzreplay *store, uint32_t *key, int32_t *pos);
int mzreplay_reanalyse_set_rng(mzreplay *store, const uint32_t *key, int32_t pos);
/* The plan of a pass of n_games draws (1..4096) in one launch.  given_ids: NULL, or host i64[n_games], each a stored
 * game (oldest_game_id <= id < oldest_game_id + n_stored).  Lengths are read from the store's own device array, so games
 * that were filed on the device work unchanged.  n_stored == 0: nothing is drawn, ids and slots are -1, R = 0.  A store
 * whose n_games * max_moves leaves int32 is refused.  Asynchronous. */
int mzreplay_reanalyse_plan(mzreplay *store, int32_t n_games, int64_t oldest_game_id, int32_t n_stored,
                            const int64_t *given_ids, int64_t *game_ids, int32_t *slots, int32_t *row_start, void *stream);
/* The stacked observation of every row of the plan: observations dev f32[n_rows][C'][H][W], compact, in row order -- the
 * input batch of initial_inference for any network.  n_rows: the rows the output holds (R, read back by the caller, or
 * an upper bound of it); rows past row_start[n_games] are not written.  Asynchronous. */
int mzreplay_reanalyse_observations(mzreplay *store, int32_t n_games, const int32_t *slots, const int32_t *row_start,
                                    int32_t n_rows, float *observations, void *stream);
/* values dev f32[R] into reanalysed[slot][0 .. length) of every carrying draw and has_reanalysed[slot] = 1, as
 * mzreplay_set_reanalysed leaves them; nothing else of the store is written and no slot without rows is touched.
 * Asynchronous. */
int mzreplay_reanalyse_store(mzreplay *store, int32_t n_games, const int32_t *slots, const int32_t *row_start,
                             const float *values, void *stream);
/* Read Reanalyse's values back (host outputs, each may be NULL): values f32[n][max_moves], the whole row of every slot in
 * `slots` (host i32[n]) as it sits in the store -- entries past a game's length are whatever was there --, and
 * has_values u8[n] (1: the slot's targets bootstrap from them).  Blocking. */
int mzreplay_read_reanalysed(mzreplay *store, int32_t n, const int32_t *slots, float *values, uint8_t *has_values,
                             void *stream);
/* The pass for a fully-connected network, in one launch behind the plan.  _fc_configure describes the network as
 * mzmcts_fc_configure does (weights: dev f32[n_weights] in state_dict order; the pointer is RETAINED, so a publish or a
 * broadcast into that buffer refreshes the network without a call) plus config.support_size; it refuses what
 * mzmcts_fc_configure refuses, an observation_floats that is not the store's stacked observation (or wider than 256
 * floats), and a network whose weights, neuron tables and activations exceed a workgroup's LDS.  Blocking.
 * _fc: per row the stacked observation is built in the lane group's LDS scratch, fc_initial and support_to_scalar_group
 * (csrc/fc_net_device.h, tree_device.h) run on it and the float32 value goes where mzreplay_reanalyse_store would put
 * it; no observation, logit or value passes through device memory on the way.  Asynchronous, allocation-free. */
int mzreplay_reanalyse_fc_configure(mzreplay *store, const struct mzmcts_fc_desc *desc, int32_t support_size,
                                    const float *weights, int64_t n_weights);
int mzreplay_reanalyse_fc(mzreplay *store, int32_t n_games, const int32_t *slots, const int32_t *row_start, void *stream);
/* Lanes of a wavefront that evaluate one row in mzreplay_reanalyse_fc (the decode's rounding depends on it). */
int32_t mzreplay_reanalyse_fc_group_width(void);

/* Bytes of device memory the store occupies. */
int64_t mzreplay_device_bytes(const mzreplay *store);

#ifdef __cplusplus
}
#endif
#endif /* MZREPLAY_H */
