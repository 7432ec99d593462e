// mzreplay.hip -- device-resident replay store and target kernels (include/mzreplay.h).
//
// Layout (game-slot major, a slot holds one game padded to max_moves = L):
//     obs f32 [G][L+1][obs] | actions i32 [G][L+1] | rewards f64 [G][L+1] | to_play i8 [G][L+1]
//     child_visits f64 [G][L][A] | root_values f64 [G][L] | length i32 [G]
// Both kernels are gather / short-scan work over these rows: HBM-bound, no contraction.
//   priorities_kernel   one workgroup per new game, one thread per position: the td_steps-long discounted
//                       reward sum in the reference's order, |root - target| ** alpha, block max
//   make_batch_kernel   one workgroup per sample: threads 0..U evaluate the U+1 unroll targets, all threads
//                       copy the policy rows and the (stacked) observation planes
// The sampler (mzreplay_sampler_enable; arithmetic in replay_sampler.h) keeps priorities f32 [G][L], game_priority
// f32 [G], game_id i64 [G] and numpy's MT19937 stream on the device and draws a batch in four launches:
//   sample_games_kernel      one workgroup: game probabilities (numpy's pairwise float32 sum, leaves in parallel), their
//                            fp64 running sum (ONE lane: the order of the additions is the contract), B game draws
//   position_tables_kernel   one wavefront per sample: the game's float32 sum and fp64 running sum (one lane each)
//   sample_walk_kernel       one wavefront walks the samples in batch order: position uniform, number of absorbing
//                            steps (from the table's last U entries, staged in LDS), their rejection draws 64 words
//                            at a time by ballot; the MT19937 twist runs across the lanes
//   sample_finish_kernel     positions by bisection, importance weights, batch maximum, all samples in parallel
// and update_priorities in two (writes with the reference's later-sample-wins order, then the game maxima).
// Reanalyse in batches (mzreplay_reanalyse_*; index arithmetic in reanalyse_plan.h) is a plan and its consumers:
//   reanalyse_plan_kernel          one workgroup: the draws (a wavefront consumes 64 words a round, all lanes twist), the last
//                                  occurrence of every game, the rows' exclusive prefix sum
//   reanalyse_observations_kernel  a workgroup per row, grid-stride: the network's input batch
//   reanalyse_store_kernel         a workgroup per draw, grid-stride: values into the slots of the carrying draws
//   reanalyse_fc_kernel            fully-connected networks: a fixed grid, weights and neuron tables staged once per
//                                  workgroup, a lane group per row from the observation to the stored value
// What a finished game reports (mzreplay_game_outcomes, mzreplay_filer_enable_outcomes; the rule in game_outcomes.h) is one
// device function, wave_outcome, a wavefront per game, with two callers:
//   game_outcomes_kernel           a workgroup of one wavefront per requested slot
//   filer_append_kernel<., true>   where the filer finishes a game, on the row it is about to copy
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mzreplay.h"
#include "fc_net_host.h"
#include "game_outcomes.h"
#include "reanalyse_plan.h"
#include "replay_filer.h"
#include "replay_sampler.h"

namespace {

struct StoreParams {
    int32_t G, L, A, obs_floats, C, H, W, stacked, td_steps, unroll;
    double alpha;
    float* obs;
    int32_t* actions;
    double* rewards;
    int8_t* to_play;
    double* child_visits;
    double* root_values;
    int32_t* length;
    float* reanalysed;           // [G][L] Reanalyse's fresh root values (float32, as the reference stores them)
    uint8_t* has_reanalysed;     // [G]
    const double* discount_pow;  // [td_steps + 1]
};

// ReplayBuffer.compute_target_value (replay_buffer.py:222-256), fp64, the reference's operation order
__device__ __forceinline__ double target_value(const StoreParams& p, int slot, int n, int index) {
    const double* rewards = p.rewards + static_cast<size_t>(slot) * (p.L + 1);
    const int8_t* to_play = p.to_play + static_cast<size_t>(slot) * (p.L + 1);
    const int bootstrap = index + p.td_steps;
    double value = 0.0;
    if (bootstrap < n && p.has_reanalysed[slot]) {
        // reanalysed_predicted_root_values is a numpy float32 array (replay_buffer.py:226-231, 351-353): under
        // NumPy 2 promotion the bootstrap product and every `value += python_float` stay float32
        float last = p.reanalysed[static_cast<size_t>(slot) * p.L + bootstrap];
        if (to_play[bootstrap] != to_play[index]) last = -last;
        float v32 = last * static_cast<float>(p.discount_pow[p.td_steps]);
        const int stop32 = bootstrap + 1 < n + 1 ? bootstrap + 1 : n + 1;
        for (int k = index + 1, i = 0; k < stop32; ++k, ++i) {
            const double r = rewards[k];
            const double signed_r = (to_play[index] == to_play[index + i]) ? r : -r;
            v32 = v32 + static_cast<float>(signed_r * p.discount_pow[i]);
        }
        return static_cast<double>(v32);
    }
    if (bootstrap < n) {
        double last = p.root_values[static_cast<size_t>(slot) * p.L + bootstrap];
        if (to_play[bootstrap] != to_play[index]) last = -last;
        value = last * p.discount_pow[p.td_steps];
    }
    // reward_history[index + 1 : bootstrap + 1]; the history has n + 1 entries
    const int stop = bootstrap + 1 < n + 1 ? bootstrap + 1 : n + 1;
    for (int k = index + 1, i = 0; k < stop; ++k, ++i) {
        const double r = rewards[k];
        const double signed_r = (to_play[index] == to_play[index + i]) ? r : -r;
        value += signed_r * p.discount_pow[i];
    }
    return value;
}

// ReplayBuffer.save_game's initial priority of one position (replay_buffer.py:33-50): |root value - target| ** alpha
__device__ __forceinline__ float position_priority(const StoreParams& p, int slot, int n, int i) {
    const double rv = p.root_values[static_cast<size_t>(slot) * p.L + i];
    return static_cast<float>(pow(fabs(rv - target_value(p, slot, n, i)), p.alpha));
}

__global__ __launch_bounds__(256) void priorities_kernel(StoreParams p, const int32_t* __restrict__ slots,
                                                         float* __restrict__ priorities,  // [n][L]
                                                         float* __restrict__ game_priority) {
    __shared__ float block_max[256];
    const int slot = slots[blockIdx.x];
    const int n = p.length[slot];
    float best = -INFINITY;
    for (int i = threadIdx.x; i < p.L; i += blockDim.x) {
        float pr = 0.f;
        if (i < n) {
            pr = position_priority(p, slot, n, i);
            best = fmaxf(best, pr);
        }
        priorities[static_cast<size_t>(blockIdx.x) * p.L + i] = pr;
    }
    block_max[threadIdx.x] = best;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) block_max[threadIdx.x] = fmaxf(block_max[threadIdx.x], block_max[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) game_priority[blockIdx.x] = block_max[0];
}

// GameHistory.get_stacked_observations (self_play.py:514-548): float t of the stacked observation of one position
__device__ __forceinline__ float stacked_element(const StoreParams& p, int slot, int pos, int t) {
    const int32_t* actions = p.actions + static_cast<size_t>(slot) * (p.L + 1);
    const int plane = p.H * p.W;
    const float* game_obs = p.obs + static_cast<size_t>(slot) * (p.L + 1) * p.obs_floats;
    const int ch = t / plane, px = t - ch * plane;
    if (ch < p.C) return game_obs[static_cast<size_t>(pos) * p.obs_floats + t];
    const int k = (ch - p.C) / (p.C + 1);        // k-th past frame: index pos - 1 - k
    const int c = (ch - p.C) - k * (p.C + 1);    // its channel; c == C is the action plane
    const int past = pos - 1 - k;
    if (past < 0) return 0.f;
    if (c < p.C) return game_obs[static_cast<size_t>(past) * p.obs_floats + c * plane + px];
    return static_cast<float>(actions[past + 1]);
}

// ... of one position, by the whole workgroup
__device__ __forceinline__ void stacked_observation(const StoreParams& p, int slot, int pos, float* out) {
    const int floats = (p.C + p.stacked * (p.C + 1)) * p.H * p.W;
    for (int t = threadIdx.x; t < floats; t += blockDim.x) out[t] = stacked_element(p, slot, pos, t);
}

// every position of one game, stacked: the input batch of Reanalyse's initial_inference (replay_buffer.py:335-346)
__global__ __launch_bounds__(128) void game_observations_kernel(StoreParams p, int slot, float* __restrict__ obs_out) {
    const int pos = blockIdx.x;
    if (pos >= p.length[slot]) return;
    stacked_observation(p, slot, pos, obs_out + static_cast<size_t>(pos) * (p.C + p.stacked * (p.C + 1)) * p.H * p.W);
}

// T = double: the reference's dtypes; T = float: the trainer's (the fp64 results rounded to nearest at the store)
template <typename T>
__global__ __launch_bounds__(128) void make_batch_kernel(StoreParams p, const int32_t* __restrict__ slots,
                                                         const int32_t* __restrict__ positions,
                                                         const int32_t* __restrict__ absorbing,  // [B][U+1]
                                                         float* __restrict__ obs_out, int64_t* __restrict__ actions_out,
                                                         T* __restrict__ values_out, T* __restrict__ rewards_out,
                                                         T* __restrict__ policies_out, T* __restrict__ scale_out) {
    const int b = blockIdx.x;
    const int slot = slots[b], pos = positions[b];
    if (slot < 0 || slot >= p.G || pos < 0 || pos > p.L) return;   // indices that come from the device are checked here
    const int n = p.length[slot];
    const int U1 = p.unroll + 1;
    const double* rewards = p.rewards + static_cast<size_t>(slot) * (p.L + 1);
    const int32_t* actions = p.actions + static_cast<size_t>(slot) * (p.L + 1);
    // ---- make_target (replay_buffer.py:258-295): one thread per unroll step
    for (int u = threadIdx.x; u < U1; u += blockDim.x) {
        const int cur = pos + u;
        const size_t o = static_cast<size_t>(b) * U1 + u;
        double value = 0.0, reward = 0.0;
        int64_t action;
        if (cur < n) {
            value = target_value(p, slot, n, cur);
            reward = rewards[cur];
            action = actions[cur];
        } else if (cur == n) {
            reward = rewards[cur];
            action = actions[cur];
        } else {
            action = absorbing[o];  // numpy.random.choice(action_space), drawn by the caller in the reference's order
        }
        values_out[o] = static_cast<T>(value);
        rewards_out[o] = static_cast<T>(reward);
        actions_out[o] = action;
        const int remaining = n + 1 - pos;  // len(action_history) - game_pos
        scale_out[o] = static_cast<T>(p.unroll < remaining ? p.unroll : remaining);
    }
    // ---- policies: child_visits[cur], or the uniform policy at and past the end of the game
    const double uniform = 1 / static_cast<double>(p.A);
    for (int t = threadIdx.x; t < U1 * p.A; t += blockDim.x) {
        const int u = t / p.A, a = t - u * p.A;
        const int cur = pos + u;
        policies_out[static_cast<size_t>(b) * U1 * p.A + t] =
            static_cast<T>(cur < n ? p.child_visits[(static_cast<size_t>(slot) * p.L + cur) * p.A + a] : uniform);
    }
    stacked_observation(p, slot, pos, obs_out + static_cast<size_t>(b) * (p.C + p.stacked * (p.C + 1)) * p.H * p.W);
}


// ---- the sampler (replay_sampler.h) ---------------------------------------------------------------------------------
struct SamplerParams {
    float* priorities;       // [G][L]
    float* game_priority;    // [G]
    int64_t* game_id;        // [G], -1 while the slot is empty
    uint32_t* mt_key;        // [624] numpy's stream as RandomState.get_state() gives it
    int32_t* mt_pos;         // [1]
    float* probs;            // [G] scratch where the game tables do not fit LDS
    double* cdf;             // [G]
    int32_t lds_games;       // 1: probabilities and their running sum live in LDS
    // one batch
    int32_t* game_len;       // [Bcap]
    float* game_prob;        // [Bcap]
    double* u_game;          // [Bcap]
    double* u_pos;           // [Bcap]
    float* totals;           // [Bcap]
    double* tables;          // [Bcap][L] normalised running sums of the sampled games' position probabilities
};

// pairwise leaves summed in parallel.  64 leaves per full piece of 8192: every store of up to 65 032 games has at most 512,
// 65 033 has 513, and the count is not monotone after that (65 040 and 65 536 are back at 512, 65 537 has 513).  More
// leaves than this: one lane adds them up.
constexpr int kMaxLeaves = 512;
constexpr int kSampleThreads = 256;

// the next block of 624 words, across the workgroup's (or the wavefront's) lanes: three ranges that each read only
// what the previous one wrote, then the last word.  `sync` separates them.
template <typename Sync>
__device__ __forceinline__ void twist_parallel(uint32_t* key, uint32_t* fresh, int lane, int lanes, Sync sync) {
    for (int k = lane; k < mz::kMtN - mz::kMtM; k += lanes) fresh[k] = mz::mt_mix(key[k], key[k + 1], key[k + mz::kMtM]);
    sync();
    for (int k = mz::kMtN - mz::kMtM + lane; k < 2 * (mz::kMtN - mz::kMtM); k += lanes)
        fresh[k] = mz::mt_mix(key[k], key[k + 1], fresh[k + mz::kMtM - mz::kMtN]);
    sync();
    for (int k = 2 * (mz::kMtN - mz::kMtM) + lane; k < mz::kMtN - 1; k += lanes)
        fresh[k] = mz::mt_mix(key[k], key[k + 1], fresh[k + mz::kMtM - mz::kMtN]);
    sync();
    if (lane == 0) fresh[mz::kMtN - 1] = mz::mt_mix(key[mz::kMtN - 1], fresh[0], fresh[mz::kMtM - 1]);
    sync();
    for (int k = lane; k < mz::kMtN; k += lanes) key[k] = fresh[k];
    sync();
}

__global__ __launch_bounds__(kSampleThreads) void sample_games_kernel(StoreParams p, SamplerParams s, int batch,
                                                                      int64_t oldest_id, int n_games, int per,
                                                                      int64_t* __restrict__ game_ids,
                                                                      int32_t* __restrict__ slots) {
    extern __shared__ double lds_dyn[];
    __shared__ uint32_t key[mz::kMtN], fresh[mz::kMtN];
    __shared__ int32_t leaf_off[kMaxLeaves], leaf_len[kMaxLeaves];
    __shared__ float leaf_sum[kMaxLeaves];
    __shared__ float total_s;
    __shared__ int32_t leaves_s, pos_s, done_s, have_hi_s;
    __shared__ uint32_t hi_s;
    const int t = threadIdx.x;
    double* cdf = s.lds_games ? lds_dyn : s.cdf;
    float* probs = s.lds_games ? reinterpret_cast<float*>(lds_dyn + p.G) : s.probs;
    auto sync = [] { __syncthreads(); };
    for (int k = t; k < mz::kMtN; k += kSampleThreads) key[k] = s.mt_key[k];
    if (t == 0) {
        pos_s = s.mt_pos[0];
        done_s = 0;
        have_hi_s = 0;
    }
    if (per) {
        // game_probs in ring order, oldest to newest
        for (int i = t; i < n_games; i += kSampleThreads)
            probs[i] = s.game_priority[static_cast<int>((oldest_id + i) % p.G)];
        __syncthreads();
        if (t == 0) {
            int count = 0;
            mz::replay::numpy_sum_walk(n_games, [&](int off, int len) {
                if (count < kMaxLeaves) {
                    leaf_off[count] = off;
                    leaf_len[count] = len;
                }
                ++count;
                return 0.f;
            });
            leaves_s = count;
        }
        __syncthreads();
        const int leaves = leaves_s;
        auto at = [&](int i) { return probs[i]; };
        if (leaves <= kMaxLeaves) {
            for (int k = t; k < leaves; k += kSampleThreads) leaf_sum[k] = mz::replay::pairwise_leaf(at, leaf_off[k], leaf_len[k]);
            __syncthreads();
            if (t == 0) {
                int k = 0;
                total_s = mz::replay::numpy_sum_walk(n_games, [&](int, int) { return leaf_sum[k++]; });
            }
        } else if (t == 0) {
            total_s = mz::replay::numpy_sum_f32(at, n_games);
        }
        __syncthreads();
        const float total = total_s;
        for (int i = t; i < n_games; i += kSampleThreads) {
            const float q = probs[i] / total;
            probs[i] = q;
            cdf[i] = static_cast<double>(q);
        }
        __syncthreads();
        if (t == 0) {   // cumsum: one chain of fp64 additions, left to right
            double run = 0.0;
            for (int i = 0; i < n_games; ++i) {
                run += cdf[i];
                cdf[i] = run;
            }
        }
        __syncthreads();
        const double last = cdf[n_games - 1];
        __syncthreads();
        for (int i = t; i < n_games; i += kSampleThreads) cdf[i] = cdf[i] / last;
    }
    __syncthreads();
    // B game draws: lane 0 consumes the words, every lane helps with the twist
    const uint32_t top = static_cast<uint32_t>(n_games) - 1u;
    const uint32_t mask = mz::mask_for(top);
    if (!per && top == 0u) {
        for (int b = t; b < batch; b += kSampleThreads) s.game_len[b] = 0;   // (index 0; filled in below)
        if (t == 0) done_s = batch;
        __syncthreads();
    }
    while (done_s < batch) {
        if (pos_s >= mz::kMtN) {
            twist_parallel(key, fresh, t, kSampleThreads, sync);
            if (t == 0) pos_s = 0;
        }
        __syncthreads();
        if (t == 0) {
            int pos = pos_s, b = done_s;
            while (pos < mz::kMtN && b < batch) {
                const uint32_t w = mz::mt_temper(key[pos++]);
                if (per) {
                    if (!have_hi_s) {
                        hi_s = w;
                        have_hi_s = 1;
                    } else {
                        s.u_game[b++] = mz::replay::uniform_from_words(hi_s, w);
                        have_hi_s = 0;
                    }
                } else if ((w & mask) <= top) {
                    s.game_len[b++] = static_cast<int32_t>(w & mask);   // the drawn index, replaced by the length below
                }
            }
            pos_s = pos;
            done_s = b;
        }
        __syncthreads();
    }
    for (int b = t; b < batch; b += kSampleThreads) {
        int g;
        if (per) {
            g = mz::replay::bisect_right([&](int i) { return cdf[i]; }, n_games, s.u_game[b]);
            if (g >= n_games) g = n_games - 1;
            s.game_prob[b] = probs[g];
        } else {
            g = s.game_len[b];
        }
        const int64_t id = oldest_id + g;
        const int slot = static_cast<int>(id % p.G);
        game_ids[b] = id;
        slots[b] = slot;
        s.game_len[b] = p.length[slot];
    }
    __syncthreads();
    for (int k = t; k < mz::kMtN; k += kSampleThreads) s.mt_key[k] = key[k];
    if (t == 0) s.mt_pos[0] = pos_s;
}

// one wavefront per sample: position_probs = priorities / sum(priorities) and choice()'s table for it
__global__ __launch_bounds__(64) void position_tables_kernel(StoreParams p, SamplerParams s, int lds_rows,
                                                             const int32_t* __restrict__ slots) {
    extern __shared__ double lds_dyn[];
    __shared__ float total_s;
    const int b = blockIdx.x, t = threadIdx.x;
    const int slot = slots[b];
    const int n = s.game_len[b];
    const float* pri = s.priorities + static_cast<size_t>(slot) * p.L;
    double* row = s.tables + static_cast<size_t>(b) * p.L;
    double* work = lds_rows ? lds_dyn : row;
    for (int i = t; i < n; i += 64) work[i] = static_cast<double>(pri[i]);   // (exact both ways)
    __syncthreads();
    if (t == 0) total_s = mz::replay::python_sum_f32([&](int i) { return static_cast<float>(work[i]); }, n);
    __syncthreads();
    const float total = total_s;
    for (int i = t; i < n; i += 64) work[i] = static_cast<double>(static_cast<float>(work[i]) / total);
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int i = 0; i < n; ++i) {
            run += work[i];
            work[i] = run;
        }
        s.totals[b] = total;
    }
    __syncthreads();
    const double last = work[n - 1];
    __syncthreads();
    for (int i = t; i < n; i += 64) row[i] = work[i] / last;
}

// One wavefront, every lane in step: the part of a batch whose word positions depend on the draws before them.
__global__ __launch_bounds__(64) void sample_walk_kernel(StoreParams p, SamplerParams s, int batch, int per, int tail,
                                                         int lds_tails, int32_t* __restrict__ positions,
                                                         int32_t* __restrict__ absorbing) {
    extern __shared__ double lds_dyn[];   // [batch] lengths as i32 behind [batch][tail] table ends
    __shared__ uint32_t key[mz::kMtN], fresh[mz::kMtN];
    const int lane = threadIdx.x;
    const int U = p.unroll, U1 = p.unroll + 1;
    double* tails = lds_dyn;
    int32_t* len_s = reinterpret_cast<int32_t*>(lds_dyn + (lds_tails ? static_cast<size_t>(batch) * tail : 0));
    auto sync = [] { __syncthreads(); };
    for (int k = lane; k < mz::kMtN; k += 64) key[k] = s.mt_key[k];
    for (int b = lane; b < batch; b += 64) len_s[b] = s.game_len[b];
    __syncthreads();
    // entry j of sample b's tail is table entry max(0, n - U) + j: the positions from which unrolling passes the end
    auto tail_entry = [&](int b, int j) {
        const int n = len_s[b];
        const int i = (n - U > 0 ? n - U : 0) + j;
        return i < n ? s.tables[static_cast<size_t>(b) * p.L + i] : INFINITY;
    };
    if (per && lds_tails)
        for (int idx = lane; idx < batch * tail; idx += 64) tails[idx] = tail_entry(idx / tail, idx % tail);
    __syncthreads();
    int wp = s.mt_pos[0];
    const uint32_t top_a = static_cast<uint32_t>(p.A) - 1u;
    const uint32_t mask_a = mz::mask_for(top_a);
    auto word = [&]() {   // the next word, for every lane
        if (wp >= mz::kMtN) {
            twist_parallel(key, fresh, lane, 64, sync);
            wp = 0;
        }
        return mz::mt_temper(key[wp++]);
    };
    for (int b = 0; b < batch; ++b) {
        const int n = len_s[b];
        int c;   // unrolled steps past the end of the game
        if (per) {
            const uint32_t w0 = word(), w1 = word();
            const double u = mz::replay::uniform_from_words(w0, w1);
            if (lane == 0) s.u_pos[b] = u;
            int beyond = 0;   // table entries <= u among the last min(U, n): the position is that far into the tail
            for (int j0 = 0; j0 < tail; j0 += 64) {
                const int j = j0 + lane;
                const bool le = j < tail && (lds_tails ? tails[static_cast<size_t>(b) * tail + j] : tail_entry(b, j)) <= u;
                beyond += __popcll(__ballot(le));
            }
            c = beyond + (U - n > 0 ? U - n : 0);
        } else {
            const uint32_t top = static_cast<uint32_t>(n) - 1u;
            const uint32_t mask = mz::mask_for(top);
            uint32_t v = 0u;
            if (top != 0u) do { v = word() & mask; } while (v > top);
            if (lane == 0) positions[b] = static_cast<int32_t>(v);
            c = mz::replay::absorbing_steps(static_cast<int>(v), n, U);
        }
        if (c > U1) c = U1;
        int u_next = U1 - c;
        if (top_a == 0u) c = 0;   // one action: choice() consumes nothing and answers 0 (the rows are zeroed)
        while (c > 0) {           // masked rejection, up to 64 words per round
            if (wp >= mz::kMtN) {
                twist_parallel(key, fresh, lane, 64, sync);
                wp = 0;
            }
            const int avail = mz::kMtN - wp < 64 ? mz::kMtN - wp : 64;
            const uint32_t v = lane < avail ? (mz::mt_temper(key[wp + lane]) & mask_a) : 0u;
            const bool ok = lane < avail && v <= top_a;
            unsigned long long accepted = __ballot(ok);
            const int k = __popcll(accepted);
            const int rank = __popcll(accepted & ((1ull << lane) - 1ull));
            int consumed = avail;
            if (k >= c) {         // the c-th accepted word ends the sample
                unsigned long long m = accepted;
                for (int r = 1; r < c; ++r) m &= m - 1ull;
                consumed = __ffsll(static_cast<long long>(m));
            }
            if (ok && rank < c) absorbing[static_cast<size_t>(b) * U1 + u_next + rank] = static_cast<int32_t>(v);
            const int took = k < c ? k : c;
            u_next += took;
            c -= took;
            wp += consumed;
        }
    }
    __syncthreads();
    for (int k = lane; k < mz::kMtN; k += 64) s.mt_key[k] = key[k];
    if (lane == 0) s.mt_pos[0] = wp;
}

// positions, importance weights and their maximum: nothing here depends on the stream
__global__ __launch_bounds__(kSampleThreads) void sample_finish_kernel(StoreParams p, SamplerParams s, int batch,
                                                                       int64_t total_samples,
                                                                       const int32_t* __restrict__ slots,
                                                                       int32_t* __restrict__ positions,
                                                                       float* __restrict__ weights) {
    __shared__ float block_max[kSampleThreads];
    const int t = threadIdx.x;
    float best = -INFINITY;
    for (int b = t; b < batch; b += kSampleThreads) {
        const int n = s.game_len[b];
        const double* row = s.tables + static_cast<size_t>(b) * p.L;
        int pos = mz::replay::bisect_right([&](int i) { return row[i]; }, n, s.u_pos[b]);
        if (pos >= n) pos = n - 1;
        positions[b] = pos;
        const float pos_prob = s.priorities[static_cast<size_t>(slots[b]) * p.L + pos] / s.totals[b];
        const float w = mz::replay::importance_weight(total_samples, s.game_prob[b], pos_prob);
        weights[b] = w;
        best = w > best ? w : best;
    }
    block_max[t] = best;
    __syncthreads();
    for (int half = kSampleThreads / 2; half > 0; half >>= 1) {
        if (t < half) block_max[t] = block_max[t + half] > block_max[t] ? block_max[t + half] : block_max[t];
        __syncthreads();
    }
    const float top = block_max[0];
    for (int b = t; b < batch; b += kSampleThreads) weights[b] = weights[b] / top;
}

// update_priorities, first half: one workgroup per sample writes its row, except where a later sample of the same game
// covers the position (the reference applies the samples in batch order)
__global__ __launch_bounds__(128) void update_priorities_kernel(StoreParams p, SamplerParams s, int batch,
                                                                const int64_t* __restrict__ game_ids,
                                                                const int32_t* __restrict__ positions,
                                                                const float* __restrict__ fresh) {
    extern __shared__ double lds_dyn[];   // [batch] game ids, [batch] positions
    int64_t* ids = reinterpret_cast<int64_t*>(lds_dyn);
    int32_t* pos = reinterpret_cast<int32_t*>(ids + batch);
    const int b = blockIdx.x, U1 = p.unroll + 1;
    for (int i = threadIdx.x; i < batch; i += blockDim.x) {
        ids[i] = game_ids[i];
        pos[i] = positions[i];
    }
    __syncthreads();
    const int64_t id = ids[b];
    if (id < 0 || pos[b] < 0) return;
    const int slot = static_cast<int>(id % p.G);
    if (s.game_id[slot] != id) return;   // the game was removed since its selection
    const int n = p.length[slot];
    for (int k = threadIdx.x; k < U1 && pos[b] + k < n; k += blockDim.x)
        if (mz::replay::update_survives(b, k, batch, U1, [&](int i) { return ids[i]; }, [&](int i) { return pos[i]; }, n))
            s.priorities[static_cast<size_t>(slot) * p.L + pos[b] + k] = fresh[static_cast<size_t>(b) * U1 + k];
}

// second half: game_priority = numpy.max(priorities) of every touched game (samples of one game write the same value)
__global__ __launch_bounds__(64) void game_priority_kernel(StoreParams p, SamplerParams s,
                                                           const int64_t* __restrict__ game_ids) {
    __shared__ float lane_max[64];
    const int64_t id = game_ids[blockIdx.x];
    if (id < 0) return;
    const int slot = static_cast<int>(id % p.G);
    if (s.game_id[slot] != id) return;
    const int n = p.length[slot];
    const float* pri = s.priorities + static_cast<size_t>(slot) * p.L;
    float best = pri[0];
    for (int i = threadIdx.x; i < n; i += 64) best = mz::replay::numpy_max2(best, pri[i]);
    lane_max[threadIdx.x] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 64; ++i) best = mz::replay::numpy_max2(best, lane_max[i]);
        s.game_priority[slot] = best;
    }
}

// mzreplay_add_games with the sampler on: the new games' priorities, game priorities and ids into the sampler's arrays
__global__ __launch_bounds__(256) void adopt_games_kernel(StoreParams p, SamplerParams s, int n_new, int64_t first_id,
                                                          const int32_t* __restrict__ slots,
                                                          const float* __restrict__ priorities,
                                                          const float* __restrict__ game_priority) {
    const int g = blockIdx.x;
    const int slot = slots[g];
    for (int later = g + 1; later < n_new; ++later)
        if (slots[later] == slot) return;   // overwritten within this call
    for (int i = threadIdx.x; i < p.L; i += blockDim.x)
        s.priorities[static_cast<size_t>(slot) * p.L + i] = priorities[static_cast<size_t>(g) * p.L + i];
    if (threadIdx.x == 0) {
        s.game_priority[slot] = game_priority[g];
        s.game_id[slot] = first_id + g;
    }
}

// ---- Reanalyse in batches (reanalyse_plan.h) --------------------------------------------------------------------------
struct ReanalyseParams {
    uint32_t* mt_key;        // [624] the pass's own numpy stream
    int32_t* mt_pos;         // [1]
    int32_t* last_draw;      // [G] scratch of a plan: the last draw that names the slot
    int64_t* given_ids;      // [kMaxGames] staging of ids handed in by the caller
};

constexpr int kPlanThreads = 256;
constexpr int kReanalyseGroup = 16;    // lanes per row in reanalyse_fc_kernel
constexpr int kReanalyseThreads = 256;
constexpr int kReanalyseRowsPerBlock = kReanalyseThreads / kReanalyseGroup;

// One workgroup.  Stored ids are consecutive, so two draws name the same game exactly when they name the same slot: the
// last occurrence of a game is the largest draw index its slot has seen (an LDS-free atomicMax per draw on a [G] array).
__global__ __launch_bounds__(kPlanThreads) void reanalyse_plan_kernel(StoreParams p, ReanalyseParams r, int n_games,
                                                                      int64_t oldest_id, int n_stored, int given,
                                                                      int64_t* __restrict__ game_ids,
                                                                      int32_t* __restrict__ slots,
                                                                      int32_t* __restrict__ row_start) {
    __shared__ uint32_t key[mz::kMtN], fresh[mz::kMtN];
    __shared__ int32_t index_s[mz::reanalyse::kMaxGames];   // the draws; then rows per draw
    __shared__ int32_t part[2][kPlanThreads];
    __shared__ int32_t pos_s, done_s;
    const int t = threadIdx.x;
    if (n_stored <= 0) {
        for (int d = t; d < n_games; d += kPlanThreads) {
            game_ids[d] = -1;
            slots[d] = -1;
        }
        for (int d = t; d <= n_games; d += kPlanThreads) row_start[d] = 0;
        return;
    }
    if (!given) {
        auto sync = [] { __syncthreads(); };
        for (int k = t; k < mz::kMtN; k += kPlanThreads) key[k] = r.mt_key[k];
        if (t == 0) {
            pos_s = r.mt_pos[0];
            done_s = 0;
        }
        __syncthreads();
        const uint32_t top = static_cast<uint32_t>(n_stored) - 1u;
        const uint32_t mask = mz::mask_for(top);
        if (top == 0u) {   // choice(1): no word, index 0
            for (int d = t; d < n_games; d += kPlanThreads) index_s[d] = 0;
            if (t == 0) done_s = n_games;
            __syncthreads();
        }
        while (done_s < n_games) {
            if (pos_s >= mz::kMtN) {
                twist_parallel(key, fresh, t, kPlanThreads, sync);
                if (t == 0) pos_s = 0;
            }
            __syncthreads();
            if (t < 64) {   // the first wavefront: masked rejection, up to 64 words per round, accepted words ranked by ballot
                int pos = pos_s, d = done_s;
                while (pos < mz::kMtN && d < n_games) {
                    const int avail = mz::kMtN - pos < 64 ? mz::kMtN - pos : 64;
                    const uint32_t v = t < avail ? (mz::mt_temper(key[pos + t]) & mask) : 0u;
                    const bool ok = t < avail && v <= top;
                    const unsigned long long accepted = __ballot(ok);
                    const int k = __popcll(accepted);
                    const int rank = __popcll(accepted & ((1ull << t) - 1ull));
                    const int need = n_games - d;
                    int consumed = avail;
                    if (k >= need) {   // the need-th accepted word ends the pass: the words behind it stay in the stream
                        unsigned long long m = accepted;
                        for (int i = 1; i < need; ++i) m &= m - 1ull;
                        consumed = __ffsll(static_cast<long long>(m));
                    }
                    if (ok && rank < need) index_s[d + rank] = static_cast<int32_t>(v);
                    d += k < need ? k : need;
                    pos += consumed;
                }
                if (t == 0) {
                    pos_s = pos;
                    done_s = d;
                }
            }
            __syncthreads();
        }
        for (int k = t; k < mz::kMtN; k += kPlanThreads) r.mt_key[k] = key[k];
        if (t == 0) r.mt_pos[0] = pos_s;
    }
    for (int d = t; d < n_games; d += kPlanThreads) {
        const int64_t id = given ? r.given_ids[d] : oldest_id + index_s[d];
        const int slot = mz::reanalyse::slot_of(id, p.G);
        game_ids[d] = id;
        slots[d] = slot;
        __hip_atomic_store(&r.last_draw[slot], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (int d = t; d < n_games; d += kPlanThreads) atomicMax(&r.last_draw[slots[d]], d);
    __syncthreads();
    for (int d = t; d < n_games; d += kPlanThreads) {
        const int slot = slots[d];
        int rows = 0;
        if (__hip_atomic_load(&r.last_draw[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == d) {   // (past the L1)
            rows = p.length[slot];
            rows = rows < 0 ? 0 : (rows > p.L ? p.L : rows);
        }
        index_s[d] = rows;
    }
    __syncthreads();
    // exclusive prefix sum: a contiguous piece per thread, the pieces' sums scanned across the workgroup
    const int piece = (n_games + kPlanThreads - 1) / kPlanThreads;
    const int lo = t * piece < n_games ? t * piece : n_games;
    const int hi = lo + piece < n_games ? lo + piece : n_games;
    int32_t sum = 0;
    for (int d = lo; d < hi; ++d) sum += index_s[d];
    int cur = 0;
    part[0][t] = sum;
    __syncthreads();
    for (int step = 1; step < kPlanThreads; step <<= 1) {   // inclusive scan of the pieces' sums
        part[cur ^ 1][t] = part[cur][t] + (t >= step ? part[cur][t - step] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (t == kPlanThreads - 1) row_start[n_games] = part[cur][t];
    int32_t run = part[cur][t] - sum;
    for (int d = lo; d < hi; ++d) {
        row_start[d] = run;
        run += index_s[d];
    }
}

// (draw, slot, position) of row r; false where an index read from the plan does not fit the store
__device__ __forceinline__ bool reanalyse_row(const StoreParams& p, int n_games, const int32_t* __restrict__ slots,
                                              const int32_t* __restrict__ row_start, int r, int* slot, int* pos) {
    const int d = mz::reanalyse::draw_of_row([&](int i) { return row_start[i]; }, n_games, r);
    if (d < 0 || d >= n_games) return false;
    *slot = slots[d];
    *pos = r - row_start[d];
    return *slot >= 0 && *slot < p.G && *pos >= 0 && *pos < p.L;
}

__global__ __launch_bounds__(128) void reanalyse_observations_kernel(StoreParams p, int n_games,
                                                                     const int32_t* __restrict__ slots,
                                                                     const int32_t* __restrict__ row_start, int n_rows,
                                                                     float* __restrict__ obs_out) {
    const int total = row_start[n_games] < n_rows ? row_start[n_games] : n_rows;
    const size_t floats = static_cast<size_t>(p.C + p.stacked * (p.C + 1)) * p.H * p.W;
    for (int r = blockIdx.x; r < total; r += gridDim.x) {
        int slot, pos;
        if (!reanalyse_row(p, n_games, slots, row_start, r, &slot, &pos)) continue;
        stacked_observation(p, slot, pos, obs_out + static_cast<size_t>(r) * floats);
    }
}

__global__ __launch_bounds__(128) void reanalyse_store_kernel(StoreParams p, int n_games, const int32_t* __restrict__ slots,
                                                              const int32_t* __restrict__ row_start,
                                                              const float* __restrict__ values) {
    for (int d = blockIdx.x; d < n_games; d += gridDim.x) {
        const int first = row_start[d];
        int rows = row_start[d + 1] - first;
        const int slot = slots[d];
        if (rows <= 0 || first < 0 || slot < 0 || slot >= p.G) continue;
        rows = rows > p.L ? p.L : rows;
        for (int i = threadIdx.x; i < rows; i += blockDim.x)
            p.reanalysed[static_cast<size_t>(slot) * p.L + i] = values[static_cast<size_t>(first) + i];
        if (threadIdx.x == 0) p.has_reanalysed[slot] = 1;
    }
}

// Reanalyse for a fully-connected network.  Dynamic LDS: [padded weights][neuron tables of initial_inference]
// [kReanalyseRowsPerBlock activation scratches].  R is only known on the device: the grid is fixed, every workgroup stages
// the weights once and walks rows blockIdx.x * 16 + group, stride gridDim.x * 16.  Rows are independent: after the staging
// nothing is exchanged between lane groups, and a group that runs out of rows leaves.
template <int G>
__global__ __launch_bounds__(kReanalyseThreads) void reanalyse_fc_kernel(StoreParams p, mz::FcNet net,
                                                                         const float* __restrict__ weights, int n_games,
                                                                         const int32_t* __restrict__ slots,
                                                                         const int32_t* __restrict__ row_start) {
    extern __shared__ __attribute__((aligned(16))) float re_smem[];
    const int total = row_start[n_games];
    if (static_cast<int>(blockIdx.x) * kReanalyseRowsPerBlock >= total) return;   // (block-uniform: before any barrier)
    float* w_lds = re_smem;
    mz::NeuronDesc* table = reinterpret_cast<mz::NeuronDesc*>(re_smem + ((net.n_weights_lds + 3) & ~3));
    mz::stage_mlp_weights(net.repr, weights, w_lds, threadIdx.x, kReanalyseThreads);
    mz::stage_mlp_weights(net.policy, weights, w_lds, threadIdx.x, kReanalyseThreads);
    mz::stage_mlp_weights(net.value, weights, w_lds, threadIdx.x, kReanalyseThreads);
    __syncthreads();
    int entries = mz::build_phase_tables(net.init_pre, net.n_init_pre, w_lds, table, G, threadIdx.x, kReanalyseThreads);
    entries += mz::build_phase_tables(net.init_post, net.n_init_post, w_lds, table + entries, G, threadIdx.x, kReanalyseThreads);
    __syncthreads();
    const int group = threadIdx.x / G, j = threadIdx.x % G;
    float* scratch = reinterpret_cast<float*>(table + entries) + static_cast<size_t>(group) * net.scratch_floats;
    mz::fc_clear_scratch<G>(net, scratch, j);
    for (int r = blockIdx.x * kReanalyseRowsPerBlock + group; r < total; r += gridDim.x * kReanalyseRowsPerBlock) {
        int slot, pos;
        if (!reanalyse_row(p, n_games, slots, row_start, r, &slot, &pos)) continue;
        for (int t = j; t < net.obs; t += G) scratch[t] = stacked_element(p, slot, pos, t);
        mz::group_memory_fence();
        mz::fc_initial<G>(net, table, w_lds, scratch, scratch, j);   // (the observation is in place: x <- x)
        const float value = mz::support_to_scalar_group<G>(scratch + net.off_value, net.F, net.support, j);
        if (j == 0) {
            p.reanalysed[static_cast<size_t>(slot) * p.L + pos] = value;
            if (pos == 0) p.has_reanalysed[slot] = 1;
        }
        mz::group_memory_fence();   // the logits are read before the next row's layers overwrite them
    }
}

// ---- the filer (replay_filer.h; include/mzreplay.h mzreplay_filer_file) ------------------------------------------------
// Three launches per move batch, no host decision in between:
//   filer_count_kernel        a thread per env: prefix of played moves, validation of everything later used as an index,
//                             games finished
//   filer_scan_kernel         one workgroup: exclusive scan of the E counts in LDS, 1024 at a time; the call's plan
//                             (first id, games, how many a wrap drops), the lengths of the stored games the call evicts,
//                             the counters
//   filer_append_kernel       a wavefront per env walks its moves in order: lanes spread over the policy entries and the
//                             observation floats; a finished game's row goes to its slot in coalesced copies
//                             (with outcomes on, game_outcomes.h's rule on the complete row, same launch)
//   filer_priorities_kernel   a fixed grid strides over the call's surviving games: priorities_kernel's arithmetic into the
//                             priority arrays (the sampler's when it is on, with the game id)
// The store-wide counters are one device block of the store (FilerParams::shared), which the calls of every filer move in
// the order the host made them (mzreplay_filer_file chains the calls with the store's "last filing" event).
struct FilerState {                  // a filer's own block of device memory, read back whole by mzreplay_filer_sync
    int32_t pending;                 // games in the list since the last sync
    int32_t error;                   // mz::filer::kErr* bits
};

struct FilerParams {
    int32_t E;
    float* obs;                      // the running games, one row per env, in the store's slot layout
    int32_t* actions;
    double* rewards;
    int8_t* to_play;
    double* child_visits;
    double* root_values;
    int32_t* length;
    int32_t* played;                 // [E] scratch of a call: prefix length, games finished, their first rank
    int32_t* count;
    int32_t* offset;
    FilerState* state;
    mz::filer::Counters* shared;     // the store's counters: one block for all its filers
    mz::filer::Call* call;
    int32_t* list_env;               // [list_cap] games filed since the last sync
    int32_t* list_len;
    int64_t* list_id;                // (another filer's calls may lie between two of this one's: ids are not consecutive)
    int32_t list_cap;
    float* priorities;               // [G][L], [G]: the sampler's arrays when it is on, else the filer's own
    float* game_priority;
    int64_t* game_id;                // the sampler's [G], or null
    mz::outcomes::Outcome* list_out; // [list_cap] parallel to the list (mzreplay_filer_enable_outcomes), else null
    double* packed;                  // [E][L] an env's counted root values, compacted (outcomes on), else null
};

constexpr int kScanThreads = 1024;
constexpr int kFilerWave = 64;

template <typename T>
__device__ __forceinline__ const T* move_block(const void* base, int64_t stride, int m) {
    return reinterpret_cast<const T*>(static_cast<const uint8_t*>(base) + stride * m);
}

__global__ __launch_bounds__(256) void filer_count_kernel(StoreParams p, FilerParams f, mzreplay_file_moves mv) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= f.E) return;
    const int E = f.E, A = p.A, M = mv.n_moves;
    const int k = mz::filer::prefix_length(M, [&](int m) { return move_block<int32_t>(mv.actions, mv.actions_stride, m)[e]; });
    bool bad_legal = false;
    for (int m = 0; m < k; ++m) {
        const int n_legal = move_block<int32_t>(mv.num_legal, mv.num_legal_stride, m)[e];
        if (n_legal < 0 || n_legal > A) {
            bad_legal = true;
        } else {
            const int32_t* legal = move_block<int32_t>(mv.legal, mv.legal_stride, m) + static_cast<size_t>(e) * A;
            for (int i = 0; i < n_legal; ++i) bad_legal |= legal[i] < 0 || legal[i] >= A;
        }
    }
    int len = f.length[e];
    bool overflow = len < 0 || len > p.L;
    const int count = mz::filer::count_finished(&len, k, p.L, [&](int m) { return mv.done[static_cast<size_t>(m) * E + e] != 0; },
                                                &overflow);
    f.played[e] = k;
    f.count[e] = count;
    if (bad_legal) atomicOr(&f.state->error, mz::filer::kErrLegal);
    if (overflow) atomicOr(&f.state->error, mz::filer::kErrOverflow);
}

__global__ __launch_bounds__(kScanThreads) void filer_scan_kernel(StoreParams p, FilerParams f) {
    __shared__ int32_t scan[2][kScanThreads];
    __shared__ long long evicted_s[kScanThreads];
    const int t = threadIdx.x;
    // exclusive scan, a chunk of 1024 counts at a time (mz::filer::exclusive_scan_chunked is its serial statement)
    int32_t carry = 0;
    for (int base = 0; base < f.E; base += kScanThreads) {
        const int e = base + t;
        const int32_t own = e < f.E ? f.count[e] : 0;
        int cur = 0;
        scan[0][t] = own;
        __syncthreads();
        for (int step = 1; step < kScanThreads; step <<= 1) {
            scan[cur ^ 1][t] = scan[cur][t] + (t >= step ? scan[cur][t - step] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (e < f.E) f.offset[e] = carry + scan[cur][t] - own;
        carry += scan[cur][kScanThreads - 1];
        __syncthreads();
    }
    const mz::filer::Counters before = *f.shared;
    const bool refused = f.state->error != 0;
    const int64_t list_room = static_cast<int64_t>(f.list_cap) - f.state->pending;
    // (the host sized the list for E x M games per unsynced call: a call that does not fit is refused whole)
    const bool no_room = carry > list_room;
    const mz::filer::Call call = mz::filer::plan_call(before, carry, p.G, f.state->pending, refused || no_room);
    // the stored games this call evicts lose their lengths from total_samples: read before any slot is rewritten
    const int64_t evicted = mz::filer::evicted_old(before, call.n_new, p.G);
    const int64_t first = mz::filer::first_evicted_id(before);
    long long sum = 0;
    for (int64_t j = t; j < evicted; j += kScanThreads) sum += p.length[mz::filer::slot_of(first + j, p.G)];
    evicted_s[t] = sum;
    __syncthreads();
    for (int half = kScanThreads / 2; half > 0; half >>= 1) {
        if (t < half) evicted_s[t] += evicted_s[t + half];
        __syncthreads();
    }
    if (t == 0) {
        if (no_room) atomicOr(&f.state->error, mz::filer::kErrList);
        // (the new games' own lengths are added by the wavefronts that file them)
        *f.shared = mz::filer::counters_after(before, call.n_new, p.G, 0, 0, evicted_s[0]);
        f.state->pending += call.n_new;
        *f.call = call;
    }
}

template <bool kVec4>
__device__ __forceinline__ void copy_floats(float* __restrict__ dst, const float* __restrict__ src, size_t count, int lane) {
    if (kVec4) {   // (count % 4 == 0 and both 16-byte aligned: the host checked)
        float4* d4 = reinterpret_cast<float4*>(dst);
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (size_t i = lane; i < count / 4; i += kFilerWave) d4[i] = s4[i];
    } else {
        for (size_t i = lane; i < count; i += kFilerWave) dst[i] = src[i];
    }
}

template <typename T>
__device__ __forceinline__ void copy_items(T* __restrict__ dst, const T* __restrict__ src, size_t count, int lane) {
    for (size_t i = lane; i < count; i += kFilerWave) dst[i] = src[i];
}

// ---- what a finished game reports (game_outcomes.h) -----------------------------------------------------------------------
// One wavefront and one complete row: the counted root values are compacted in order by ballot into `packed` (room for n
// doubles), every lane sums the leaves of numpy's tree whose turn is its own and leaves each sum in the leaf's first
// cell (only that lane reads the leaf), and one lane adds the leaves up as the recursion would, its stack in LDS (`walk`:
// 640 bytes whatever max_moves is; four indexed arrays in registers cost the kernel its occupancy).  The three reward
// sums are one ascending chain each, on lanes 0..2 in step.  Called by all 64 lanes of a one-wavefront workgroup.
__device__ __forceinline__ void wave_outcome(const double* __restrict__ rewards, const int8_t* __restrict__ to_play,
                                             const double* __restrict__ root_values, int n, double* __restrict__ packed,
                                             mz::outcomes::Outcome* __restrict__ out, mz::outcomes::WalkStack* walk,
                                             int lane) {
    int count = 0;
    for (int base = 0; base < n; base += kFilerWave) {
        const int i = base + lane;
        const double v = i < n ? root_values[i] : 0.0;
        const bool keep = i < n && mz::outcomes::counts(v);
        const unsigned long long mask = __ballot(keep);
        if (keep) packed[count + __popcll(mask & ((1ull << lane) - 1ull))] = v;
        count += __popcll(mask);
    }
    __syncthreads();
    // leaf k of the tree goes to lane k % 64: leaf_of names it from its first value, no stack
    for (int off = 0, leaf_index = 0; off < count; ++leaf_index) {
        int leaf_off, leaf_len;
        mz::outcomes::leaf_of(count, off, &leaf_off, &leaf_len);
        if (leaf_index % kFilerWave == lane)
            packed[leaf_off] = mz::outcomes::pairwise_leaf([&](int i) { return packed[i]; }, leaf_off, leaf_len);
        off = leaf_off + leaf_len;
    }
    __syncthreads();
    double acc = 0.0;
    if (lane < 3) {
        // lane 0: every reward from i = 0; lanes 1 and 2: rewards[i], i >= 1, earned on the moves of player lane - 1
        for (int i = lane == 0 ? 0 : 1; i <= n; ++i) {
            const bool mine = lane == 0 || to_play[i - 1] == lane - 1;
            if (mine) acc = acc + rewards[i];
        }
    } else if (lane == 3 && count > 0) {
        acc = mz::outcomes::pairwise_walk(*walk, 0, count, [&](int off, int) { return packed[off]; });
    }
    if (lane == 0) out->total_reward = acc;
    if (lane == 1 || lane == 2) out->reward_of_player[lane - 1] = acc;
    if (lane == 3) {
        out->value_sum = acc;
        out->value_count = count;
        out->reserved = 0;
    }
}

// mzreplay_game_outcomes: a wavefront per stored game
__global__ __launch_bounds__(kFilerWave) void game_outcomes_kernel(StoreParams p, const int32_t* __restrict__ slots,
                                                                   double* __restrict__ packed,   // [n][L]
                                                                   mz::outcomes::Outcome* __restrict__ out) {
    __shared__ mz::outcomes::WalkStack walk;
    const int g = blockIdx.x, lane = threadIdx.x;
    const int slot = slots[g];
    const int n = p.length[slot];
    if (n < 1 || n > p.L) {   // an empty slot (block-uniform: before any barrier)
        if (lane == 0) out[g] = mz::outcomes::Outcome{0.0, {0.0, 0.0}, 0.0, 0, 0};
        return;
    }
    const size_t L = p.L;
    wave_outcome(p.rewards + slot * (L + 1), p.to_play + slot * (L + 1), p.root_values + slot * L, n, packed + g * L,
                 out + g, &walk, lane);
}

template <bool kVec4, bool kOutcomes>
__global__ __launch_bounds__(kFilerWave) void filer_append_kernel(StoreParams p, FilerParams f, mzreplay_file_moves mv) {
    extern __shared__ double policy_row[];   // [A] one move's child_visits row, scattered by action, written out in order
    const int e = blockIdx.x, lane = threadIdx.x;
    const mz::filer::Call call = *f.call;
    const int k = f.played[e];
    if (call.refused || k == 0) return;
    const int E = f.E, A = p.A, M = mv.n_moves, obs = p.obs_floats;
    const size_t L = p.L, L1 = L + 1;
    const double S = static_cast<double>(mv.num_simulations);
    float* row_obs = f.obs + static_cast<size_t>(e) * L1 * obs;
    int32_t* row_act = f.actions + static_cast<size_t>(e) * L1;
    double* row_rew = f.rewards + static_cast<size_t>(e) * L1;
    int8_t* row_tp = f.to_play + static_cast<size_t>(e) * L1;
    double* row_cv = f.child_visits + static_cast<size_t>(e) * L * A;
    double* row_rv = f.root_values + static_cast<size_t>(e) * L;
    int len = f.length[e];
    int rank = f.offset[e];   // of the env's next finished game within the call
    for (int m = 0; m < k; ++m) {
        const size_t me = static_cast<size_t>(m) * E + e;
        const int32_t* visits = move_block<int32_t>(mv.visits, mv.visits_stride, m) + static_cast<size_t>(e) * A;
        const int32_t* legal = move_block<int32_t>(mv.legal, mv.legal_stride, m) + static_cast<size_t>(e) * A;
        const int n_legal = move_block<int32_t>(mv.num_legal, mv.num_legal_stride, m)[e];   // (checked by filer_count_kernel)
        for (int a = lane; a < A; a += kFilerWave) policy_row[a] = 0.0;
        __syncthreads();
        for (int i = lane; i < n_legal; i += kFilerWave) policy_row[legal[i]] = static_cast<double>(visits[i]) / S;
        __syncthreads();
        double* cv = row_cv + static_cast<size_t>(len) * A;
        for (int a = lane; a < A; a += kFilerWave) cv[a] = policy_row[a];
        const int to_play = mv.to_play ? move_block<int32_t>(mv.to_play, mv.to_play_stride, m)[e] : 0;
        if (lane == 0) {
            row_rv[len] = move_block<double>(mv.root_value_sum, mv.root_value_sum_stride, m)[e] / S;
            row_act[len + 1] = move_block<int32_t>(mv.actions, mv.actions_stride, m)[e];
            row_rew[len + 1] = static_cast<double>(mv.rewards[me]);
            row_tp[len + 1] = static_cast<int8_t>(mv.players > 1 ? 1 - to_play : 0);
        }
        copy_floats<kVec4>(row_obs + static_cast<size_t>(len + 1) * obs, mv.obs_after + me * obs, obs, lane);
        ++len;
        if (mv.done[me]) {
            __syncthreads();   // the row is complete (and visible to every lane) before it is copied
            const int j = rank++;
            if constexpr (kOutcomes) {   // of every game the call finishes, dropped ones included: the row is whole here only
                __shared__ mz::outcomes::WalkStack walk;
                wave_outcome(row_rew, row_tp, row_rv, len, f.packed + static_cast<size_t>(e) * L, f.list_out + call.list_base + j,
                             &walk, lane);
            }
            if (mz::filer::survives(call, j)) {
                const size_t slot = static_cast<size_t>(mz::filer::slot_of(mz::filer::game_id(call, j), p.G));
                copy_floats<kVec4>(p.obs + slot * L1 * obs, row_obs, static_cast<size_t>(len + 1) * obs, lane);
                copy_items(p.actions + slot * L1, row_act, len + 1, lane);
                copy_items(p.rewards + slot * L1, row_rew, len + 1, lane);
                copy_items(p.to_play + slot * L1, row_tp, len + 1, lane);
                copy_items(p.child_visits + slot * L * A, row_cv, static_cast<size_t>(len) * A, lane);
                copy_items(p.root_values + slot * L, row_rv, len, lane);
                if (lane == 0) {
                    p.length[slot] = len;
                    p.has_reanalysed[slot] = 0;
                }
            }
            if (lane == 0) {
                f.list_env[call.list_base + j] = e;
                f.list_len[call.list_base + j] = len;
                f.list_id[call.list_base + j] = mz::filer::game_id(call, j);
                atomicAdd(reinterpret_cast<unsigned long long*>(&f.shared->steps_played), static_cast<unsigned long long>(len));
                if (mz::filer::survives(call, j))
                    atomicAdd(reinterpret_cast<unsigned long long*>(&f.shared->total_samples), static_cast<unsigned long long>(len));
            }
            __syncthreads();   // the copies have read the row before the next game starts in it
            len = 0;
            copy_floats<kVec4>(row_obs, mv.obs_next + me * obs, obs, lane);
            if (lane == 0) {
                row_act[0] = 0;
                row_rew[0] = 0.0;
                int next = 0;   // the next move's recorded player: the envs' own after the batch's last move
                if (mv.to_play) next = m + 1 < M ? move_block<int32_t>(mv.to_play, mv.to_play_stride, m + 1)[e] : mv.to_play_last[e];
                row_tp[0] = static_cast<int8_t>(next);
            }
        }
    }
    if (lane == 0) f.length[e] = len;
}

__global__ __launch_bounds__(256) void filer_priorities_kernel(StoreParams p, FilerParams f) {
    __shared__ float block_max[256];
    const mz::filer::Call call = *f.call;
    for (int j = call.dropped + blockIdx.x; j < call.n_new; j += gridDim.x) {
        const int64_t id = mz::filer::game_id(call, j);
        const int slot = mz::filer::slot_of(id, p.G);
        const int n = p.length[slot];
        float best = -INFINITY;
        for (int i = threadIdx.x; i < p.L; i += blockDim.x) {
            float pr = 0.f;
            if (i < n) {
                pr = position_priority(p, slot, n, i);
                best = fmaxf(best, pr);
            }
            f.priorities[static_cast<size_t>(slot) * p.L + i] = pr;
        }
        block_max[threadIdx.x] = best;
        __syncthreads();
        for (int s = blockDim.x / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) block_max[threadIdx.x] = fmaxf(block_max[threadIdx.x], block_max[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            f.game_priority[slot] = block_max[0];
            if (f.game_id) f.game_id[slot] = id;
        }
        __syncthreads();
    }
}

// every env starts a game (mzhist_begin)
__global__ __launch_bounds__(256) void filer_begin_kernel(StoreParams p, FilerParams f, const float* __restrict__ first_obs,
                                                          const int32_t* __restrict__ first_to_play) {
    const int e = blockIdx.x;
    const size_t L1 = static_cast<size_t>(p.L) + 1;
    for (int t = threadIdx.x; t < p.obs_floats; t += blockDim.x)
        f.obs[static_cast<size_t>(e) * L1 * p.obs_floats + t] = first_obs[static_cast<size_t>(e) * p.obs_floats + t];
    if (threadIdx.x == 0) {
        f.actions[e * L1] = 0;
        f.rewards[e * L1] = 0.0;
        f.to_play[e * L1] = static_cast<int8_t>(first_to_play ? first_to_play[e] : 0);
        f.length[e] = 0;
    }
}

__global__ __launch_bounds__(256) void gather_priorities_kernel(StoreParams p, FilerParams f, const int32_t* __restrict__ slots,
                                                                float* __restrict__ priorities,
                                                                float* __restrict__ game_priority) {
    const int g = blockIdx.x, slot = slots[g];
    for (int i = threadIdx.x; i < p.L; i += blockDim.x)
        priorities[static_cast<size_t>(g) * p.L + i] = f.priorities[static_cast<size_t>(slot) * p.L + i];
    if (threadIdx.x == 0) game_priority[g] = f.game_priority[slot];
}

}  // namespace

struct mzreplay {
    mzreplay_config cfg{};
    StoreParams p{};
    std::string error;
    std::vector<void*> allocs;
    int64_t bytes = 0;
    int32_t* d_slots = nullptr;      // staging for kernel arguments (capacity / batch sized, grown on demand)
    int32_t* d_positions = nullptr;
    int32_t* d_absorbing = nullptr;
    float* d_priorities = nullptr;
    float* d_game_priority = nullptr;
    size_t staging_games = 0, staging_batch = 0;
    int32_t* d_outcome_slots = nullptr;      // mzreplay_game_outcomes' staging (grown on demand)
    double* d_outcome_packed = nullptr;
    mz::outcomes::Outcome* d_outcomes = nullptr;
    size_t outcome_games = 0;
    bool sampler_on = false;
    SamplerParams sp{};
    int64_t next_game_id = 0;        // id of the next game mzreplay_add_games stores (sampler on)
    size_t sampler_batch = 0;        // samples the per-batch scratch holds
    std::vector<mzreplay_filer*> filers;         // the device filers bound to this store, one per filing actor
    mz::filer::Counters* filer_counters = nullptr;   // the store-wide counters every filer's kernels move (device)
    hipEvent_t last_filing = nullptr;            // recorded behind every mzreplay_filer_file: the next one waits for it
    float* filer_priorities = nullptr;           // [G][L], [G]: what the filers write while the sampler is off
    float* filer_game_priority = nullptr;
    bool reanalyse_on = false;       // mzreplay_reanalyse_enable: the pass's stream and scratch exist
    ReanalyseParams rp{};
    bool re_fc_ready = false;        // mzreplay_reanalyse_fc_configure
    mz::FcNet re_fc{};
    const float* re_fc_weights = nullptr;
    size_t re_fc_lds = 0;
    int re_fc_grid = 0;
};

struct mzreplay_filer {
    mzreplay* store = nullptr;
    FilerParams f{};
    std::vector<void*> allocs;
    int64_t pending_bound = 0;       // games the unsynced calls can have filed at most (E x M each)
    int32_t* d_gather_slots = nullptr;   // mzreplay_filer_priorities' staging
    float* d_gather = nullptr;
    size_t gather_games = 0;
    std::vector<int32_t> h_env, h_len;   // games drained from the device list since the last sync
    std::vector<int64_t> h_id;
    std::vector<int32_t> out_env, out_len;   // what the last mzreplay_filer_sync handed out
    std::vector<int64_t> out_id;
    bool begun = false;                  // mzreplay_filer_begin was called: the outcome switch no longer moves
    bool outcomes_on = false;            // mzreplay_filer_enable_outcomes
    std::vector<mz::outcomes::Outcome> h_outcome, out_outcome;   // parallel to h_* / out_* while the switch is on
};

static_assert(sizeof(mz::outcomes::Outcome) == 40 && sizeof(mzreplay_game_outcome) == 40,
              "mzreplay_game_outcome is mz::outcomes::Outcome: 40 bytes per game");

namespace {
std::string g_create_error;

int fail(mzreplay* s, const std::string& msg) {
    if (s) s->error = msg;
    g_create_error = msg;
    return -1;
}

#define RP_HIP(s, call)                                                                   \
    do {                                                                                  \
        hipError_t err__ = (call);                                                        \
        if (err__ != hipSuccess) return fail(s, std::string(#call) + ": " + hipGetErrorString(err__)); \
    } while (0)

template <typename T>
int dev_alloc(mzreplay* s, T** out, size_t count) {
    void* ptr = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    RP_HIP(s, hipMalloc(&ptr, bytes));
    RP_HIP(s, hipMemset(ptr, 0, bytes));
    s->allocs.push_back(ptr);
    s->bytes += static_cast<int64_t>(bytes);
    *out = static_cast<T*>(ptr);
    return 0;
}
}  // namespace

extern "C" {

const char* mzreplay_last_error(const mzreplay* s) { return s ? s->error.c_str() : g_create_error.c_str(); }

int mzreplay_create(const mzreplay_config* c, mzreplay** out) {
    if (!c || !out || !c->discount_powers) return fail(nullptr, "mzreplay_create: null argument");
    *out = nullptr;
    if (c->capacity <= 0 || c->max_moves <= 0 || c->num_actions <= 0 || c->obs_channels <= 0 || c->obs_height <= 0 ||
        c->obs_width <= 0 || c->stacked_observations < 0 || c->td_steps < 0 || c->num_unroll_steps < 0)
        return fail(nullptr, "mzreplay_create: sizes must be positive");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(nullptr, "mzreplay_create: no HIP device (the replay store has no CPU fallback)");
    mzreplay* s = new mzreplay();
    s->cfg = *c;
    if (hipSetDevice(c->device) != hipSuccess) {
        delete s;
        return fail(nullptr, "mzreplay_create: bad device");
    }
    StoreParams& p = s->p;
    p.G = c->capacity;
    p.L = c->max_moves;
    p.A = c->num_actions;
    p.C = c->obs_channels;
    p.H = c->obs_height;
    p.W = c->obs_width;
    p.obs_floats = p.C * p.H * p.W;
    p.stacked = c->stacked_observations;
    p.td_steps = c->td_steps;
    p.unroll = c->num_unroll_steps;
    p.alpha = c->per_alpha;
    const size_t G = p.G, L = p.L;
    double* d_pow = nullptr;
    int rc = 0;
    rc |= dev_alloc(s, &p.obs, G * (L + 1) * p.obs_floats);
    rc |= dev_alloc(s, &p.actions, G * (L + 1));
    rc |= dev_alloc(s, &p.rewards, G * (L + 1));
    rc |= dev_alloc(s, &p.to_play, G * (L + 1));
    rc |= dev_alloc(s, &p.child_visits, G * L * p.A);
    rc |= dev_alloc(s, &p.root_values, G * L);
    rc |= dev_alloc(s, &p.length, G);
    rc |= dev_alloc(s, &p.reanalysed, G * L);
    rc |= dev_alloc(s, &p.has_reanalysed, G);
    rc |= dev_alloc(s, &d_pow, static_cast<size_t>(p.td_steps) + 1);
    if (rc || hipMemcpy(d_pow, c->discount_powers, sizeof(double) * (p.td_steps + 1), hipMemcpyHostToDevice) != hipSuccess) {
        const std::string msg = s->error.empty() ? "mzreplay_create: device allocation failed" : s->error;
        mzreplay_destroy(s);
        return fail(nullptr, msg);
    }
    p.discount_pow = d_pow;
    s->cfg.discount_powers = nullptr;
    *out = s;
    return 0;
}

void mzreplay_destroy(mzreplay* s) {
    if (!s) return;
    while (!s->filers.empty()) mzreplay_filer_destroy(s->filers.back());
    if (s->last_filing) (void)hipEventDestroy(s->last_filing);
    for (void* ptr : s->allocs) (void)hipFree(ptr);
    delete s;
}

int64_t mzreplay_device_bytes(const mzreplay* s) { return s ? s->bytes : 0; }

int mzreplay_add_games(mzreplay* s, int32_t n, const int32_t* slots, const int32_t* lengths, const float* observations,
                       const int32_t* actions, const double* rewards, const int32_t* to_play, const double* child_visits,
                       const double* root_values, float* priorities, float* game_priority, void* stream_) {
    if (!s || !slots || !lengths || !observations || !actions || !rewards || !to_play || !child_visits || !root_values)
        return fail(s, "mzreplay_add_games: null argument");
    if (n <= 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const StoreParams& p = s->p;
    const size_t L = p.L, L1 = L + 1;
    for (int g = 0; g < n; ++g)
        if (slots[g] < 0 || slots[g] >= p.G || lengths[g] < 1 || lengths[g] > p.L)
            return fail(s, "mzreplay_add_games: slot or length out of range");
    if (static_cast<size_t>(n) > s->staging_games) {
        if (dev_alloc(s, &s->d_slots, static_cast<size_t>(n)) || dev_alloc(s, &s->d_priorities, static_cast<size_t>(n) * L) ||
            dev_alloc(s, &s->d_game_priority, static_cast<size_t>(n)))
            return -1;
        s->staging_games = static_cast<size_t>(n);
    }
    std::vector<int8_t> tp8(L1);
    for (int g = 0; g < n; ++g) {
        const size_t slot = static_cast<size_t>(slots[g]);
        const size_t len = static_cast<size_t>(lengths[g]);
        RP_HIP(s, hipMemcpyAsync(p.obs + slot * L1 * p.obs_floats, observations + static_cast<size_t>(g) * L1 * p.obs_floats,
                                 sizeof(float) * (len + 1) * p.obs_floats, hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipMemcpyAsync(p.actions + slot * L1, actions + static_cast<size_t>(g) * L1, sizeof(int32_t) * (len + 1),
                                 hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipMemcpyAsync(p.rewards + slot * L1, rewards + static_cast<size_t>(g) * L1, sizeof(double) * (len + 1),
                                 hipMemcpyHostToDevice, stream));
        for (size_t i = 0; i <= len; ++i) tp8[i] = static_cast<int8_t>(to_play[static_cast<size_t>(g) * L1 + i]);
        RP_HIP(s, hipMemcpyAsync(p.to_play + slot * L1, tp8.data(), len + 1, hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipStreamSynchronize(stream));  // tp8 is reused for the next game
        RP_HIP(s, hipMemcpyAsync(p.child_visits + slot * L * p.A, child_visits + static_cast<size_t>(g) * L * p.A,
                                 sizeof(double) * len * p.A, hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipMemcpyAsync(p.root_values + slot * L, root_values + static_cast<size_t>(g) * L, sizeof(double) * len,
                                 hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipMemcpyAsync(p.length + slot, lengths + g, sizeof(int32_t), hipMemcpyHostToDevice, stream));
        RP_HIP(s, hipMemsetAsync(p.has_reanalysed + slot, 0, 1, stream));
    }
    RP_HIP(s, hipMemcpyAsync(s->d_slots, slots, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
    priorities_kernel<<<dim3(n), dim3(256), 0, stream>>>(s->p, s->d_slots, s->d_priorities, s->d_game_priority);
    RP_HIP(s, hipGetLastError());
    if (s->sampler_on) {
        adopt_games_kernel<<<dim3(n), dim3(256), 0, stream>>>(s->p, s->sp, n, s->next_game_id, s->d_slots, s->d_priorities,
                                                             s->d_game_priority);
        RP_HIP(s, hipGetLastError());
        s->next_game_id += n;
    }
    if (priorities)
        RP_HIP(s, hipMemcpyAsync(priorities, s->d_priorities, sizeof(float) * n * L, hipMemcpyDeviceToHost, stream));
    if (game_priority)
        RP_HIP(s, hipMemcpyAsync(game_priority, s->d_game_priority, sizeof(float) * n, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_game_observations(mzreplay* s, int32_t slot, int32_t length, float* observations, void* stream_) {
    if (!s || !observations || slot < 0 || slot >= s->p.G || length < 1 || length > s->p.L)
        return fail(s, "mzreplay_game_observations: bad argument");
    game_observations_kernel<<<dim3(length), dim3(128), 0, static_cast<hipStream_t>(stream_)>>>(s->p, slot, observations);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_set_reanalysed(mzreplay* s, int32_t slot, const float* values, int32_t length, void* stream_) {
    if (!s || !values || slot < 0 || slot >= s->p.G || length < 1 || length > s->p.L)
        return fail(s, "mzreplay_set_reanalysed: bad argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    RP_HIP(s, hipMemcpyAsync(s->p.reanalysed + static_cast<size_t>(slot) * s->p.L, values, sizeof(float) * length,
                             hipMemcpyDefault, stream));
    RP_HIP(s, hipMemsetAsync(s->p.has_reanalysed + slot, 1, 1, stream));
    return 0;
}

int mzreplay_make_batch(mzreplay* s, int32_t batch, const int32_t* slots, const int32_t* positions,
                        const int32_t* absorbing_actions, float* observations, int64_t* actions, double* values,
                        double* rewards, double* policies, double* gradient_scale, void* stream_) {
    if (!s || !slots || !positions || !absorbing_actions || !observations || !actions || !values || !rewards || !policies ||
        !gradient_scale)
        return fail(s, "mzreplay_make_batch: null argument");
    if (batch <= 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const StoreParams& p = s->p;
    const size_t U1 = static_cast<size_t>(p.unroll) + 1;
    for (int b = 0; b < batch; ++b)
        if (slots[b] < 0 || slots[b] >= p.G || positions[b] < 0 || positions[b] > p.L)
            return fail(s, "mzreplay_make_batch: slot or position out of range");
    if (static_cast<size_t>(batch) > s->staging_batch) {
        int32_t* block = nullptr;
        if (dev_alloc(s, &block, static_cast<size_t>(batch) * (2 + U1))) return -1;
        s->d_positions = block;
        s->d_absorbing = block + 2 * static_cast<size_t>(batch);
        s->staging_batch = static_cast<size_t>(batch);
    }
    int32_t* d_slots = s->d_positions + batch;  // [positions B | slots B | absorbing B*(U+1)]
    RP_HIP(s, hipMemcpyAsync(s->d_positions, positions, sizeof(int32_t) * batch, hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipMemcpyAsync(d_slots, slots, sizeof(int32_t) * batch, hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipMemcpyAsync(s->d_absorbing, absorbing_actions, sizeof(int32_t) * batch * U1, hipMemcpyHostToDevice, stream));
    make_batch_kernel<double><<<dim3(batch), dim3(128), 0, stream>>>(s->p, d_slots, s->d_positions, s->d_absorbing, observations,
                                                            actions, values, rewards, policies, gradient_scale);
    RP_HIP(s, hipGetLastError());
    return 0;
}

// ---- the sampler's entries ---------------------------------------------------------------------------------------
namespace {
constexpr size_t kLdsBudget = 144 * 1024;   // of the 160 KB of a CU, beside the kernels' static arrays (11 KB)

int sampler_ready(mzreplay* s, const char* who) {
    if (!s) return fail(s, std::string(who) + ": null store");
    if (!s->sampler_on) return fail(s, std::string(who) + ": call mzreplay_sampler_enable first");
    return 0;
}

int grow_batch_scratch(mzreplay* s, size_t batch) {
    if (batch <= s->sampler_batch) return 0;
    SamplerParams& sp = s->sp;
    if (dev_alloc(s, &sp.game_len, batch) || dev_alloc(s, &sp.game_prob, batch) || dev_alloc(s, &sp.u_game, batch) ||
        dev_alloc(s, &sp.u_pos, batch) || dev_alloc(s, &sp.totals, batch) ||
        dev_alloc(s, &sp.tables, batch * static_cast<size_t>(s->p.L)))
        return -1;
    s->sampler_batch = batch;
    return 0;
}
}  // namespace

int mzreplay_sampler_enable(mzreplay* s, uint32_t seed, int64_t next_game_id) {
    if (!s) return fail(s, "mzreplay_sampler_enable: null store");
    if (next_game_id < 0) return fail(s, "mzreplay_sampler_enable: negative game id");
    if (!s->sampler_on) {
        SamplerParams& sp = s->sp;
        const size_t G = s->p.G, L = s->p.L;
        if (dev_alloc(s, &sp.priorities, G * L) || dev_alloc(s, &sp.game_priority, G) || dev_alloc(s, &sp.game_id, G) ||
            dev_alloc(s, &sp.mt_key, static_cast<size_t>(mz::kMtN)) || dev_alloc(s, &sp.mt_pos, 1) ||
            dev_alloc(s, &sp.probs, G) || dev_alloc(s, &sp.cdf, G))
            return -1;
        RP_HIP(s, hipMemset(sp.game_id, 0xff, sizeof(int64_t) * G));   // -1: empty slots
        sp.lds_games = G * (sizeof(double) + sizeof(float)) <= kLdsBudget ? 1 : 0;
        RP_HIP(s, hipFuncSetAttribute(reinterpret_cast<const void*>(sample_games_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBudget)));
        RP_HIP(s, hipFuncSetAttribute(reinterpret_cast<const void*>(position_tables_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBudget)));
        RP_HIP(s, hipFuncSetAttribute(reinterpret_cast<const void*>(sample_walk_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBudget)));
        s->sampler_on = true;
    }
    s->next_game_id = next_game_id;
    uint32_t key[mz::kMtN];
    int32_t pos;
    mz::mt_seed(key, &pos, seed);   // numpy.random.seed(seed)
    return mzreplay_sampler_set_rng(s, key, pos);
}

int mzreplay_sampler_set_rng(mzreplay* s, const uint32_t* key, int32_t pos) {
    if (sampler_ready(s, "mzreplay_sampler_set_rng")) return -1;
    if (!key || pos < 0 || pos > mz::kMtN) return fail(s, "mzreplay_sampler_set_rng: bad state");
    RP_HIP(s, hipDeviceSynchronize());
    RP_HIP(s, hipMemcpy(s->sp.mt_key, key, sizeof(uint32_t) * mz::kMtN, hipMemcpyHostToDevice));
    RP_HIP(s, hipMemcpy(s->sp.mt_pos, &pos, sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int mzreplay_sampler_get_rng(mzreplay* s, uint32_t* key, int32_t* pos) {
    if (sampler_ready(s, "mzreplay_sampler_get_rng")) return -1;
    if (!key || !pos) return fail(s, "mzreplay_sampler_get_rng: null argument");
    RP_HIP(s, hipDeviceSynchronize());
    RP_HIP(s, hipMemcpy(key, s->sp.mt_key, sizeof(uint32_t) * mz::kMtN, hipMemcpyDeviceToHost));
    RP_HIP(s, hipMemcpy(pos, s->sp.mt_pos, sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mzreplay_set_priorities(mzreplay* s, int32_t slot, int64_t game_id, const float* priorities, int32_t length,
                            void* stream_) {
    if (sampler_ready(s, "mzreplay_set_priorities")) return -1;
    if (!priorities || slot < 0 || slot >= s->p.G || length < 1 || length > s->p.L || game_id < 0)
        return fail(s, "mzreplay_set_priorities: bad argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    std::vector<float> row(static_cast<size_t>(s->p.L), 0.f);
    float top = priorities[0];
    for (int i = 0; i < length; ++i) {
        row[i] = priorities[i];
        top = mz::replay::numpy_max2(top, priorities[i]);
    }
    RP_HIP(s, hipMemcpyAsync(s->sp.priorities + static_cast<size_t>(slot) * s->p.L, row.data(), sizeof(float) * s->p.L,
                             hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipMemcpyAsync(s->sp.game_priority + slot, &top, sizeof(float), hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipMemcpyAsync(s->sp.game_id + slot, &game_id, sizeof(int64_t), hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_get_priorities(mzreplay* s, int32_t slot, float* priorities, float* game_priority, int64_t* game_id,
                            void* stream_) {
    if (sampler_ready(s, "mzreplay_get_priorities")) return -1;
    if (slot < 0 || slot >= s->p.G) return fail(s, "mzreplay_get_priorities: bad slot");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (priorities)
        RP_HIP(s, hipMemcpyAsync(priorities, s->sp.priorities + static_cast<size_t>(slot) * s->p.L, sizeof(float) * s->p.L,
                                 hipMemcpyDeviceToHost, stream));
    if (game_priority)
        RP_HIP(s, hipMemcpyAsync(game_priority, s->sp.game_priority + slot, sizeof(float), hipMemcpyDeviceToHost, stream));
    if (game_id) RP_HIP(s, hipMemcpyAsync(game_id, s->sp.game_id + slot, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_sample_batch(mzreplay* s, int32_t batch, int64_t oldest_game_id, int32_t n_games, int64_t total_samples,
                          int32_t per, int64_t* game_ids, int32_t* slots, int32_t* positions, int32_t* absorbing_actions,
                          float* weights, void* stream_) {
    if (sampler_ready(s, "mzreplay_sample_batch")) return -1;
    if (!game_ids || !slots || !positions || !absorbing_actions || (per && !weights))
        return fail(s, "mzreplay_sample_batch: null argument");
    const StoreParams& p = s->p;
    if (batch <= 0 || batch > 4096) return fail(s, "mzreplay_sample_batch: batch must be 1..4096");
    if (n_games < 1 || n_games > p.G || oldest_game_id < 0 || total_samples < 1)
        return fail(s, "mzreplay_sample_batch: no stored games, or more than the capacity");
    if (grow_batch_scratch(s, static_cast<size_t>(batch))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const SamplerParams& sp = s->sp;
    const size_t U1 = static_cast<size_t>(p.unroll) + 1;
    RP_HIP(s, hipMemsetAsync(absorbing_actions, 0, sizeof(int32_t) * batch * U1, stream));
    const size_t games_lds = sp.lds_games ? static_cast<size_t>(p.G) * (sizeof(double) + sizeof(float)) : 0;
    sample_games_kernel<<<dim3(1), dim3(kSampleThreads), games_lds, stream>>>(p, sp, batch, oldest_game_id, n_games,
                                                                             per ? 1 : 0, game_ids, slots);
    RP_HIP(s, hipGetLastError());
    const int tail = p.unroll < p.L ? p.unroll : p.L;
    int lds_tails = 0;
    if (per) {
        const int lds_rows = sizeof(double) * static_cast<size_t>(p.L) <= kLdsBudget ? 1 : 0;
        position_tables_kernel<<<dim3(batch), dim3(64), lds_rows ? sizeof(double) * p.L : 0, stream>>>(p, sp, lds_rows, slots);
        RP_HIP(s, hipGetLastError());
        lds_tails = sizeof(double) * static_cast<size_t>(batch) * tail + sizeof(int32_t) * batch <= kLdsBudget ? 1 : 0;
    }
    const size_t walk_lds = (lds_tails ? sizeof(double) * static_cast<size_t>(batch) * tail : 0) + sizeof(int32_t) * batch;
    sample_walk_kernel<<<dim3(1), dim3(64), walk_lds, stream>>>(p, sp, batch, per ? 1 : 0, tail, lds_tails, positions,
                                                               absorbing_actions);
    RP_HIP(s, hipGetLastError());
    if (per) {
        sample_finish_kernel<<<dim3(1), dim3(kSampleThreads), 0, stream>>>(p, sp, batch, total_samples, slots, positions,
                                                                          weights);
        RP_HIP(s, hipGetLastError());
    }
    return 0;
}

int mzreplay_make_batch_device(mzreplay* s, int32_t batch, const int32_t* slots, const int32_t* positions,
                               const int32_t* absorbing_actions, float* observations, int64_t* actions, float* values,
                               float* rewards, float* policies, float* gradient_scale, void* stream_) {
    if (!s || !slots || !positions || !absorbing_actions || !observations || !actions || !values || !rewards || !policies ||
        !gradient_scale)
        return fail(s, "mzreplay_make_batch_device: null argument");
    if (batch <= 0) return 0;
    make_batch_kernel<float><<<dim3(batch), dim3(128), 0, static_cast<hipStream_t>(stream_)>>>(
        s->p, slots, positions, absorbing_actions, observations, actions, values, rewards, policies, gradient_scale);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_update_priorities(mzreplay* s, int32_t batch, const int64_t* game_ids, const int32_t* positions,
                               const float* priorities, void* stream_) {
    if (sampler_ready(s, "mzreplay_update_priorities")) return -1;
    if (!game_ids || !positions || !priorities) return fail(s, "mzreplay_update_priorities: null argument");
    if (batch <= 0) return 0;
    if (batch > 4096) return fail(s, "mzreplay_update_priorities: batch must be 1..4096");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    update_priorities_kernel<<<dim3(batch), dim3(128), (sizeof(int64_t) + sizeof(int32_t)) * batch, stream>>>(
        s->p, s->sp, batch, game_ids, positions, priorities);
    RP_HIP(s, hipGetLastError());
    game_priority_kernel<<<dim3(batch), dim3(64), 0, stream>>>(s->p, s->sp, game_ids);
    RP_HIP(s, hipGetLastError());
    return 0;
}

// ---- reading games back, and the device filer's entries ----------------------------------------------------------------
int mzreplay_read_games(mzreplay* s, int32_t n, const int32_t* slots, int32_t* lengths, float* observations, int32_t* actions,
                        double* rewards, int32_t* to_play, double* child_visits, double* root_values, void* stream_) {
    if (!s || !slots) return fail(s, "mzreplay_read_games: null argument");
    if (n <= 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const StoreParams& p = s->p;
    const size_t L = p.L, L1 = L + 1, A = p.A, obs = p.obs_floats;
    for (int g = 0; g < n; ++g)
        if (slots[g] < 0 || slots[g] >= p.G) return fail(s, "mzreplay_read_games: slot out of range");
    std::vector<int32_t> all(static_cast<size_t>(p.G));
    RP_HIP(s, hipMemcpyAsync(all.data(), p.length, sizeof(int32_t) * p.G, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    std::vector<int8_t> tp8(to_play ? static_cast<size_t>(n) * L1 : 0);
    if (observations) std::memset(observations, 0, sizeof(float) * n * L1 * obs);
    if (actions) std::memset(actions, 0, sizeof(int32_t) * n * L1);
    if (rewards) std::memset(rewards, 0, sizeof(double) * n * L1);
    if (to_play) std::memset(to_play, 0, sizeof(int32_t) * n * L1);
    if (child_visits) std::memset(child_visits, 0, sizeof(double) * n * L * A);
    if (root_values) std::memset(root_values, 0, sizeof(double) * n * L);
    for (int g = 0; g < n; ++g) {
        const size_t slot = static_cast<size_t>(slots[g]), o = static_cast<size_t>(g);
        const int32_t stored = all[slot];
        if (stored < 0 || stored > p.L) return fail(s, "mzreplay_read_games: a stored length is out of range");
        const size_t len = static_cast<size_t>(stored);
        if (lengths) lengths[g] = stored;
        if (observations)
            RP_HIP(s, hipMemcpyAsync(observations + o * L1 * obs, p.obs + slot * L1 * obs, sizeof(float) * (len + 1) * obs,
                                     hipMemcpyDeviceToHost, stream));
        if (actions)
            RP_HIP(s, hipMemcpyAsync(actions + o * L1, p.actions + slot * L1, sizeof(int32_t) * (len + 1), hipMemcpyDeviceToHost, stream));
        if (rewards)
            RP_HIP(s, hipMemcpyAsync(rewards + o * L1, p.rewards + slot * L1, sizeof(double) * (len + 1), hipMemcpyDeviceToHost, stream));
        if (to_play) RP_HIP(s, hipMemcpyAsync(tp8.data() + o * L1, p.to_play + slot * L1, len + 1, hipMemcpyDeviceToHost, stream));
        if (child_visits && len)
            RP_HIP(s, hipMemcpyAsync(child_visits + o * L * A, p.child_visits + slot * L * A, sizeof(double) * len * A,
                                     hipMemcpyDeviceToHost, stream));
        if (root_values && len)
            RP_HIP(s, hipMemcpyAsync(root_values + o * L, p.root_values + slot * L, sizeof(double) * len, hipMemcpyDeviceToHost, stream));
    }
    RP_HIP(s, hipStreamSynchronize(stream));
    if (to_play)
        for (int g = 0; g < n; ++g)
            for (int32_t i = 0; i <= all[static_cast<size_t>(slots[g])]; ++i)
                to_play[static_cast<size_t>(g) * L1 + i] = tp8[static_cast<size_t>(g) * L1 + i];
    return 0;
}

}  // extern "C"

namespace {
template <typename T>
int filer_alloc(mzreplay_filer* fl, T** out, size_t count) {
    mzreplay* s = fl->store;
    void* ptr = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    RP_HIP(s, hipMalloc(&ptr, bytes));
    RP_HIP(s, hipMemset(ptr, 0, bytes));
    fl->allocs.push_back(ptr);
    s->bytes += static_cast<int64_t>(bytes);
    *out = static_cast<T*>(ptr);
    return 0;
}

// the games of the unsynced calls, moved from the device list to the host arrays mzreplay_filer_sync hands out
// (`stream` need not be the filer's own: it waits for the store's last filing, behind which every earlier one has run;
// the counters it reads are then those after every filing queued so far)
int filer_drain(mzreplay_filer* fl, FilerState* state_out, mz::filer::Counters* counters_out, hipStream_t stream) {
    mzreplay* s = fl->store;
    FilerState st{};
    mz::filer::Counters counters{};
    RP_HIP(s, hipStreamWaitEvent(stream, s->last_filing, 0));
    RP_HIP(s, hipMemcpyAsync(&st, fl->f.state, sizeof(st), hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipMemcpyAsync(&counters, fl->f.shared, sizeof(counters), hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    if (st.pending < 0 || st.pending > fl->f.list_cap) return fail(s, "mzreplay_filer_sync: the device list is corrupt");
    if (st.pending > 0) {
        const size_t have = fl->h_env.size(), more = static_cast<size_t>(st.pending);
        fl->h_env.resize(have + more);
        fl->h_len.resize(have + more);
        fl->h_id.resize(have + more);
        RP_HIP(s, hipMemcpyAsync(fl->h_env.data() + have, fl->f.list_env, sizeof(int32_t) * more, hipMemcpyDeviceToHost, stream));
        RP_HIP(s, hipMemcpyAsync(fl->h_len.data() + have, fl->f.list_len, sizeof(int32_t) * more, hipMemcpyDeviceToHost, stream));
        RP_HIP(s, hipMemcpyAsync(fl->h_id.data() + have, fl->f.list_id, sizeof(int64_t) * more, hipMemcpyDeviceToHost, stream));
        if (fl->outcomes_on) {
            fl->h_outcome.resize(have + more);
            RP_HIP(s, hipMemcpyAsync(fl->h_outcome.data() + have, fl->f.list_out, sizeof(mz::outcomes::Outcome) * more,
                                     hipMemcpyDeviceToHost, stream));
        }
    }
    // pending starts again at zero; the error word (adjacent) only for the sync, which reports it: a drain between two
    // unsynced calls leaves it standing, so the device goes on refusing and the next sync still sees it
    RP_HIP(s, hipMemsetAsync(&fl->f.state->pending, 0, (state_out ? 2 : 1) * sizeof(int32_t), stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    fl->pending_bound = 0;
    if (state_out) *state_out = st;
    if (counters_out) *counters_out = counters;
    return 0;
}
}  // namespace

extern "C" {

int mzreplay_filer_create(mzreplay* s, int32_t num_envs, mzreplay_filer** out) {
    if (!s || !out) return fail(s, "mzreplay_filer_create: null store or output");
    *out = nullptr;
    if (num_envs <= 0) return fail(s, "mzreplay_filer_create: num_envs must be positive");
    // (a store with stacked_observations > 0 is filed like any other: the rows hold the plain observations the env
    // kernels produced, and stacked_element stacks them when a batch is built; the actor's frame stack feeds the searches)
    RP_HIP(s, hipSetDevice(s->cfg.device));
    // what the store's filers share exists from the first of them on: the counters' block and the event that orders the calls
    if (!s->filer_counters && dev_alloc(s, &s->filer_counters, 1)) return -1;
    if (!s->last_filing) RP_HIP(s, hipEventCreateWithFlags(&s->last_filing, hipEventDisableTiming));
    mzreplay_filer* fl = new mzreplay_filer();
    fl->store = s;
    FilerParams& f = fl->f;
    const StoreParams& p = s->p;
    const size_t E = static_cast<size_t>(num_envs), L = p.L, L1 = L + 1;
    f.E = num_envs;
    int rc = 0;
    rc |= filer_alloc(fl, &f.obs, E * L1 * p.obs_floats);
    rc |= filer_alloc(fl, &f.actions, E * L1);
    rc |= filer_alloc(fl, &f.rewards, E * L1);
    rc |= filer_alloc(fl, &f.to_play, E * L1);
    rc |= filer_alloc(fl, &f.child_visits, E * L * p.A);
    rc |= filer_alloc(fl, &f.root_values, E * L);
    rc |= filer_alloc(fl, &f.length, E);
    rc |= filer_alloc(fl, &f.played, E);
    rc |= filer_alloc(fl, &f.count, E);
    rc |= filer_alloc(fl, &f.offset, E);
    rc |= filer_alloc(fl, &f.state, 1);
    rc |= filer_alloc(fl, &f.call, 1);
    if (rc) {
        const std::string msg = s->error;
        mzreplay_filer_destroy(fl);
        return fail(s, msg.empty() ? "mzreplay_filer_create: device allocation failed" : msg);
    }
    f.shared = s->filer_counters;
    s->filers.push_back(fl);
    *out = fl;
    return 0;
}

void mzreplay_filer_destroy(mzreplay_filer* fl) {
    if (!fl) return;
    (void)hipDeviceSynchronize();
    for (void* ptr : fl->allocs) (void)hipFree(ptr);
    if (fl->store) {
        std::vector<mzreplay_filer*>& all = fl->store->filers;
        all.erase(std::remove(all.begin(), all.end(), fl), all.end());
    }
    delete fl;
}

int mzreplay_filer_begin(mzreplay_filer* fl, const float* first_observations, const int32_t* first_to_play, void* stream_) {
    if (!fl || !first_observations) return fail(fl ? fl->store : nullptr, "mzreplay_filer_begin: null argument");
    mzreplay* s = fl->store;
    fl->begun = true;
    filer_begin_kernel<<<dim3(fl->f.E), dim3(256), 0, static_cast<hipStream_t>(stream_)>>>(s->p, fl->f, first_observations,
                                                                                          first_to_play);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_filer_set_counters(mzreplay_filer* fl, const int64_t* counters, void* stream_) {
    if (!fl || !counters) return fail(fl ? fl->store : nullptr, "mzreplay_filer_set_counters: null argument");
    mzreplay* s = fl->store;
    if (counters[0] < 0 || counters[1] < 0 || counters[1] > s->p.G || counters[1] > counters[0] || counters[2] < 0 || counters[3] < 0)
        return fail(s, "mzreplay_filer_set_counters: counters out of range");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    mz::filer::Counters c{counters[0], counters[1], counters[2], counters[3]};
    RP_HIP(s, hipStreamWaitEvent(stream, s->last_filing, 0));   // (behind the filings queued so far, on whichever stream)
    RP_HIP(s, hipMemcpyAsync(fl->f.shared, &c, sizeof(c), hipMemcpyHostToDevice, stream));
    RP_HIP(s, hipStreamSynchronize(stream));   // (c is a local)
    s->next_game_id = counters[0];
    return 0;
}

int mzreplay_filer_file(mzreplay_filer* fl, const mzreplay_file_moves* mv, void* stream_) {
    if (!fl || !mv) return fail(fl ? fl->store : nullptr, "mzreplay_filer_file: null argument");
    mzreplay* s = fl->store;
    if (!mv->actions || !mv->visits || !mv->root_value_sum || !mv->legal || !mv->num_legal || !mv->rewards || !mv->done ||
        !mv->obs_after || !mv->obs_next || (mv->to_play && !mv->to_play_last))
        return fail(s, "mzreplay_filer_file: null argument");
    const StoreParams& p = s->p;
    FilerParams& f = fl->f;
    if (mv->n_moves <= 0) return 0;
    if (mv->num_simulations <= 0 || mv->players < 1 || mv->players > 2)
        return fail(s, "mzreplay_filer_file: num_simulations must be positive and players 1 or 2");
    const int64_t most = static_cast<int64_t>(f.E) * mv->n_moves;   // games the batch can finish
    if (most > (int64_t{1} << 30)) return fail(s, "mzreplay_filer_file: the batch is too large");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (fl->pending_bound + most > f.list_cap) {
        // the list grows: what it holds goes to the host first (blocking, like any allocation; a warmed-up actor that
        // syncs after every batch does not come here again)
        if (filer_drain(fl, nullptr, nullptr, stream)) return -1;
        if (most > f.list_cap) {
            int32_t *env = nullptr, *len = nullptr;
            int64_t* id = nullptr;
            if (filer_alloc(fl, &env, static_cast<size_t>(most)) || filer_alloc(fl, &len, static_cast<size_t>(most)) ||
                filer_alloc(fl, &id, static_cast<size_t>(most)))
                return -1;
            f.list_env = env;
            f.list_len = len;
            f.list_id = id;
            if (fl->outcomes_on && filer_alloc(fl, &f.list_out, static_cast<size_t>(most))) return -1;
            f.list_cap = static_cast<int32_t>(most);
        }
    }
    if (fl->outcomes_on && (!f.list_out || !f.packed))   // (the switch moved after a filing that came before begin)
        return fail(s, "mzreplay_filer_file: the outcome list does not exist: mzreplay_filer_enable_outcomes comes before "
                       "mzreplay_filer_begin and before the first filing");
    if (s->sampler_on) {
        f.priorities = s->sp.priorities;
        f.game_priority = s->sp.game_priority;
        f.game_id = s->sp.game_id;
    } else {
        // (the store's, not the filer's: mzreplay_filer_priorities reads a slot whichever filer wrote it)
        if (!s->filer_priorities &&
            (dev_alloc(s, &s->filer_priorities, static_cast<size_t>(p.G) * p.L) || dev_alloc(s, &s->filer_game_priority, static_cast<size_t>(p.G))))
            return -1;
        f.priorities = s->filer_priorities;
        f.game_priority = s->filer_game_priority;
        f.game_id = nullptr;
    }
    fl->pending_bound += most;
    // the store numbers games in the order of these calls: this one's launches run behind the last launch of the call
    // made before it, on whichever stream that was queued
    RP_HIP(s, hipStreamWaitEvent(stream, s->last_filing, 0));
    filer_count_kernel<<<dim3((f.E + 255) / 256), dim3(256), 0, stream>>>(p, f, *mv);
    RP_HIP(s, hipGetLastError());
    filer_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, stream>>>(p, f);
    RP_HIP(s, hipGetLastError());
    auto aligned = [](const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; };
    const bool vec4 = p.obs_floats % 4 == 0 && aligned(mv->obs_after) && aligned(mv->obs_next);
    const size_t lds = sizeof(double) * p.A;
    if (fl->outcomes_on) {
        if (vec4)
            filer_append_kernel<true, true><<<dim3(f.E), dim3(kFilerWave), lds, stream>>>(p, f, *mv);
        else
            filer_append_kernel<false, true><<<dim3(f.E), dim3(kFilerWave), lds, stream>>>(p, f, *mv);
    } else if (vec4) {
        filer_append_kernel<true, false><<<dim3(f.E), dim3(kFilerWave), lds, stream>>>(p, f, *mv);
    } else {
        filer_append_kernel<false, false><<<dim3(f.E), dim3(kFilerWave), lds, stream>>>(p, f, *mv);
    }
    RP_HIP(s, hipGetLastError());
    const int64_t grid = std::min<int64_t>(std::min<int64_t>(most, p.G), 2048);
    filer_priorities_kernel<<<dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream>>>(p, f);
    RP_HIP(s, hipGetLastError());
    RP_HIP(s, hipEventRecord(s->last_filing, stream));
    return 0;
}

int mzreplay_filer_sync_ids(mzreplay_filer* fl, int32_t* n_new, const int32_t** env_index, const int32_t** lengths,
                            const int64_t** game_ids, int64_t* counters, void* stream_) {
    if (!fl || !n_new) return fail(fl ? fl->store : nullptr, "mzreplay_filer_sync: null argument");
    mzreplay* s = fl->store;
    FilerState st{};
    mz::filer::Counters now{};
    if (filer_drain(fl, &st, &now, static_cast<hipStream_t>(stream_))) return -1;
    s->next_game_id = now.next_game_id;
    if (counters) {
        counters[0] = now.next_game_id;
        counters[1] = now.games_stored;
        counters[2] = now.total_samples;
        counters[3] = now.steps_played;
    }
    if (st.error) {
        // (the batch that raised it filed nothing; games of earlier, unsynced batches stay for the next sync)
        *n_new = 0;
        if (st.error & mz::filer::kErrLegal)
            return fail(s, "mzhist_file: a legal-action count outside [0, A] or a legal action outside [0, A)");
        if (st.error & mz::filer::kErrOverflow) return fail(s, "mzhist_file: a game outgrew max_moves");
        return fail(s, "mzreplay_filer_file: the list of filed games was full");
    }
    fl->out_env.swap(fl->h_env);
    fl->out_len.swap(fl->h_len);
    fl->out_id.swap(fl->h_id);
    fl->out_outcome.swap(fl->h_outcome);
    fl->h_env.clear();
    fl->h_len.clear();
    fl->h_id.clear();
    fl->h_outcome.clear();
    *n_new = static_cast<int32_t>(fl->out_env.size());
    if (env_index) *env_index = fl->out_env.data();
    if (lengths) *lengths = fl->out_len.data();
    if (game_ids) *game_ids = fl->out_id.data();
    return 0;
}

int mzreplay_filer_sync(mzreplay_filer* fl, int32_t* n_new, const int32_t** env_index, const int32_t** lengths,
                        int64_t* first_game_id, int64_t* counters, void* stream_) {
    if (!fl || !n_new) return fail(fl ? fl->store : nullptr, "mzreplay_filer_sync: null argument");
    mzreplay* s = fl->store;
    if (s->filers.size() > 1)
        return fail(s, "mzreplay_filer_sync: the store has more than one filer, whose games are not consecutive: use "
                       "mzreplay_filer_sync_ids");
    int64_t now[4] = {0, 0, 0, 0};
    const int rc = mzreplay_filer_sync_ids(fl, n_new, env_index, lengths, nullptr, now, stream_);
    if (counters) std::memcpy(counters, now, sizeof(now));
    if (rc) return rc;
    if (first_game_id) *first_game_id = now[0] - static_cast<int64_t>(*n_new);
    return 0;
}

int mzreplay_filer_lengths(mzreplay_filer* fl, int32_t* lengths, void* stream_) {
    if (!fl || !lengths) return fail(fl ? fl->store : nullptr, "mzreplay_filer_lengths: null argument");
    mzreplay* s = fl->store;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    RP_HIP(s, hipMemcpyAsync(lengths, fl->f.length, sizeof(int32_t) * fl->f.E, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_outcomes_reference(int32_t n, const double* rewards, const int8_t* to_play, const double* root_values,
                                mzreplay_game_outcome* out) {
    if (!rewards || !to_play || !root_values || !out) return fail(nullptr, "mzreplay_outcomes_reference: null argument");
    if (n < 1) return fail(nullptr, "mzreplay_outcomes_reference: a game has at least one move");
    std::vector<double> packed(static_cast<size_t>(n));
    const mz::outcomes::Outcome o = mz::outcomes::game_outcome(rewards, to_play, root_values, n, packed.data());
    std::memcpy(out, &o, sizeof(o));
    return 0;
}

int mzreplay_game_outcomes(mzreplay* s, int32_t n, const int32_t* slots, mzreplay_game_outcome* outcomes, void* stream_) {
    if (n < 0) return fail(s, "mzreplay_game_outcomes: n must not be negative");   // (before the pointers: no device needed)
    if (!s || !slots || !outcomes) return fail(s, "mzreplay_game_outcomes: null argument");
    const StoreParams& p = s->p;
    for (int g = 0; g < n; ++g)
        if (slots[g] < 0 || slots[g] >= p.G) return fail(s, "mzreplay_game_outcomes: slot out of range");
    if (n == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t count = static_cast<size_t>(n);
    if (count > s->outcome_games) {
        if (dev_alloc(s, &s->d_outcome_slots, count) || dev_alloc(s, &s->d_outcome_packed, count * p.L) ||
            dev_alloc(s, &s->d_outcomes, count))
            return -1;
        s->outcome_games = count;
    }
    if (s->last_filing) RP_HIP(s, hipStreamWaitEvent(stream, s->last_filing, 0));   // (behind the filings queued so far)
    RP_HIP(s, hipMemcpyAsync(s->d_outcome_slots, slots, sizeof(int32_t) * count, hipMemcpyHostToDevice, stream));
    game_outcomes_kernel<<<dim3(n), dim3(kFilerWave), 0, stream>>>(p, s->d_outcome_slots, s->d_outcome_packed, s->d_outcomes);
    RP_HIP(s, hipGetLastError());
    RP_HIP(s, hipMemcpyAsync(outcomes, s->d_outcomes, sizeof(mz::outcomes::Outcome) * count, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_filer_enable_outcomes(mzreplay_filer* fl, int32_t on) {
    if (!fl) return fail(nullptr, "mzreplay_filer_enable_outcomes: null filer");
    mzreplay* s = fl->store;
    if (fl->begun) return fail(s, "mzreplay_filer_enable_outcomes: the switch is set before mzreplay_filer_begin");
    if (on && !fl->f.packed && filer_alloc(fl, &fl->f.packed, static_cast<size_t>(fl->f.E) * s->p.L)) return -1;
    fl->outcomes_on = on != 0;
    return 0;
}

int mzreplay_filer_sync_outcomes(mzreplay_filer* fl, int32_t* n, const mzreplay_game_outcome** outcomes) {
    if (!fl || !n || !outcomes) return fail(fl ? fl->store : nullptr, "mzreplay_filer_sync_outcomes: null argument");
    if (!fl->outcomes_on)
        return fail(fl->store, "mzreplay_filer_sync_outcomes: the filer reports no outcomes: call "
                               "mzreplay_filer_enable_outcomes(filer, 1) before mzreplay_filer_begin");
    *n = static_cast<int32_t>(fl->out_outcome.size());
    *outcomes = reinterpret_cast<const mzreplay_game_outcome*>(fl->out_outcome.data());
    return 0;
}

int mzreplay_filer_priorities(mzreplay_filer* fl, int32_t n, const int32_t* slots, float* priorities, float* game_priority,
                              void* stream_) {
    if (!fl || !slots || !priorities || !game_priority) return fail(fl ? fl->store : nullptr, "mzreplay_filer_priorities: null argument");
    mzreplay* s = fl->store;
    if (n <= 0) return 0;
    // (the arrays the store's filers write, whichever of them filed: this one may not have filed yet)
    FilerParams from = fl->f;
    from.priorities = s->sampler_on ? s->sp.priorities : s->filer_priorities;
    from.game_priority = s->sampler_on ? s->sp.game_priority : s->filer_game_priority;
    if (!from.priorities) return fail(s, "mzreplay_filer_priorities: nothing has been filed yet");
    const StoreParams& p = s->p;
    for (int g = 0; g < n; ++g)
        if (slots[g] < 0 || slots[g] >= p.G) return fail(s, "mzreplay_filer_priorities: slot out of range");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t L = p.L, count = static_cast<size_t>(n);
    if (count > fl->gather_games) {
        if (filer_alloc(fl, &fl->d_gather_slots, count) || filer_alloc(fl, &fl->d_gather, count * (L + 1))) return -1;
        fl->gather_games = count;
    }
    float* d_pri = fl->d_gather;
    float* d_game = fl->d_gather + count * L;
    RP_HIP(s, hipMemcpyAsync(fl->d_gather_slots, slots, sizeof(int32_t) * count, hipMemcpyHostToDevice, stream));
    gather_priorities_kernel<<<dim3(n), dim3(256), 0, stream>>>(p, from, fl->d_gather_slots, d_pri, d_game);
    RP_HIP(s, hipGetLastError());
    RP_HIP(s, hipMemcpyAsync(priorities, d_pri, sizeof(float) * count * L, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipMemcpyAsync(game_priority, d_game, sizeof(float) * count, hipMemcpyDeviceToHost, stream));
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"

// ---- Reanalyse in batches ---------------------------------------------------------------------------------------------
namespace {
constexpr size_t kLdsPerWorkgroup = 160 * 1024;   // gfx950

int reanalyse_ready(mzreplay* s, const char* who) {
    if (!s) return fail(s, std::string(who) + ": null store");
    if (!s->reanalyse_on) return fail(s, std::string(who) + ": call mzreplay_reanalyse_enable first");
    return 0;
}

int plan_arguments(mzreplay* s, const char* who, int32_t n_games, const int32_t* slots, const int32_t* row_start) {
    if (!s) return fail(s, std::string(who) + ": null store");
    if (!slots || !row_start) return fail(s, std::string(who) + ": null argument");
    if (n_games < 1 || n_games > mz::reanalyse::kMaxGames) return fail(s, std::string(who) + ": n_games must be 1..4096");
    return 0;
}

int phase_entries(const mz::FcPhase* list, int n, int G) {
    int total = 0;
    for (int i = 0; i < n; ++i) total += (list[i].total_out + 4 * G - 1) / (4 * G) * 4 * G;
    return total;
}

// dynamic LDS of reanalyse_fc_kernel
size_t reanalyse_fc_lds_bytes(const mz::FcNet& net) {
    const int entries = phase_entries(net.init_pre, net.n_init_pre, kReanalyseGroup) +
                        phase_entries(net.init_post, net.n_init_post, kReanalyseGroup);
    return sizeof(float) * (static_cast<size_t>((net.n_weights_lds + 3) & ~3) +
                            static_cast<size_t>(net.scratch_floats) * kReanalyseRowsPerBlock) +
           sizeof(mz::NeuronDesc) * static_cast<size_t>(entries);
}
}  // namespace

extern "C" {

int32_t mzreplay_reanalyse_fc_group_width(void) { return kReanalyseGroup; }

int mzreplay_reanalyse_enable(mzreplay* s, uint32_t seed) {
    if (!s) return fail(s, "mzreplay_reanalyse_enable: null store");
    if (!mz::reanalyse::rows_fit(mz::reanalyse::kMaxGames, s->p.L))
        return fail(s, "mzreplay_reanalyse_enable: 4096 games of max_moves rows do not fit int32");
    if (!s->reanalyse_on) {
        ReanalyseParams& rp = s->rp;
        if (dev_alloc(s, &rp.mt_key, static_cast<size_t>(mz::kMtN)) || dev_alloc(s, &rp.mt_pos, 1) ||
            dev_alloc(s, &rp.last_draw, static_cast<size_t>(s->p.G)) ||
            dev_alloc(s, &rp.given_ids, static_cast<size_t>(mz::reanalyse::kMaxGames)))
            return -1;
        s->reanalyse_on = true;
    }
    uint32_t key[mz::kMtN];
    int32_t pos;
    mz::mt_seed(key, &pos, seed);   // numpy.random.seed(seed)
    return mzreplay_reanalyse_set_rng(s, key, pos);
}

int mzreplay_reanalyse_set_rng(mzreplay* s, const uint32_t* key, int32_t pos) {
    if (reanalyse_ready(s, "mzreplay_reanalyse_set_rng")) return -1;
    if (!key || pos < 0 || pos > mz::kMtN) return fail(s, "mzreplay_reanalyse_set_rng: bad state");
    RP_HIP(s, hipDeviceSynchronize());
    RP_HIP(s, hipMemcpy(s->rp.mt_key, key, sizeof(uint32_t) * mz::kMtN, hipMemcpyHostToDevice));
    RP_HIP(s, hipMemcpy(s->rp.mt_pos, &pos, sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int mzreplay_reanalyse_get_rng(mzreplay* s, uint32_t* key, int32_t* pos) {
    if (reanalyse_ready(s, "mzreplay_reanalyse_get_rng")) return -1;
    if (!key || !pos) return fail(s, "mzreplay_reanalyse_get_rng: null argument");
    RP_HIP(s, hipDeviceSynchronize());
    RP_HIP(s, hipMemcpy(key, s->rp.mt_key, sizeof(uint32_t) * mz::kMtN, hipMemcpyDeviceToHost));
    RP_HIP(s, hipMemcpy(pos, s->rp.mt_pos, sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

int mzreplay_reanalyse_plan(mzreplay* s, int32_t n_games, int64_t oldest_game_id, int32_t n_stored, const int64_t* given_ids,
                            int64_t* game_ids, int32_t* slots, int32_t* row_start, void* stream_) {
    if (reanalyse_ready(s, "mzreplay_reanalyse_plan")) return -1;
    if (!game_ids) return fail(s, "mzreplay_reanalyse_plan: null argument");
    if (plan_arguments(s, "mzreplay_reanalyse_plan", n_games, slots, row_start)) return -1;
    const StoreParams& p = s->p;
    if (n_stored < 0 || n_stored > p.G || oldest_game_id < 0)
        return fail(s, "mzreplay_reanalyse_plan: more stored games than the capacity, or a negative id");
    if (!mz::reanalyse::rows_fit(n_games, p.L)) return fail(s, "mzreplay_reanalyse_plan: n_games * max_moves does not fit int32");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (given_ids && n_stored > 0) {
        for (int d = 0; d < n_games; ++d)
            if (given_ids[d] < oldest_game_id || given_ids[d] >= oldest_game_id + n_stored)
                return fail(s, "mzreplay_reanalyse_plan: game " + std::to_string(given_ids[d]) + " is not stored");
        RP_HIP(s, hipMemcpyAsync(s->rp.given_ids, given_ids, sizeof(int64_t) * n_games, hipMemcpyHostToDevice, stream));
    }
    reanalyse_plan_kernel<<<dim3(1), dim3(kPlanThreads), 0, stream>>>(p, s->rp, n_games, oldest_game_id, n_stored,
                                                                     given_ids ? 1 : 0, game_ids, slots, row_start);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_reanalyse_observations(mzreplay* s, int32_t n_games, const int32_t* slots, const int32_t* row_start,
                                    int32_t n_rows, float* observations, void* stream_) {
    if (plan_arguments(s, "mzreplay_reanalyse_observations", n_games, slots, row_start)) return -1;
    if (n_rows < 0 || (n_rows > 0 && !observations)) return fail(s, "mzreplay_reanalyse_observations: bad argument");
    if (n_rows == 0) return 0;
    const int grid = n_rows < 65536 ? n_rows : 65536;
    reanalyse_observations_kernel<<<dim3(grid), dim3(128), 0, static_cast<hipStream_t>(stream_)>>>(s->p, n_games, slots, row_start,
                                                                                              n_rows, observations);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_reanalyse_store(mzreplay* s, int32_t n_games, const int32_t* slots, const int32_t* row_start, const float* values,
                             void* stream_) {
    if (plan_arguments(s, "mzreplay_reanalyse_store", n_games, slots, row_start)) return -1;
    if (!values) return fail(s, "mzreplay_reanalyse_store: null argument");
    reanalyse_store_kernel<<<dim3(n_games), dim3(128), 0, static_cast<hipStream_t>(stream_)>>>(s->p, n_games, slots, row_start,
                                                                                          values);
    RP_HIP(s, hipGetLastError());
    return 0;
}

int mzreplay_read_reanalysed(mzreplay* s, int32_t n, const int32_t* slots, float* values, uint8_t* has_values, void* stream_) {
    if (!s || !slots) return fail(s, "mzreplay_read_reanalysed: null argument");
    if (n <= 0) return 0;
    const StoreParams& p = s->p;
    for (int g = 0; g < n; ++g)
        if (slots[g] < 0 || slots[g] >= p.G) return fail(s, "mzreplay_read_reanalysed: slot out of range");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t L = p.L;
    for (int g = 0; g < n; ++g) {
        if (values)
            RP_HIP(s, hipMemcpyAsync(values + static_cast<size_t>(g) * L, p.reanalysed + static_cast<size_t>(slots[g]) * L,
                                     sizeof(float) * L, hipMemcpyDeviceToHost, stream));
        if (has_values) RP_HIP(s, hipMemcpyAsync(has_values + g, p.has_reanalysed + slots[g], 1, hipMemcpyDeviceToHost, stream));
    }
    RP_HIP(s, hipStreamSynchronize(stream));
    return 0;
}

int mzreplay_reanalyse_fc_configure(mzreplay* s, const mzmcts_fc_desc* desc, int32_t support_size, const float* weights,
                                    int64_t n_weights) {
    if (!s || !desc || !weights) return fail(s, "mzreplay_reanalyse_fc_configure: null argument");
    const StoreParams& p = s->p;
    s->re_fc_ready = false;
    if (support_size < 1 || 2 * static_cast<int64_t>(support_size) + 1 > mz::kFcMaxWidth)
        return fail(s, std::string("mzreplay_reanalyse_fc_configure: ") + mz::kFcNetSizesMessage);
    const int64_t stacked_floats = static_cast<int64_t>(p.C + p.stacked * (p.C + 1)) * p.H * p.W;
    if (stacked_floats > mz::kFcMaxWidth)
        return fail(s, std::string("mzreplay_reanalyse_fc_configure: ") + mz::kFcNetSizesMessage);
    if (desc->observation_floats != stacked_floats)
        return fail(s, "mzreplay_reanalyse_fc_configure: observation_floats is not the store's stacked observation");
    mz::FcNet net{};
    const int rc = mz::build_fc_net(desc, p.A, support_size, n_weights, &net);
    if (rc == mz::kFcNetSizes) return fail(s, std::string("mzreplay_reanalyse_fc_configure: ") + mz::kFcNetSizesMessage);
    if (rc == mz::kFcNetWeightCount)
        return fail(s, std::string("mzreplay_reanalyse_fc_configure: ") + mz::kFcNetWeightCountMessage);
    const size_t lds = reanalyse_fc_lds_bytes(net);
    if (lds > kLdsPerWorkgroup)
        return fail(s, "mzreplay_reanalyse_fc_configure: the network's weights and activations do not fit a workgroup's "
                       "160 KB of LDS");
    int cus = 0;
    RP_HIP(s, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->cfg.device));
    RP_HIP(s, hipFuncSetAttribute(reinterpret_cast<const void*>(reanalyse_fc_kernel<kReanalyseGroup>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsPerWorkgroup)));
    const size_t per_cu = kLdsPerWorkgroup / (lds ? lds : 1);
    s->re_fc = net;
    s->re_fc_weights = weights;
    s->re_fc_lds = lds;
    s->re_fc_grid = (cus > 0 ? cus : 1) * static_cast<int>(per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu));
    s->re_fc_ready = true;
    return 0;
}

int mzreplay_reanalyse_fc(mzreplay* s, int32_t n_games, const int32_t* slots, const int32_t* row_start, void* stream_) {
    if (plan_arguments(s, "mzreplay_reanalyse_fc", n_games, slots, row_start)) return -1;
    if (!s->re_fc_ready) return fail(s, "mzreplay_reanalyse_fc: call mzreplay_reanalyse_fc_configure first");
    reanalyse_fc_kernel<kReanalyseGroup><<<dim3(s->re_fc_grid), dim3(kReanalyseThreads), s->re_fc_lds,
                                           static_cast<hipStream_t>(stream_)>>>(s->p, s->re_fc, s->re_fc_weights, n_games, slots,
                                                                                row_start);
    RP_HIP(s, hipGetLastError());
    return 0;
}

}  // extern "C"
