// replay_sampler.h -- the arithmetic of ReplayBuffer.get_batch's sampling (reference replay_buffer.py:69-195) and of
// update_priorities (:197-220), draw for draw and bit for bit.  One source for the device (the sampler kernels of
// mzreplay.hip) and for plain g++ (tests/replay_sampler_check.cpp holds this text to numpy and to fixtures G12).
//
// One batch consumes numpy's legacy stream in this order:
//   1. B game draws.  PER: game_probs = f32(game_priority) / numpy.sum(game_probs) -- numpy's PAIRWISE float32 sum, in
//      pieces of 8192 -- then
//      choice(p=game_probs): the fp64 running sum of the probabilities, left to right, divided by its last entry, one
//      legacy double (two words) per draw, right bisection.  Uniform: B masked-rejection draws below the game count.
//   2. per sample, in batch order: one position draw (PER: Python's left-to-right float32 sum of the game's priorities,
//      float32 quotients, fp64 running sum, one legacy double; uniform: one bounded draw below the length), then one
//      bounded draw below the action count for every unrolled step past the end of the game (make_target).
//   3. weight = 1 / (total_samples * game_prob * pos_prob) in float32 step by step, divided by the batch maximum.
// Every sum below runs in the order named; the library is built with -ffp-contract=off and float32 division is the
// correctly rounded one.
#pragma once
#include "np_legacy_rng.h"

namespace mz {
namespace replay {

constexpr int kPairwiseBlock = 128;   // numpy's PW_BLOCKSIZE

// numpy's pairwise sum of n <= 128 contiguous float32 values: a plain loop below 8, else eight accumulators over the
// multiple-of-8 prefix, combined as a tree, then the remainder added one by one.
template <typename At>
MZ_HD inline float pairwise_leaf(At a, int off, int n) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res = res + a(off + i);
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a(off + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a(off + i + j);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a(off + i);
    return res;
}

// The tree above the leaves is fixed by n alone: a range longer than 128 splits at n / 2 rounded down to a multiple of 8.
// `leaf(off, len)` is called once per leaf, left to right; the walk adds the halves as the recursion would.
// (An explicit stack: 32 levels cover every int32 length.)
template <typename Leaf>
MZ_HD inline float pairwise_walk(int base, int n, Leaf leaf) {
    int off_of[32], n_of[32], stage[32];
    float left[32];
    int sp = 0;
    off_of[0] = base;
    n_of[0] = n;
    stage[0] = 0;
    sp = 1;
    float ret = 0.f;
    while (sp > 0) {
        const int top = sp - 1;
        if (n_of[top] <= kPairwiseBlock) {
            ret = leaf(off_of[top], n_of[top]);
            --sp;
        } else if (stage[top] == 0) {
            int n2 = n_of[top] / 2;
            n2 -= n2 % 8;
            stage[top] = 1;
            off_of[sp] = off_of[top];
            n_of[sp] = n2;
            stage[sp] = 0;
            ++sp;
            continue;
        }
        // hand `ret` to the waiting parents
        while (sp > 0) {
            const int parent = sp - 1;
            int n2 = n_of[parent] / 2;
            n2 -= n2 % 8;
            if (stage[parent] == 1) {
                left[parent] = ret;
                stage[parent] = 2;
                off_of[sp] = off_of[parent] + n2;
                n_of[sp] = n_of[parent] - n2;
                stage[sp] = 0;
                ++sp;
                break;
            }
            ret = left[parent] + ret;
            --sp;
        }
    }
    return ret;
}

// numpy.sum over a contiguous float32 array: the reduction starts from the identity and hands the data to the inner
// loop in pieces of numpy's buffer size (8192 elements, numpy.getbufsize()), adding each piece's pairwise sum in turn.
// `leaf(off, len)` as above: the leaves of all pieces, left to right.
constexpr int kNumpyBufferSize = 8192;
template <typename Leaf>
MZ_HD inline float numpy_sum_walk(int n, Leaf leaf) {
    float res = 0.f;
    for (int off = 0; off < n; off += kNumpyBufferSize)
        res = res + pairwise_walk(off, n - off < kNumpyBufferSize ? n - off : kNumpyBufferSize, leaf);
    return res;
}
template <typename At>
MZ_HD inline float numpy_sum_f32(At a, int n) {
    return numpy_sum_walk(n, [&](int off, int len) { return pairwise_leaf(a, off, len); });
}

// legacy_double from its two words
MZ_HD inline double uniform_from_words(uint32_t first, uint32_t second) {
    const int32_t a = static_cast<int32_t>(first >> 5);
    const int32_t b = static_cast<int32_t>(second >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

// cdf.searchsorted(u, side="right") over a non-decreasing table: the number of entries <= u
template <typename At>
MZ_HD inline int bisect_right(At cdf, int n, double u) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cdf(mid) <= u)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// sum(game_history.priorities): Python's sum over numpy float32 scalars, left to right (from int 0: exact)
template <typename At>
MZ_HD inline float python_sum_f32(At a, int n) {
    float total = 0.f;
    for (int i = 0; i < n; ++i) total = total + a(i);
    return total;
}

// 1 / (total_samples * game_prob * pos_prob): a Python int times numpy float32 scalars stays float32 at every step
MZ_HD inline float importance_weight(int64_t total_samples, float game_prob, float pos_prob) {
    const float t = static_cast<float>(total_samples) * game_prob;
    return 1.f / (t * pos_prob);
}

// make_target draws for the unrolled steps u with position + u > length: how many of the U + 1 steps those are
MZ_HD inline int absorbing_steps(int position, int length, int unroll) {
    const int c = position + unroll - length;
    return c > 0 ? (c < unroll + 1 ? c : unroll + 1) : 0;
}

// numpy.max as a fold: a NaN stays
MZ_HD inline float numpy_max2(float a, float b) { return (a > b || a != a) ? a : b; }

// update_priorities: sample b writes priorities[b][k] to position positions[b] + k of its game for k < length - position;
// entries are applied in batch order, so the write survives unless a later sample of the same game covers the position.
template <typename GameOf, typename PosOf>
MZ_HD inline bool update_survives(int b, int k, int batch, int steps, GameOf game_of, PosOf pos_of, int length_of_game) {
    const int64_t game = game_of(b);
    const int target = pos_of(b) + k;
    for (int later = b + 1; later < batch; ++later) {
        if (game_of(later) != game) continue;
        const int p = pos_of(later);
        int end = p + steps;
        if (end > length_of_game) end = length_of_game;
        if (target >= p && target < end) return false;
    }
    return true;
}

// ---- the whole batch on one thread: what the kernels compute, in the reference's order (host checks) -------------
struct BatchView {
    int n_games;                 // stored games, ring order oldest to newest
    const float* game_priority;  // [n_games]
    const int32_t* length;       // [n_games]
    const float* priorities;     // [n_games][stride]
    int stride;
    int unroll, num_actions;
    int64_t total_samples;
};

// outputs: game_index i32[B], position i32[B], absorbing i32[B][U+1] (zero where not drawn), weight f32[B] (PER)
inline void sample_batch_serial(const BatchView& v, bool per, int batch, uint32_t* key, int32_t* pos, uint64_t* words,
                                int32_t* game_index, int32_t* position, int32_t* absorbing, float* weight, float* probs,
                                double* cdf) {
    const int U1 = v.unroll + 1;
    uint32_t used = 0;
    if (per) {
        const float total = numpy_sum_f32([&](int i) { return v.game_priority[i]; }, v.n_games);
        for (int i = 0; i < v.n_games; ++i) probs[i] = v.game_priority[i] / total;
        double run = 0.0;
        for (int i = 0; i < v.n_games; ++i) {
            run += static_cast<double>(probs[i]);
            cdf[i] = run;
        }
        const double last = cdf[v.n_games - 1];
        for (int i = 0; i < v.n_games; ++i) cdf[i] = cdf[i] / last;
        for (int b = 0; b < batch; ++b) {
            const uint32_t w0 = mt_next(key, pos), w1 = mt_next(key, pos);
            used += 2;
            game_index[b] = bisect_right([&](int i) { return cdf[i]; }, v.n_games, uniform_from_words(w0, w1));
        }
    } else {
        for (int b = 0; b < batch; ++b) game_index[b] = static_cast<int32_t>(mt_below(key, pos, v.n_games, &used));
    }
    for (int b = 0; b < batch; ++b) {
        const int g = game_index[b], n = v.length[g];
        const float* pri = v.priorities + static_cast<size_t>(g) * v.stride;
        if (per) {
            const float total = python_sum_f32([&](int i) { return pri[i]; }, n);
            double run = 0.0;
            for (int i = 0; i < n; ++i) {
                run += static_cast<double>(pri[i] / total);
                cdf[i] = run;
            }
            const double last = cdf[n - 1];
            for (int i = 0; i < n; ++i) cdf[i] = cdf[i] / last;
            const uint32_t w0 = mt_next(key, pos), w1 = mt_next(key, pos);
            used += 2;
            position[b] = bisect_right([&](int i) { return cdf[i]; }, n, uniform_from_words(w0, w1));
            weight[b] = importance_weight(v.total_samples, probs[g], pri[position[b] < n ? position[b] : n - 1] / total);
        } else {
            position[b] = static_cast<int32_t>(mt_below(key, pos, n, &used));
        }
        for (int u = 0; u < U1; ++u) {
            absorbing[b * U1 + u] = 0;
            if (position[b] + u > n) absorbing[b * U1 + u] = static_cast<int32_t>(mt_below(key, pos, v.num_actions, &used));
        }
    }
    if (per) {
        float top = weight[0];
        for (int b = 1; b < batch; ++b) top = weight[b] > top ? weight[b] : top;   // Python's max()
        for (int b = 0; b < batch; ++b) weight[b] = weight[b] / top;
    }
    *words += used;
}

// update_priorities on host arrays, through update_survives (what the kernel evaluates per entry)
inline void update_priorities_serial(int batch, int steps, const int64_t* game_ids, const int32_t* positions,
                                     const float* new_priorities, int64_t oldest_id, int n_games, const int32_t* length,
                                     float* priorities, int stride, float* game_priority) {
    for (int b = 0; b < batch; ++b) {
        const int64_t g = game_ids[b] - oldest_id;
        if (g < 0 || g >= n_games) continue;   // removed since its selection
        const int n = length[g];
        for (int k = 0; k < steps && positions[b] + k < n; ++k)
            if (update_survives(b, k, batch, steps, [&](int i) { return game_ids[i]; }, [&](int i) { return positions[i]; }, n))
                priorities[static_cast<size_t>(g) * stride + positions[b] + k] = new_priorities[b * steps + k];
    }
    for (int b = 0; b < batch; ++b) {
        const int64_t g = game_ids[b] - oldest_id;
        if (g < 0 || g >= n_games) continue;
        float top = priorities[static_cast<size_t>(g) * stride];
        for (int i = 1; i < length[g]; ++i) top = numpy_max2(top, priorities[static_cast<size_t>(g) * stride + i]);
        game_priority[g] = top;
    }
}

}  // namespace replay
}  // namespace mz
