// game_outcomes.h -- what a finished game reports to the training loop's log (reference self_play.py:65-90): episode
// length aside, its total reward, the reward earned on each player's moves, and the sum and count of its non-zero root
// values, from which the host takes numpy.mean.  One source for the device (game_outcomes_kernel and filer_append_kernel
// of mzreplay.hip) and for plain g++ (tests/game_outcomes_check.cpp holds this text to the library's host entry).
//
// The input is a game of n >= 1 moves in the store's row layout: rewards f64[n + 1], to_play i8[n + 1], root_values f64[n].
//   total_reward         +0.0, then + rewards[i] for i = 0 .. n ascending: Python's sum(game_history.reward_history)
//   reward_of_player[p]  +0.0, then + rewards[i] for i = 1 .. n ascending where to_play[i - 1] == p: the reference's
//                        muzero_reward expression with muzero_player = p.  (Its i = 0 term indexes to_play_history[-1];
//                        the term carries rewards[0], which is 0.0 in every game, so leaving it out changes no sum.)
//   value_count          the number of i < n with root_values[i] != 0: `if value` is true for a NaN and false for both zeros
//   value_sum            numpy's pairwise fp64 sum over those values, in order; mean = value_sum / value_count on the host
//                        is numpy.mean([v for v in root_values if v]) bit for bit
// numpy's pairwise sum of c contiguous doubles: fewer than 8 are added left to right; up to 128 run eight sums over strides
// of 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remaining c % 8 values one by one; more than 128 split at
// c / 2 rounded down to a multiple of 8 and the halves are added.  (replay_sampler.h walks the same tree in float32.)
// The library is built with -ffp-contract=off; nothing here can contract anyway: there is no product.
#pragma once
#include <stdint.h>

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {
namespace outcomes {

constexpr int kPairwiseBlock = 128;   // numpy's PW_BLOCKSIZE

// one game's report: mzreplay_game_outcome of include/mzreplay.h, 40 bytes
struct Outcome {
    double total_reward;
    double reward_of_player[2];
    double value_sum;
    int32_t value_count;
    int32_t reserved;
};

// `if value`: a NaN counts, +0.0 and -0.0 do not
MZ_HD inline bool counts(double v) { return v != 0.0; }

template <typename RewardAt>
MZ_HD inline double total_reward(RewardAt reward_at, int n) {
    double total = 0.0;
    for (int i = 0; i <= n; ++i) total = total + reward_at(i);
    return total;
}

template <typename RewardAt, typename ToPlayAt>
MZ_HD inline double reward_of_player(RewardAt reward_at, ToPlayAt to_play_at, int n, int player) {
    double total = 0.0;
    for (int i = 1; i <= n; ++i)
        if (to_play_at(i - 1) == player) total = total + reward_at(i);
    return total;
}

// a leaf of the tree: c <= 128 values from `off`
template <typename At>
MZ_HD inline double pairwise_leaf(At a, int off, int c) {
    if (c < 8) {
        double res = 0.0;
        for (int i = 0; i < c; ++i) res = res + a(off + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a(off + j);
    int i = 8;
    for (; i < c - (c % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a(off + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < c; ++i) res = res + a(off + i);
    return res;
}

// The tree above the leaves is fixed by c alone.  The leaf that holds value `index` (0 <= index < c), found by walking
// down from the root: no stack, so every lane of a wavefront can name its own leaves.
MZ_HD inline void leaf_of(int c, int index, int* leaf_off, int* leaf_len) {
    int base = 0;
    while (c > kPairwiseBlock) {
        int half = c / 2;
        half -= half % 8;
        if (index < base + half) {
            c = half;
        } else {
            base += half;
            c -= half;
        }
    }
    *leaf_off = base;
    *leaf_len = c;
}

// The walk's explicit stack (32 levels cover every int32 length): the caller says where it lives -- a local on the host,
// LDS on the device, where keeping four indexed arrays in registers would cost the kernel its occupancy.
struct WalkStack {
    int off_of[32], c_of[32], stage[32];
    double left[32];
};

// `leaf(off, len)` is called once per leaf, left to right; the walk adds the halves as numpy's recursion does.
template <typename Leaf>
MZ_HD inline double pairwise_walk(WalkStack& st, int base, int c, Leaf leaf) {
    int sp = 1;
    st.off_of[0] = base;
    st.c_of[0] = c;
    st.stage[0] = 0;
    double ret = 0.0;
    while (sp > 0) {
        const int top = sp - 1;
        if (st.c_of[top] <= kPairwiseBlock) {
            ret = leaf(st.off_of[top], st.c_of[top]);
            --sp;
        } else if (st.stage[top] == 0) {
            int half = st.c_of[top] / 2;
            half -= half % 8;
            st.stage[top] = 1;
            st.off_of[sp] = st.off_of[top];
            st.c_of[sp] = half;
            st.stage[sp] = 0;
            ++sp;
            continue;
        }
        while (sp > 0) {   // hand `ret` to the waiting parents
            const int parent = sp - 1;
            int half = st.c_of[parent] / 2;
            half -= half % 8;
            if (st.stage[parent] == 1) {
                st.left[parent] = ret;
                st.stage[parent] = 2;
                st.off_of[sp] = st.off_of[parent] + half;
                st.c_of[sp] = st.c_of[parent] - half;
                st.stage[sp] = 0;
                ++sp;
                break;
            }
            ret = st.left[parent] + ret;
            --sp;
        }
    }
    return ret;
}

template <typename At>
MZ_HD inline double pairwise_sum(WalkStack& st, At a, int c) {
    return pairwise_walk(st, 0, c, [&](int off, int len) { return pairwise_leaf(a, off, len); });
}

// pairwise_sum the way a wavefront computes it (wave_outcome of mzreplay.hip), on one thread: every leaf, named by leaf_of
// from its first value, leaves its sum in its first cell, then the walk adds those cells up.  Overwrites `packed`.
inline double pairwise_sum_by_leaves(WalkStack& st, double* packed, int c) {
    for (int off = 0; off < c;) {
        int leaf_off, leaf_len;
        leaf_of(c, off, &leaf_off, &leaf_len);
        packed[leaf_off] = pairwise_leaf([&](int i) { return packed[i]; }, leaf_off, leaf_len);
        off = leaf_off + leaf_len;
    }
    return c > 0 ? pairwise_walk(st, 0, c, [&](int off, int) { return packed[off]; }) : 0.0;
}

// the counted root values, in order, into packed[0 .. count): returns count.  `packed` has room for n doubles.
template <typename ValueAt>
MZ_HD inline int compact_values(ValueAt value_at, int n, double* packed) {
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const double v = value_at(i);
        if (counts(v)) packed[count++] = v;
    }
    return count;
}

// the whole rule on one thread: what the kernels compute (`packed`: scratch of n doubles)
inline Outcome game_outcome(const double* rewards, const int8_t* to_play, const double* root_values, int n, double* packed) {
    Outcome out;
    auto reward_at = [&](int i) { return rewards[i]; };
    auto to_play_at = [&](int i) { return static_cast<int>(to_play[i]); };
    out.total_reward = total_reward(reward_at, n);
    out.reward_of_player[0] = reward_of_player(reward_at, to_play_at, n, 0);
    out.reward_of_player[1] = reward_of_player(reward_at, to_play_at, n, 1);
    out.value_count = compact_values([&](int i) { return root_values[i]; }, n, packed);
    // (the leaves as leaf_of names them are the leaves the walk visits: the device relies on it)
    WalkStack stack;
    out.value_sum = pairwise_sum(stack, [&](int i) { return packed[i]; }, out.value_count);
    out.reserved = 0;
    return out;
}

}  // namespace outcomes
}  // namespace mz
