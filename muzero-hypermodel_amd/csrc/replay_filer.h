// replay_filer.h -- the index arithmetic of filing finished self-play games into the replay store on the device
// (include/mzreplay.h mzreplay_filer_file): which moves of a batch an env played, how many games it finished, where each
// finished game goes and what the store-wide counters become.  One source for the device (the filer kernels of
// mzreplay.hip) and for plain g++ (tests/replay_filer_check.cpp holds this text to HistoryFiler and to
// ReplayBuffer._add, the host path it must equal).
//
// One call files a batch of M moves of E envs:
//   prefix     an env's played moves are a prefix of the batch: they end at its first move whose action reads < 0
//              (mzmcts_moves_collect derives moves_done the same way; the env kernels leave such an env alone)
//   count      games the env finished among those moves (done flags), the running game's length carried over
//   order      finished games are numbered env-major, then in move order within an env (mzhist_finished's order):
//              game j of the call = exclusive scan of the counts over E + its rank within the env
//   ids        id = next id + j, slot = id % capacity (ReplayBuffer._add)
//   wrap       a call that finishes more games than the ring has slots writes only the last `capacity` of them, so that
//              no two games of a call share a slot; the counters move as if all had been stored and evicted in turn
//   counters   next id += n; stored = min(stored + n, capacity); steps += every new game's length;
//              total_samples += every new game's length - the length of every game evicted on the way (old ones that
//              lose their slot, new ones overwritten within the call) = the survivors' lengths - the evicted old ones'
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
namespace filer {

// bits of the device error word (mzreplay_filer_sync turns them into mzhist_file's messages)
constexpr int32_t kErrLegal = 1;      // a legal-action count outside [0, A] or a legal action outside [0, A)
constexpr int32_t kErrOverflow = 2;   // a game outgrew max_moves
constexpr int32_t kErrList = 4;       // the list of filed games had no room for the call (the host sizes it: a defect)

// the store-wide counters, in device memory (ReplayBuffer.num_played_games, len(buffer), total_samples, num_played_steps)
struct Counters {
    int64_t next_game_id;
    int64_t games_stored;
    int64_t total_samples;
    int64_t steps_played;
};

// what one call publishes for its later launches
struct Call {
    int64_t first_id;      // id of the call's game 0
    int32_t n_new;         // games the call finished (0 when the call was refused)
    int32_t dropped;       // the first `dropped` of them are not written: later games of the call take their slots
    int32_t list_base;     // where the call's games start in the list mzreplay_filer_sync hands out
    int32_t refused;       // the error word was set: nothing of the batch is filed
};

// rule 2: moves 0..k-1 were played, k = the first move whose action reads < 0 (M if none)
template <typename ActionAt>
MZ_HD inline int prefix_length(int n_moves, ActionAt action_at) {
    int k = 0;
    while (k < n_moves && action_at(k) >= 0) ++k;
    return k;
}

// games finished among the env's first k moves, starting from a running game of `length` moves; *overflow is set when a
// game would hold more than max_moves moves.  `length` leaves as the running game's length after the batch.
template <typename DoneAt>
MZ_HD inline int count_finished(int* length, int k, int max_moves, DoneAt done_at, bool* overflow) {
    int len = *length, count = 0;
    for (int m = 0; m < k; ++m) {
        ++len;
        if (len > max_moves) *overflow = true;
        if (done_at(m)) {
            ++count;
            len = 0;
        }
    }
    *length = len;
    return count;
}

MZ_HD inline Call plan_call(const Counters& c, int64_t n_new, int64_t capacity, int32_t list_base, bool refused) {
    Call call;
    call.first_id = c.next_game_id;
    call.n_new = refused ? 0 : static_cast<int32_t>(n_new);
    call.dropped = call.n_new > capacity ? static_cast<int32_t>(call.n_new - capacity) : 0;
    call.list_base = list_base;
    call.refused = refused ? 1 : 0;
    return call;
}

MZ_HD inline int64_t game_id(const Call& call, int j) { return call.first_id + j; }
MZ_HD inline int32_t slot_of(int64_t id, int64_t capacity) { return static_cast<int32_t>(id % capacity); }
// rule 4: does game j of the call reach the store?  (the last `capacity` games of a call do)
MZ_HD inline bool survives(const Call& call, int j) { return j >= call.dropped; }

// stored games that lose their slot to the call: the oldest `evicted_old` of them, ids first_evicted_id ...
MZ_HD inline int64_t evicted_old(const Counters& c, int64_t n_new, int64_t capacity) {
    const int64_t over = c.games_stored + n_new - capacity;
    return over <= 0 ? 0 : (over < c.games_stored ? over : c.games_stored);
}
MZ_HD inline int64_t first_evicted_id(const Counters& c) { return c.next_game_id - c.games_stored; }

// the counters after a call of n_new games: `all_lengths` = the sum of every new game's length, `survivor_lengths` = of
// those that reach the store, `evicted_lengths` = of the stored games evicted_old() names
MZ_HD inline Counters counters_after(const Counters& c, int64_t n_new, int64_t capacity, int64_t all_lengths,
                                     int64_t survivor_lengths, int64_t evicted_lengths) {
    Counters out;
    out.next_game_id = c.next_game_id + n_new;
    out.games_stored = c.games_stored + n_new < capacity ? c.games_stored + n_new : capacity;
    out.total_samples = c.total_samples + survivor_lengths - evicted_lengths;
    out.steps_played = c.steps_played + all_lengths;
    return out;
}

// Exclusive scan of E counts in chunks of `chunk` (the device scans a chunk in LDS and carries the running total to the
// next one); returns the total.  The serial statement of what the scan kernel computes.
template <typename CountAt, typename Put>
MZ_HD inline int64_t exclusive_scan_chunked(int n, int chunk, CountAt count_at, Put put) {
    int64_t carry = 0;
    for (int base = 0; base < n; base += chunk) {
        int64_t run = carry;
        const int end = base + chunk < n ? base + chunk : n;
        for (int i = base; i < end; ++i) {
            put(i, run);
            run += count_at(i);
        }
        carry = run;
    }
    return carry;
}

}  // namespace filer
}  // namespace mz
