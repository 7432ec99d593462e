// reanalyse_plan.h -- the plan of a batched Reanalyse pass (reference replay_buffer.py:297-361, N games per pass instead of
// one).  One source for the device (reanalyse_plan_kernel and its consumers in mzreplay.hip) and for plain g++
// (tests/reanalyse_plan_check.cpp holds this text to numpy).
//
// A pass over n_games draws out of n_stored stored games whose ids start at oldest_game_id (slot = id % capacity):
//   1. draw d = numpy.random.choice(n_stored) (replay_buffer.py:151, force_uniform=True): one masked-rejection draw below
//      n_stored from the pass's own legacy MT19937 stream, in order d = 0 .. n_games - 1; n_stored == 1 consumes no word.
//      game_id[d] = oldest_game_id + index.  Ids handed in by the caller replace the draws; the stream does not move.
//   2. the weights do not change inside a pass, so a game is evaluated once: a draw whose game is drawn again LATER in the
//      pass gets no rows, the last occurrence carries them.
//   3. rows[d] = the game's length in moves for a carrying draw, 0 otherwise; row_start = their exclusive prefix sum,
//      int32[n_games + 1]; row_start[n_games] = R, the rows of the pass.  Row r belongs to the draw found by right bisection
//      in row_start, at position r - row_start[d].
#pragma once
#include "np_legacy_rng.h"

namespace mz {
namespace reanalyse {

constexpr int kMaxGames = 4096;   // draws per pass (the limit mzreplay_sample_batch has for a batch)

// R <= n_games * max_moves has to fit row_start's int32
MZ_HD inline bool rows_fit(int64_t n_games, int64_t max_moves) { return n_games * max_moves <= 2147483647ll; }

// one draw of step 1 on caller-provided MT19937 storage
MZ_HD inline int32_t draw_index(uint32_t* key, int32_t* pos, uint32_t n_stored) {
    uint32_t words = 0;
    return static_cast<int32_t>(mt_below(key, pos, n_stored, &words));
}

MZ_HD inline int32_t slot_of(int64_t game_id, int32_t capacity) { return static_cast<int32_t>(game_id % capacity); }

// step 2: no later draw of the pass names the same game
template <typename IdAt>
MZ_HD inline bool carries(int d, int n_games, IdAt id) {
    const int64_t own = id(d);
    for (int later = d + 1; later < n_games; ++later)
        if (id(later) == own) return false;
    return true;
}

// step 3, serially: row_start[0 .. n_games] from rows(d)
template <typename RowsAt>
MZ_HD inline void prefix_rows(int n_games, RowsAt rows, int32_t* row_start) {
    int32_t run = 0;
    for (int d = 0; d < n_games; ++d) {
        row_start[d] = run;
        run += rows(d);
    }
    row_start[n_games] = run;
}

// the draw that owns row r (0 <= r < row_start[n_games]): the last d with row_start[d] <= r.  Draws without rows share
// their start with the next draw, so right bisection never lands on them.
template <typename StartAt>
MZ_HD inline int draw_of_row(StartAt row_start, int n_games, int32_t r) {
    int lo = 0, hi = n_games + 1;   // first index whose start is > r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row_start(mid) <= r)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

// The whole plan on one thread: the statement the kernel is held to.  given_ids == nullptr: drawn.  Returns R.
inline int32_t plan_serial(uint32_t* key, int32_t* pos, int n_games, int64_t oldest_game_id, int32_t n_stored,
                           int32_t capacity, const int64_t* given_ids, const int32_t* length_of_slot, int64_t* game_ids,
                           int32_t* slots, int32_t* row_start) {
    if (n_stored <= 0) {
        for (int d = 0; d < n_games; ++d) {
            game_ids[d] = -1;
            slots[d] = -1;
        }
        for (int d = 0; d <= n_games; ++d) row_start[d] = 0;
        return 0;
    }
    for (int d = 0; d < n_games; ++d) {
        game_ids[d] = given_ids ? given_ids[d] : oldest_game_id + draw_index(key, pos, static_cast<uint32_t>(n_stored));
        slots[d] = slot_of(game_ids[d], capacity);
    }
    prefix_rows(n_games, [&](int d) { return carries(d, n_games, [&](int i) { return game_ids[i]; }) ? length_of_slot[slots[d]] : 0; },
                row_start);
    return row_start[n_games];
}

}  // namespace reanalyse
}  // namespace mz
