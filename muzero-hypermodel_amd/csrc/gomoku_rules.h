// gomoku_rules.h -- the rules of Gomoku (reference games/gomoku.py:219-289) as __host__ __device__ functions, included
// by board_rules.h.  The environment kernels (env_kernels.hip) and a CPU check (tests/gomoku_rules_check.cpp) compile
// this same text.
//
// Board int8[121], cell = 11 * row + column, 0 empty, +1 first player, -1 second; an action is a cell.  A game is
// finished when ANY stone of EITHER colour starts five equal stones in one of the directions (row, column) +=
// (1,-1), (1,0), (1,1), (0,1) without leaving the board, or when no cell is empty: the reference scans the whole board
// after every ply, so six in a row finishes (it contains a five) and a five already on the board finishes the next ply
// whoever moves.  The ply that finishes a game earns 1 (a full-board draw included), every other ply 0.
//
// The line scan runs on a PADDED copy of the board: row stride 15 (11 cells, then 4 zero bytes), 15 rows (11, then 4
// zero rows).  A five-step walk in one of the four directions moves at most 4 rows down and 4 columns left or right:
// a step past the right edge lands in the row's own padding, a step past the left edge in the padding of the row
// above, a step past the bottom in the zero rows -- every walk that leaves the board reads a 0, which equals no stone,
// so the scan needs no bounds test and a run cannot continue from column 10 into column 0 of the next row.
#pragma once
#include <cstdint>

#include "np_legacy_rng.h"  // MZ_HD

namespace mz {

constexpr int kGmkSize = 11;
constexpr int kGmkCells = kGmkSize * kGmkSize;  // 121 = the action count
constexpr int kGmkStride = kGmkSize + 4;        // padded row
constexpr int kGmkPadded = kGmkStride * kGmkStride;  // 225 bytes

MZ_HD inline int gmk_padded_index(int cell) { return (cell / kGmkSize) * kGmkStride + cell % kGmkSize; }

// Does the stone at padded index i (if there is one) start five equal stones in one of the four directions?
MZ_HD inline bool gmk_five_from(const int8_t* padded, int i) {
    const int p = padded[i];
    if (p == 0) return false;
    // (1,-1), (1,0), (1,1), (0,1) as padded-index steps
    const int steps[4] = {kGmkStride - 1, kGmkStride, kGmkStride + 1, 1};
    for (int d = 0; d < 4; ++d) {
        const int s = steps[d];
        if (padded[i + s] == p && padded[i + 2 * s] == p && padded[i + 3 * s] == p && padded[i + 4 * s] == p) return true;
    }
    return false;
}

MZ_HD inline void gmk_pad(const int8_t* b, int8_t* padded) {
    for (int i = 0; i < kGmkPadded; ++i) padded[i] = 0;
    for (int i = 0; i < kGmkCells; ++i) padded[gmk_padded_index(i)] = b[i];
}

// Gomoku.legal_actions(): the empty cells in ascending cell order
MZ_HD inline int gmk_legal(const int8_t* b, int32_t* legal) {
    int n = 0;
    for (int i = 0; i < kGmkCells; ++i)
        if (b[i] == 0) legal[n++] = i;
    return n;
}

// Gomoku.is_finished() in one thread (the wavefront kernels spread the same scan over the lanes of a group)
MZ_HD inline bool gmk_finished(const int8_t* b) {
    int8_t padded[kGmkPadded];
    gmk_pad(b, padded);
    bool empty = false;
    for (int i = 0; i < kGmkCells; ++i) {
        if (b[i] == 0) empty = true;
        else if (gmk_five_from(padded, gmk_padded_index(i))) return true;
    }
    return !empty;
}

}  // namespace mz
