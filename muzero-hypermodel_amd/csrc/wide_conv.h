// wide_conv.h -- geometry, packed-weight index rule and range rule of the 128-channel 3 x 3 convolution on 11 x 11 boards
// (wide_conv_split_kernel, csrc/wide_conv.hip: Gomoku's residual layers on the 16-bit matrix path, every operand as two
// fp16 halves).  Host and device compile this text: the kernel and its launcher count with it, launch_plan.h sizes the
// launch with it, tests/wide_conv_check.cpp walks it with g++.  No HIP include.
//
// The padded plane: a board row is followed by ONE zero column (the right border of row y is the left border of row
// y + 1), with a zero row above and below and one more cell so that the last row's lower-right neighbour exists:
//     position of board cell (y, x) = (y + 1) * 12 + x + 1,        157 positions, 13 .. 143 hold the board.
// A workgroup owns one board; its 121 output rows fill 8 row tiles of 16, the last 7 rows are padding: they read a cell
// that is always zero (column 0 of a padded row, neighbours inside the plane) and are never stored.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {

constexpr int kWideH = 11, kWideW = 11;
constexpr int kWideP = kWideH * kWideW;                    // 121 board positions
constexpr int kWidePW = kWideW + 1;                        // 12: row stride of the padded plane
constexpr int kWidePP = (kWideH + 2) * kWidePW + 1;        // 157 = padded_plane(11, 11)
constexpr int kWideCout = 128;
constexpr int kWideMaxCin = 160;                           // 5 groups of 32: the dynamics input's 129 planes fit
constexpr int kWideGroup = 32;                             // input channels per MFMA (K of v_mfma_f32_16x16x32_f16)
constexpr int kWideWaves = 8;                              // 4 column pairs x 2 row groups
constexpr int kWideThreads = 64 * kWideWaves;
constexpr int kWideRowTiles = 8;                           // ceil(121 / 16)
constexpr int kWideZeroPos = 2 * kWidePW;                  // column 0 of padded row 2: zero, all nine neighbours exist
constexpr int kWideStageLdm = 124;                         // floats between two channels of the output staging tile
                                                           // (4 x 124 = 48 mod 64 banks: the four channel quads of a
                                                           //  wavefront's store fall into four different 16-bank runs)
constexpr float kWideActScale = 8.f, kWideWtScale = 64.f;  // powers of two: removed exactly in the epilogue
constexpr float kWideHalfMax = 65504.f;                    // largest finite fp16

MZ_HD inline int wide_groups(int cin) { return (cin + kWideGroup - 1) / kWideGroup; }
MZ_HD inline int wide_cph(int cin) { return wide_groups(cin) * kWideGroup + 8; }   // halves per (position, half); +8: bank spread

// board position p = y * 11 + x -> its cell in the padded plane
MZ_HD inline int wide_plane_pos(int p) { return (p / kWideW + 1) * kWidePW + (p % kWideW) + 1; }
// output row m of the 8 row tiles (0 .. 127) -> the padded position its A operand is read around
MZ_HD inline int wide_row_pos(int m) { return m < kWideP ? wide_plane_pos(m) : kWideZeroPos; }
// tap = 3 * ky + kx of a [cout, cin, 3, 3] weight -> offset of the source cell from the output's cell
MZ_HD inline int wide_tap_offset(int tap) { return (tap / 3 - 1) * kWidePW + (tap % 3 - 1); }

// LDS bytes: the activations [157 positions][2 halves][cph] fp16; the epilogue stages [128][124] floats over them
MZ_HD inline size_t wide_planes_bytes(int cin) { return static_cast<size_t>(kWidePP) * 2 * wide_cph(cin) * 2; }
MZ_HD inline size_t wide_stage_bytes() { return sizeof(float) * kWideCout * kWideStageLdm; }
MZ_HD inline size_t wide_lds_bytes(int cin) {
    return wide_planes_bytes(cin) > wide_stage_bytes() ? wide_planes_bytes(cin) : wide_stage_bytes();
}

// The range rule of the two-halves form: 8 x must be a finite fp16 after rounding.  NaN and inf fail the comparison.
MZ_HD inline bool wide_in_range(float x) { return __builtin_fabsf(x) * kWideActScale < kWideHalfMax; }

// ---- packed weights: [9 * groups + 2 spare][2 q][4 kk][cout][8 j] halves -------------------------------------------------
MZ_HD inline int64_t wide_packed_halfs(int cin, int cout) {
    return static_cast<int64_t>(9 * wide_groups(cin) + 2) * 2 * 4 * cout * 8;
}
struct WidePackSource {
    int n, ci, tap, q;     // packed half i is half q of 64 * w[n][ci][tap] ...
    bool zero;             // ... or zero (ci >= cin: the ragged last group; tap >= 9: the spare groups)
};
MZ_HD inline WidePackSource wide_pack_source(int64_t i, int cin, int cout) {
    WidePackSource s;
    const int j = static_cast<int>(i & 7);
    s.n = static_cast<int>((i >> 3) % cout);
    const int kk = static_cast<int>(((i >> 3) / cout) & 3);
    s.q = static_cast<int>(((i >> 3) / cout / 4) & 1);
    const int tg = static_cast<int>((i >> 3) / cout / 8);   // tap * groups + grp
    const int ng = wide_groups(cin);
    s.tap = tg / ng;
    s.ci = (tg % ng) * kWideGroup + 8 * kk + j;
    s.zero = s.tap >= 9 || s.ci >= cin;
    return s;
}

}  // namespace mz
