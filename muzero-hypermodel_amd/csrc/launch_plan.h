// launch_plan.h -- the one place a board-network launch is decided: which kernel a tower, a convolution or a set of heads
// gets, how many samples a workgroup takes, how much LDS it asks for and how wide the grid is.  Plain C++17 with no HIP
// include: board_conv.hip and net_kernels.hip validate their descriptors, ask a plan_* function here and switch from its
// answer to the instantiation; tests/launch_plan_check.cpp builds the same text with g++ and
// tests/test_launch_plan_cpu.py holds it to a restatement in Python (tests/board_tower_cases.py, tests/net_head_cases.py);
// wide_conv.hip asks plan_wide_conv (tests/wide_conv_check.cpp, tests/test_wide_conv_cpu.py).
// The constants and layout structs the kernels share with these plans live here too, so a launcher and its kernel
// cannot count differently.
//
// A plan function returns MZMCTS_OK or MZMCTS_ERR_INVALID and fills a small struct.  It reads no environment variable:
// the switches (MZ_TOWER_COLS, MZ_HEADS_COLS, MZ_SPLIT_BOARDS, MZ_HEADS_WAVE_PER_SAMPLE) arrive as values.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mzmcts.h"
#include "np_legacy_rng.h"   // MZ_HD
#include "wide_conv.h"

namespace mz {

constexpr size_t kLdsLimit = 160 * 1024;          // bytes of LDS a workgroup can have
constexpr int64_t kMaxBoardBatch = 0x3fffffff;    // samples of a tower / convolution launch (int indices of 4-byte planes)

MZ_HD inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
MZ_HD inline int max_int(int a, int b) { return a > b ? a : b; }

// ---- exact-fp32 convolution (board_conv3x3_kernel, board_tower_kernel) ---------------------------------------------------
constexpr int kConvWaves = 8;   // two per SIMD: one wave's LDS reads and weight loads hide under the other's MFMAs
constexpr int kConvGroup = 16;  // input channels per group = 4 k-steps; a lane fetches its 4 channels with one 16-byte read

MZ_HD inline int conv_groups(int cin) { return (cin + kConvGroup - 1) / kConvGroup; }
MZ_HD inline int conv_packed_floats(int cin, int cout) {  // [9 * groups + 2 spare][4 kk][cout][4 g]
    return (9 * conv_groups(cin) + 2) * 4 * cout * 4;
}
MZ_HD inline int padded_plane(int h, int w) { return (h + 2) * (w + 1) + 1; }   // positions of a plane with its zero border

// ---- split-precision convolution (board_tower_split_kernel) ------------------------------------------------------------------
constexpr int kSplitGroup = 32;   // input channels per MFMA (K of v_mfma_f32_16x16x32_f16)

MZ_HD inline int split_groups(int cin) { return (cin + kSplitGroup - 1) / kSplitGroup; }
MZ_HD inline int64_t split_packed_halfs(int cin, int cout) {   // [9 NG + 2 spare][2 q][4 kk][cout][8 j]
    return static_cast<int64_t>(9 * split_groups(cin) + 2) * 2 * 4 * cout * 8;
}

// ---- board-column kernels (board_tower_cols_kernel, board_tower_patch_kernel, board_heads_cols_kernel) -----------------------
constexpr int kColWaves = 4;                  // wavefronts per workgroup (independent of each other): 64 boards
constexpr int kColBoardStride = 148;          // floats between two boards' [9][16] activations (+4: bank spread of 16-byte reads)
constexpr int kColActStride = 12;             // floats between two boards' 17th-channel values [9]
constexpr int kColWaveFloats = 16 * (kColBoardStride + kColActStride) + 32;   // + the boards' input rows (16 pointers)
constexpr int kColHeadW1Floats = 16 * (16 * 9 + 1);          // LDS floats of one head's Linear-1 weights, worst case

template <int H, int W>
struct PatchGeometry {
    static constexpr int P = H * W;
    static constexpr int NPX = W / 3, NPY = H / 3, NP = NPX * NPY;    // patches per board
    static constexpr int BPW = 16 / NP;                                // boards per wavefront
    static constexpr int BS = P * 16 + 4;                              // floats between two boards' [P][16] activations
    static constexpr int WAVE_FLOATS = 2 * BPW * BS + BPW * P + 32;    // activations | skip | 17th channel | input rows
    static_assert(H % 3 == 0 && W % 3 == 0 && 16 % NP == 0 && NP > 1, "boards of 2, 4, 8 or 16 patches of 3 x 3");
    static_assert((BPW * 16 * P) % 64 == 0, "the fill walks whole wavefronts");
};

// ---- heads (conv_head_kernel, conv_head_mfma_kernel) ------------------------------------------------------------------------
constexpr int kHeadWaves = 4;
constexpr int kTileSamples = 16;
constexpr int kMaxConvSteps = 16;   // channels / 4 <= 16: the 1x1 convolution's weights stay in registers (4 or 16 k-steps)
constexpr int kMaxHeads = 3;        // heads sharing a launch, each reading its own tensor: blockIdx.y picks the head

struct HeadShape {
    int C, P, R, Hd, O;  // channels, board positions, reduced channels, hidden units, outputs
    int split;           // lanes sharing one hidden unit's dot product: 64 / pow2(Hd), at least 1
    MZ_HD int RP() const { return R * P; }
    MZ_HD int conv_w() const { return 0; }
    MZ_HD int conv_b() const { return conv_w() + R * C; }
    MZ_HD int fc1_w() const { return conv_b() + R; }
    MZ_HD int fc1_b() const { return fc1_w() + Hd * RP(); }
    MZ_HD int fc2_w() const { return fc1_b() + Hd; }
    MZ_HD int fc2_b() const { return fc2_w() + O * Hd; }
    MZ_HD int per_wave() const { return (fc2_b() + O + 3) & ~3; }  // 16-byte aligned boards
    // per wave: [x C*P | y R*P | partial sums split*Hd | h Hd], padded to a multiple of 4 words
    MZ_HD int wave_floats() const { return (C * P + RP() + split * Hd + Hd + 3) & ~3; }
    MZ_HD int total() const { return per_wave() + kHeadWaves * wave_floats(); }
};

struct MfmaHeadShape {
    int C, P, R, Hd, O;
    MZ_HD int RP() const { return R * P; }
    MZ_HD int ys_stride() const { return RP() + 1; }      // (+1: the 16 sample rows fall into different banks)
    MZ_HD int hs_stride() const { return Hd + 1; }
    MZ_HD int w1_stride() const { return RP() + 1; }
    MZ_HD int w2_stride() const { return Hd + 1; }
    MZ_HD int nt1() const { return (Hd + 15) / 16; }
    MZ_HD int nt2() const { return (O + 15) / 16; }
    // LDS (floats): W1 [16 nt1][w1_stride] | b1 [16 nt1] | W2 [16 nt2][w2_stride] | b2 [16 nt2] | per wave { ys, hs }
    MZ_HD int off_b1() const { return 16 * nt1() * w1_stride(); }
    MZ_HD int off_w2() const { return off_b1() + 16 * nt1(); }
    MZ_HD int off_b2() const { return off_w2() + 16 * nt2() * w2_stride(); }
    MZ_HD int off_waves() const { return off_b2() + 16 * nt2(); }
    MZ_HD int wave_floats() const { return kTileSamples * (ys_stride() + hs_stride()); }
    MZ_HD int total() const { return off_waves() + kHeadWaves * wave_floats(); }
};

// ============================================================================================================================
// The per-layer convolution (mzmcts_board_conv3x3): board_conv3x3_kernel<NT, H, W, SB, residual, relu>
// ============================================================================================================================
inline bool board_conv_supported(int cin, int cout, int height, int width) {
    const bool shape = (height == 6 && width == 7) || (height == 6 && width == 6) || (height == 3 && width == 3);
    return shape && (cout == 64 || cout == 16) && cin >= 1 && cin <= 80;
}

struct ConvPlan {
    int nt, h, w, sb;       // the instantiation; sb = samples per workgroup: 8 waves x <= 6 row tiles each, planes within LDS
    unsigned grid, block;
    size_t lds;             // bytes: the input planes, later the output staging tile with scale | shift behind it
};

inline int plan_board_conv(int64_t batch, int cin, int cout, int height, int width, ConvPlan* out) {
    *out = ConvPlan{};
    if (batch < 0 || batch > kMaxBoardBatch || !board_conv_supported(cin, cout, height, width)) return MZMCTS_ERR_INVALID;
    ConvPlan& p = *out;
    p.nt = cout / 16;
    p.h = height;
    p.w = width;
    if (width == 7) p.sb = cout == 64 ? 4 : 8;
    else if (height == 6) p.sb = cout == 64 ? 4 : 16;
    else p.sb = cout == 64 ? 16 : 32;
    const size_t planes = static_cast<size_t>(p.sb) * padded_plane(height, width) * (conv_groups(cin) * kConvGroup + 4);
    const size_t stage = static_cast<size_t>(cout) * (p.sb * height * width + 1) + 2 * cout;
    p.lds = sizeof(float) * (planes > stage ? planes : stage);
    p.block = 64 * kConvWaves;
    if (batch == 0) return MZMCTS_OK;
    if (p.lds > kLdsLimit) return MZMCTS_ERR_INVALID;
    p.grid = static_cast<unsigned>(ceil_div(batch, p.sb));
    return MZMCTS_OK;
}

// ============================================================================================================================
// The 128-channel layer of 11 x 11 boards (mzmcts_board_conv_wide): wide_conv_split_kernel, one board per workgroup
// ============================================================================================================================
// A shape of its own beside board_conv_supported (whose answers stay as they are): the geometry is wide_conv.h's.
inline bool wide_conv_supported(int cin, int cout, int height, int width) {
    return height == kWideH && width == kWideW && cout == kWideCout && cin >= 1 && cin <= kWideMaxCin;
}

struct WidePlan {
    int groups, cph;        // groups of 32 input channels (the last zero-padded); halves per (position, half) in LDS
    unsigned grid, block;
    size_t lds;             // bytes: the board as two fp16 halves, later the output staging tile
};

inline int plan_wide_conv(int64_t batch, int cin, int cout, int height, int width, WidePlan* out) {
    *out = WidePlan{};
    if (batch < 0 || batch > kMaxBoardBatch || !wide_conv_supported(cin, cout, height, width)) return MZMCTS_ERR_INVALID;
    WidePlan& p = *out;
    p.groups = wide_groups(cin);
    p.cph = wide_cph(cin);
    p.lds = wide_lds_bytes(cin);
    p.block = kWideThreads;
    if (batch == 0) return MZMCTS_OK;
    if (p.lds > kLdsLimit) return MZMCTS_ERR_INVALID;
    p.grid = static_cast<unsigned>(batch);
    return MZMCTS_OK;
}

// ============================================================================================================================
// Towers (mzmcts_board_tower, _heads, _split, _gathered, mzmcts_board_tower_blocks)
// ============================================================================================================================
enum class TowerKernel {
    kNone,       // no tower for this shape (64 channels on 3 x 3 boards)
    kRowTile,    // board_tower_kernel<nt, h, w, sb>
    kCols,       // board_tower_cols_kernel<3, 3, false>
    kColsHeads,  // board_tower_cols_kernel<3, 3, true>
    kPatch,      // board_tower_patch_kernel<6, 6>
    kSplit,      // board_tower_split_kernel<h, w, sb, waves>
};

struct TowerShape {
    int64_t batch;
    int cin0, channels, height, width, n_layers;
    const int32_t* layer_cin;   // [n_layers], as the descriptors state it: cin0, then channels
    bool split;                 // the split-precision form; else exact fp32
    bool const_plane;           // split: the input's last plane is one value per sample, taken from the table
    bool layer1_skip;           // layer 1 adds the tower's input (a tower that starts with a residual block)
    bool gated;                 // layer 0 carries a gate buffer
    int n_heads;                // heads computed inside the launch
    bool weights_aligned16;     // every packed weight pointer is 16-byte aligned (the patch kernel reads float4)
    bool cols_on;               // MZ_TOWER_COLS is not "off" (read on every call)
    int split_boards;           // MZ_SPLIT_BOARDS: boards per workgroup of the 6 x 7 split tower, 4, 2 or 1 (once per process)
};

struct TowerPlan {
    TowerKernel kernel;
    int nt, h, w, sb, waves;    // template arguments (those the kernel has; waves of the split kernel)
    int samples;                // per workgroup
    int cp0, cp1;               // channel strides of the two activation buffers: floats (fp32), halves per half (split)
    unsigned grid, block;
    size_t lds;                 // bytes
    int gate_samples;           // samples per gate entry = per workgroup of the split launch of this board
};

// Boards per workgroup of the split-precision 64-channel tower.  6 x 7: TWO boards on FOUR wavefronts (84 rows = 6 tiles,
// three per wavefront, as with 4 boards on 8), because half the LDS lets two workgroups share a CU: one's fill / epilogue
// / barrier / export phases (55 % of a workgroup's life, profiles/r02_tower_phase_stamps.jsonl) run under the other's MFMAs.
// MZ_SPLIT_BOARDS=4|2|1 selects the shape (A/B measurements).  6 x 6: 4 boards (3 fill the MFMA rounds better -- 126 rows
// = 8 tiles -- and 2 let two workgroups share a CU, but both measured slower at 4096 Connect4 boards: 700 / 744 / 900 us
// per launch for 4 / 3 / 2; again after the packed epilogue, 8192 boards with heads: 1289 us for 4, 1366 us for 3).
inline int split_samples(int height, int width, int split_boards) {
    if (height == 6 && width == 7) return (split_boards == 4 || split_boards == 1) ? split_boards : 2;
    return height == 3 ? 16 : 4;
}

inline size_t row_tile_lds_bytes(int h, int w, int sb, int cp0, int cp1) {       // two plane buffers | per sample: pointer, float
    return sizeof(float) * sb * padded_plane(h, w) * (cp0 + cp1) + (sizeof(float*) + sizeof(float)) * sb;
}
inline size_t split_lds_bytes(int h, int w, int sb, int cph0, int cph1) {        // the same, two fp16 halves per value
    return 2 * static_cast<size_t>(sb) * padded_plane(h, w) * 2 * (cph0 + cph1) + (sizeof(float*) + sizeof(float)) * sb;
}

// the board-column kernels take 16-channel towers on 3 x 3 (cols) and 6 x 6 (patch) boards whose input has 16 or 17 planes
inline bool tower_cols_applies(const TowerShape& s) {
    const bool board = (s.height == 3 && s.width == 3) || (s.height == 6 && s.width == 6);
    return s.cols_on && s.channels == 16 && board && (s.cin0 == 16 || s.cin0 == 17);
}

inline int plan_tower(const TowerShape& s, TowerPlan* out) {
    *out = TowerPlan{};
    if (s.batch < 0 || s.batch > kMaxBoardBatch || s.n_layers < 1 || s.n_layers > 16 || !s.layer_cin ||
        !board_conv_supported(s.cin0, s.channels, s.height, s.width) || s.n_heads < 0 || s.n_heads > kMaxHeads)
        return MZMCTS_ERR_INVALID;
    for (int l = 0; l < s.n_layers; ++l)
        if (s.layer_cin[l] != (l == 0 ? s.cin0 : s.channels)) return MZMCTS_ERR_INVALID;
    if (s.split) {
        if (s.channels != 64 || s.n_heads > 0 || (s.const_plane && s.cin0 < 2)) return MZMCTS_ERR_INVALID;
        // The constant plane is never staged into LDS (its contribution comes from the table).  A skip on layer 1 -- a
        // tower that starts with a residual block -- adds the input's first `channels` planes: with cin0 <= channels the
        // constant plane is one of them and would be read as zeros.  Refused; no network builds such a tower (the
        // dynamics input has channels + 1 planes and starts with a plain convolution).
        if (s.const_plane && s.n_layers > 1 && s.layer1_skip && s.cin0 <= s.channels) return MZMCTS_ERR_INVALID;
    } else {
        if (s.gated && s.channels != 64) return MZMCTS_ERR_INVALID;   // (the hand-over exists between the two 64-channel forms)
        // heads inside the launch: the 3 x 3 board-column kernel only -- decided before anything is launched
        if (s.n_heads > 0 && !(s.height == 3 && tower_cols_applies(s))) return MZMCTS_ERR_INVALID;
    }
    TowerPlan& p = *out;
    const int h = s.height, w = s.width;
    p.h = h;
    p.w = w;
    p.gate_samples = split_samples(h, w, s.split_boards);
    // ---- the kernel and its samples per workgroup -------------------------------------------------------------------
    // 64 channels on 3 x 3 boards have no tower: a workgroup's 8 wavefronts want the row tiles of 16 boards, and two
    // activation buffers of 16 padded planes are 179 KB (fp32, 64 + 4 channels) or 189 KB (split, two halves of 64 + 8)
    // -- over the 160 KB of a workgroup whatever cin0 is.  Refused by name (the caller keeps the per-layer kernels).
    if (s.channels == 64 && h == 3) {
        p.samples = 16;
    } else if (s.split) {
        p.kernel = TowerKernel::kSplit;
        p.sb = p.gate_samples;
        p.waves = (w == 7 && p.sb < 4) ? 2 * p.sb : kConvWaves;
        p.samples = p.sb;
        p.block = 64u * p.waves;
    } else if (s.channels == 64) {
        p.kernel = TowerKernel::kRowTile;
        p.nt = 4;
        p.sb = 4;
    } else if (h == 3 && tower_cols_applies(s)) {
        p.kernel = s.n_heads > 0 ? TowerKernel::kColsHeads : TowerKernel::kCols;
        p.samples = 16 * kColWaves;
    } else if (w == 6 && tower_cols_applies(s) && s.weights_aligned16) {
        p.kernel = TowerKernel::kPatch;
        p.samples = PatchGeometry<6, 6>::BPW * kColWaves;
    } else {
        // A 16-channel tower has ONE column tile, so its 8 wavefronts split the SB x H x W output rows into 16-row tiles
        // and every wavefront runs ceil(tiles / 8) of them per k-step: 16 x 9 = 144 rows = 9 tiles cost two rounds for
        // little more than one round's work.  With few boards that choice stands (more workgroups than CUs matters
        // most); with many, SB is the count whose rows fit ONE round and whose LDS lets two or more workgroups share a
        // CU, so that one's fill / epilogue / export phases run under another's MFMAs: 14 x 9 = 126 rows = 8 tiles, a
        // tile for every wavefront (measured at 65536 TicTacToe boards: SB 16 / 28 / 12 / 8 = 318 / 313 / 300 / 353 us
        // per launch, and 12 -> 14: 374 -> 338 us with heads -- 12 x 9 = 108 rows are 7 tiles and leave the eighth
        // wavefront idle; 6x6, 16384 boards: SB 4 / 7 / 3 = 513 / 513 / 428 us).
        const bool many = s.batch >= 16384;
        p.kernel = TowerKernel::kRowTile;
        p.nt = 1;
        if (w == 7) p.sb = many ? 6 : 4;
        else if (h == 6) p.sb = many ? 3 : 4;
        else p.sb = many ? 14 : 16;
    }
    // ---- LDS ----------------------------------------------------------------------------------------------------------
    if (p.kernel == TowerKernel::kRowTile) {
        p.samples = p.sb;
        p.block = 64 * kConvWaves;
        p.cp0 = conv_groups(s.cin0) * kConvGroup + 4;
        p.cp1 = 4;
        for (int l = 0; l < s.n_layers; ++l) {             // layer l reads buffer l & 1
            int& cp = (l & 1) ? p.cp1 : p.cp0;
            cp = max_int(cp, conv_groups(s.layer_cin[l]) * kConvGroup + 4);
        }
        p.cp0 = max_int(p.cp0, 16 * p.nt + 4);             // outputs (16 NT channels) land in either buffer
        p.cp1 = max_int(p.cp1, 16 * p.nt + 4);
        p.lds = row_tile_lds_bytes(h, w, p.sb, p.cp0, p.cp1);
    } else if (p.kernel == TowerKernel::kSplit) {
        p.cp0 = p.cp1 = 64 + 8;                            // outputs are 64 channels in either buffer
        for (int l = 0; l < s.n_layers; ++l) {
            const int cin_conv = s.layer_cin[l] - ((l == 0 && s.const_plane) ? 1 : 0);
            int& cp = (l & 1) ? p.cp1 : p.cp0;
            cp = max_int(cp, split_groups(cin_conv) * kSplitGroup + 8);
        }
        p.lds = split_lds_bytes(h, w, p.sb, p.cp0, p.cp1);
    } else if (p.kernel == TowerKernel::kPatch) {
        p.block = 64 * kColWaves;
        p.lds = sizeof(float) * kColWaves * PatchGeometry<6, 6>::WAVE_FLOATS;
    } else if (p.kernel != TowerKernel::kNone) {
        p.block = 64 * kColWaves;
        p.lds = sizeof(float) * (kColWaves * kColWaveFloats + (s.n_heads > 0 ? 3 * kColHeadW1Floats : 0));
    }
    // ---- the launch -------------------------------------------------------------------------------------------------
    if (s.batch == 0) return MZMCTS_OK;                    // (nothing to launch: before any size check)
    if (p.kernel == TowerKernel::kNone || p.lds > kLdsLimit) return MZMCTS_ERR_INVALID;
    const int64_t blocks = ceil_div(s.batch, p.samples);
    // a gated fp32 launch is a fixed grid whose workgroups walk the gate entries
    p.grid = static_cast<unsigned>((!s.split && s.gated && blocks > 256) ? 256 : blocks);
    return MZMCTS_OK;
}

// mzmcts_board_tower_blocks: workgroups of samples a tower launch of `batch` samples has, -1 where there is no answer.  For a
// 64-channel tower: of the SPLIT launch, whose workgroups are the units of the overflow hand-over (the gate buffer has an
// entry per block); for 16 channels: of the row-tile launch, and none for 6 x 7 boards, as ever.  The samples per block
// are the plan's, also where the plan then refuses the launch for its size (64 channels on 3 x 3 boards).
inline int64_t board_tower_blocks(int64_t batch, int channels, int height, int width, int split_boards) {
    if (batch < 0 || !board_conv_supported(channels, channels, height, width) || (channels == 16 && width == 7)) return -1;
    const int32_t cin = channels;
    TowerShape s{};
    s.batch = batch < kMaxBoardBatch ? batch : kMaxBoardBatch;      // (the plan's own limit; `many` holds from 16384 on)
    s.cin0 = s.channels = channels;
    s.height = height;
    s.width = width;
    s.n_layers = 1;
    s.layer_cin = &cin;
    s.split = channels == 64;
    s.split_boards = split_boards;
    TowerPlan p;
    plan_tower(s, &p);                                              // (its refusal of the launch is not this question's)
    return p.samples > 0 ? ceil_div(batch, p.samples) : -1;
}

// ============================================================================================================================
// Heads as a launch of their own (mzmcts_conv_heads_multi)
// ============================================================================================================================
enum class HeadsKernel {
    kNone,   // no form fits the 160 KB of a workgroup: the caller keeps the torch modules
    kCols,   // board_heads_cols_kernel: 16-channel 3 x 3 heads in the board-column shape
    kMfma,   // conv_head_mfma_kernel: a wavefront takes 16 samples through the matrix cores
    kWave,   // conv_head_kernel: a wavefront per sample
};

struct HeadDims {
    int C, P, R, Hd, O;
};

// shapes the board-column heads take (inside a tower launch and as a launch of their own)
inline bool cols_head_ok(const HeadDims& d) {
    return d.C == 16 && d.P == 9 && d.R >= 1 && d.R <= 16 && d.Hd >= 1 && d.Hd <= 16 && d.O >= 1 && d.O <= 32;
}
// shapes the matrix-core heads take: reduced channels <= 16 (one column tile), channels <= 64, hidden <= 64, outputs <= 32
inline bool mfma_head_ok(const HeadDims& d) { return d.R <= 16 && d.C <= 4 * kMaxConvSteps && d.Hd <= 64 && d.O <= 32; }

// lanes sharing one hidden unit's dot product in conv_head_kernel (a power of two; 1 from 33 units on)
inline int wave_head_split(int hidden) {
    int split = 1;
    while (split * 2 * hidden <= 64) split *= 2;
    return split;
}

struct MfmaForm {
    int nt1, nt2, ks, g;    // mfma_head_tiles<NT1, NT2, KS, G>
};
inline MfmaForm mfma_form(const MfmaHeadShape& s) {
    const bool narrow = s.C <= 16;
    return MfmaForm{s.nt1() == 1 ? 1 : 4, s.nt2() == 1 ? 1 : 2, narrow ? 4 : 16, narrow ? 6 : 2};
}

struct HeadsPlan {
    HeadsKernel kernel;
    HeadShape wave[kMaxHeads];       // kWave
    MfmaHeadShape mfma[kMaxHeads];   // kMfma
    MfmaForm form[kMaxHeads];        // kMfma: the instantiation each head runs
    size_t lds;                      // bytes: the widest head's
    int per_cu;                      // workgroups sharing a CU
    unsigned grid_x, grid_y, block;  // (mfma, wave: persistent workgroups, at most 256 * per_cu of them)
};

// cols_on: MZ_HEADS_COLS is not "off" (read on every call); use_mfma: MZ_HEADS_WAVE_PER_SAMPLE is unset (once per process)
inline int plan_heads(const HeadDims* heads, int n_heads, int64_t batch, bool cols_on, bool use_mfma, HeadsPlan* out) {
    *out = HeadsPlan{};
    if (!heads || n_heads < 1 || n_heads > kMaxHeads || batch < 0 || batch > 0x7fffffff) return MZMCTS_ERR_INVALID;
    HeadsPlan& p = *out;
    bool cols = cols_on && batch <= kMaxBoardBatch, mfma = use_mfma;   // (mfma at any batch: a sample's logits do not
    for (int h = 0; h < n_heads; ++h) {                                //  depend on how many samples share its launch)
        const HeadDims& d = heads[h];
        if (d.C <= 0 || d.P <= 0 || d.R <= 0 || d.Hd <= 0 || d.O <= 0 || d.C != heads[0].C || d.P != heads[0].P)
            return MZMCTS_ERR_INVALID;
        cols = cols && cols_head_ok(d);
        mfma = mfma && mfma_head_ok(d);
    }
    p.grid_y = static_cast<unsigned>(n_heads);
    if (cols) {
        p.kernel = HeadsKernel::kCols;
        p.lds = sizeof(float) * (kColWaves * kColWaveFloats + kColHeadW1Floats);
        p.per_cu = 1;
        p.block = 64 * kColWaves;
        p.grid_x = static_cast<unsigned>(ceil_div(batch, 16 * kColWaves));
        return MZMCTS_OK;
    }
    p.block = 64 * kHeadWaves;
    if (mfma) {                                                        // (the widest head's layout has to fit)
        for (int h = 0; h < n_heads; ++h) {
            const HeadDims& d = heads[h];
            const size_t bytes = sizeof(float) * static_cast<size_t>(MfmaHeadShape{d.C, d.P, d.R, d.Hd, d.O}.total());
            if (bytes > p.lds) p.lds = bytes;
        }
        mfma = p.lds <= kLdsLimit;
    }
    if (mfma) {
        for (int h = 0; h < n_heads; ++h) {
            p.mfma[h] = MfmaHeadShape{heads[h].C, heads[h].P, heads[h].R, heads[h].Hd, heads[h].O};
            p.form[h] = mfma_form(p.mfma[h]);
        }
    } else {
        p.lds = 0;
        for (int h = 0; h < n_heads; ++h) {
            const HeadDims& d = heads[h];
            p.wave[h] = HeadShape{d.C, d.P, d.R, d.Hd, d.O, wave_head_split(d.Hd)};
            const size_t bytes = sizeof(float) * static_cast<size_t>(p.wave[h].total());
            if (bytes > p.lds) p.lds = bytes;
        }
        if (p.lds > kLdsLimit) return MZMCTS_ERR_INVALID;
    }
    p.kernel = mfma ? HeadsKernel::kMfma : HeadsKernel::kWave;
    const size_t fit = kLdsLimit / p.lds, most = mfma ? 4 : 8;
    p.per_cu = static_cast<int>(fit < 1 ? 1 : (fit > most ? most : fit));
    const int64_t rounds = ceil_div(mfma ? ceil_div(batch, kTileSamples) : batch, kHeadWaves);
    p.grid_x = static_cast<unsigned>(rounds < 256 * p.per_cu ? rounds : 256 * p.per_cu);
    return MZMCTS_OK;
}

}  // namespace mz
