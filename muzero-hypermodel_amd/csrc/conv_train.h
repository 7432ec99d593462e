// conv_train.h -- the padded, stride-1 3 x 3 convolution of a residual network IN TRAINING: forward, data gradient and
// weight gradient (include/mztrain.h mztrain_conv_*), written once for the HIP kernels of conv_train.hip and for a host
// compiler (mztrain_conv_reference_*, tests/conv_train_check.cpp).  No HIP include.
//
// Every fused multiply-add is spelled fmaf and nothing of the form a * b + c is left to the compiler (the library is built
// with -ffp-contract=off): host and device produce the same bits.
//
// x [B][cin][H][W], w [cout][cin][3][3], y / dy [B][cout][H][W], all float32 and contiguous; P = H * W; tap = ky * 3 + kx
// reads xpad[b][ci][y + ky - 1][x + kx - 1], a float32 zero outside the board (a zero that IS multiplied: a NaN or an
// infinite weight or dy at a border tap gives NaN, as in the kernels, which read staged or predicated zeros).
//
// Forward (and the data gradient, which is the same convolution of dy with the virtual weight
// w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], ci < dx_planes: cin' = cout, cout' = dx_planes): the k-ordered fmaf chain
// of board_conv.hip from a float32 zero, one v_mfma_f32_16x16x4_f32 after the other:
//     for tap = 0..8:  for grp = 0..groups-1 (16 input channels each):  for g = 0..steps-1:  for kk = 0..3:
//         ci = 16 grp + 4 kk + g;      acc = fmaf(xpad[ci] (0 for ci >= cin), w[n][ci][tap] (0 for ci >= cin), acc)
// steps = 4, but min(4, cin - 16 (groups - 1)) in a tap's last group (17 planes: one k-step, its channels 20, 24 and 28
// are 0 * 0 terms).  The output is acc * 1 + 0 (the inference epilogue with a ones / zeros scale / shift pair): a -0 sum
// comes out as +0.
//
// Weight gradient: dw[co][ci][tap] = sum over k = b * P + p, ascending, of dy[b][co][p] * xpad[b][ci][p + tap].  The
// reduction is cut into slices of kSlice = 64 indices, slice s = [64 s, 64 s + 64); within a slice the sum is an ascending
// fmaf chain in float32 from a float32 zero of always 64 terms (indices past B * P are 0 * 0 terms) -- 16
// v_mfma_f32_16x16x4_f32 --; the slice sums are added in ascending s to a float64 zero and the total is rounded to float32
// once.  No atomics; every entry of dw is written by every call.
//
// Packings: the layout of mzmcts_board_conv_pack (board_conv.hip),
//     wt[(((tap * NG + grp) * 4 + kk) * cout + n) * 4 + g] = w[n][16 grp + 4 kk + g][tap], 0 for channels >= cin and for the
// two spare groups behind tap 8; pack_forward_value / pack_dgrad_value give entry i of the two buffers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "launch_plan.h"

namespace mz {
namespace cvt {

constexpr int kSlice = 64;        // reduction indices per float32 chain of the weight gradient (MZTRAIN_CONV_SLICE)
constexpr int kWgradWaves = 16;   // wavefronts of a weight-gradient workgroup: slices of one round
constexpr int kAffine = 64;       // floats of each half of the ones | zeros pair the pack launch writes (MZTRAIN_CONV_AFFINE)

MZ_HD inline bool dx_planes_ok(int cin, int dx_planes) {
    return dx_planes == 0 || ((dx_planes == 16 || dx_planes == 64) && dx_planes <= cin);
}
// a shape of board_conv_supported whose launch plan also fits a workgroup's LDS (16 output channels take 32, 16 or 8 samples
// per workgroup: their planes fit up to 48 input channels on 3 x 3 boards, 32 on 6 x 6, 64 on 6 x 7)
inline bool conv_launchable(int cin, int cout, int height, int width) {
    ConvPlan plan;
    return plan_board_conv(1, cin, cout, height, width, &plan) == MZMCTS_OK;
}
// forward and weight gradient of the shape, and for need_dx_planes > 0 the data gradient as the convolution cout -> need_dx_planes
inline bool conv_supported(int cin, int cout, int height, int width, int need_dx_planes) {
    if (!conv_launchable(cin, cout, height, width) || need_dx_planes < 0 || !dx_planes_ok(cin, need_dx_planes)) return false;
    return need_dx_planes == 0 || conv_launchable(cout, need_dx_planes, height, width);
}

// ---- the packings ----------------------------------------------------------------------------------------------------------
struct PackSlot {
    int n, ci, tap;      // output channel, input channel and tap of packed entry i, as the convolution kernel sees them
    bool live;           // false: a padding channel or a spare group (the entry is 0)
};
MZ_HD inline PackSlot pack_slot(int i, int cin, int cout) {
    const int g = i & 3;
    const int n = (i >> 2) % cout;
    const int kk = ((i >> 2) / cout) & 3;
    const int tg = (i >> 2) / cout / 4;                 // tap * NG + grp
    const int ng = conv_groups(cin);
    PackSlot s;
    s.n = n;
    s.tap = tg / ng;
    s.ci = (tg % ng) * kConvGroup + 4 * kk + g;
    s.live = s.tap < 9 && s.ci < cin;
    return s;
}
// entry i of the forward packing of w [cout][cin][9]
MZ_HD inline float pack_forward_value(const float* w, int cin, int cout, int i) {
    const PackSlot s = pack_slot(i, cin, cout);
    return s.live ? w[(static_cast<size_t>(s.n) * cin + s.ci) * 9 + s.tap] : 0.f;
}
// entry i of the data-gradient packing: the forward packing of w'[n][c][tap] = w[c][n][8 - tap], n < dx_planes, c < cout
MZ_HD inline float pack_dgrad_value(const float* w, int cin, int cout, int dx_planes, int i) {
    const PackSlot s = pack_slot(i, cout, dx_planes);
    return s.live ? w[(static_cast<size_t>(s.ci) * cin + s.n) * 9 + (8 - s.tap)] : 0.f;
}

// ---- the weight gradient's launch ------------------------------------------------------------------------------------------
struct WgradPlan {
    int h, w;
    int m_tiles, n_tiles;        // 16 x 16 tiles of dw seen as [cout][cin * 9]; a workgroup owns one
    int64_t slices;              // slices per block: every workgroup walks the whole reduction
    int64_t rounds;              // ceil(slices / kWgradWaves): a wavefront takes one slice per round
    unsigned grid, block;
    size_t lds;                  // bytes: one 16 x 16 float tile per wavefront
};

// the largest batch whose element indices b * max(cin, cout) * P + ... and reduction indices k + 64 stay within int32
inline int64_t wgrad_max_batch(int cin, int cout, int height, int width) {
    const int64_t widest = cin > cout ? cin : cout;
    return (INT64_C(0x7fffffff) - kSlice) / (widest * height * width);
}

inline int plan_conv_wgrad(int64_t batch, int cin, int cout, int height, int width, WgradPlan* out) {
    *out = WgradPlan{};
    if (!conv_launchable(cin, cout, height, width) || batch < 1 || batch > wgrad_max_batch(cin, cout, height, width))
        return MZMCTS_ERR_INVALID;
    WgradPlan& p = *out;
    p.h = height;
    p.w = width;
    p.m_tiles = cout / 16;
    p.n_tiles = static_cast<int>(ceil_div(cin * 9, 16));
    p.slices = ceil_div(batch * height * width, kSlice);
    p.rounds = ceil_div(p.slices, kWgradWaves);
    p.grid = static_cast<unsigned>(p.m_tiles * p.n_tiles);
    p.block = 64 * kWgradWaves;
    p.lds = sizeof(float) * kWgradWaves * 256;
    return MZMCTS_OK;
}

// ---- the rule on host arrays -------------------------------------------------------------------------------------------------
// out[b][n][p] of the convolution of x [B][cin][P] with the weight weight_at(n, ci, tap), n < cout
template <class WeightAt>
inline void reference_conv(const float* x, WeightAt weight_at, float* out, int64_t batch, int cin, int cout, int height,
                           int width) {
    const int P = height * width;
    const int ng = conv_groups(cin);
    const int last_steps = cin - (ng - 1) * kConvGroup < 4 ? cin - (ng - 1) * kConvGroup : 4;
    for (int64_t b = 0; b < batch; ++b)
        for (int n = 0; n < cout; ++n)
            for (int p = 0; p < P; ++p) {
                float acc = 0.f;
                for (int tap = 0; tap < 9; ++tap) {
                    const int yy = p / width + tap / 3 - 1, xx = p % width + tap % 3 - 1;
                    const bool inside = yy >= 0 && yy < height && xx >= 0 && xx < width;
                    for (int grp = 0; grp < ng; ++grp) {
                        const int steps = grp == ng - 1 ? last_steps : 4;
                        for (int g = 0; g < steps; ++g)
                            for (int kk = 0; kk < 4; ++kk) {
                                const int ci = grp * kConvGroup + 4 * kk + g;
                                const bool real = ci < cin;
                                const float a = (real && inside) ? x[(b * cin + ci) * P + yy * width + xx] : 0.f;
                                const float w = real ? weight_at(n, ci, tap) : 0.f;
                                acc = fmaf(a, w, acc);
                            }
                    }
                }
                out[(b * cout + n) * P + p] = acc * 1.f + 0.f;
            }
}

inline void reference_forward(const float* x, const float* w, float* y, int64_t batch, int cin, int cout, int height,
                              int width) {
    reference_conv(x, [=](int n, int ci, int tap) { return w[(static_cast<size_t>(n) * cin + ci) * 9 + tap]; }, y, batch, cin,
                   cout, height, width);
}

// dx [B][dx_planes][P]: the gradient of the input's first dx_planes planes
inline void reference_dgrad(const float* dy, const float* w, float* dx, int64_t batch, int cin, int cout, int height,
                            int width, int dx_planes) {
    reference_conv(dy, [=](int n, int co, int tap) { return w[(static_cast<size_t>(co) * cin + n) * 9 + (8 - tap)]; }, dx,
                   batch, cout, dx_planes, height, width);
}

inline void reference_wgrad(const float* x, const float* dy, float* dw, int64_t batch, int cin, int cout, int height,
                            int width) {
    const int P = height * width;
    const int64_t K = batch * P;
    const int64_t slices = ceil_div(K, kSlice);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                double total = 0.0;
                for (int64_t s = 0; s < slices; ++s) {
                    float acc = 0.f;
                    for (int j = 0; j < kSlice; ++j) {
                        const int64_t k = s * kSlice + j;
                        float a = 0.f, v = 0.f;
                        if (k < K) {
                            const int64_t b = k / P;
                            const int p = static_cast<int>(k - b * P);
                            const int yy = p / width + tap / 3 - 1, xx = p % width + tap % 3 - 1;
                            a = dy[(b * cout + co) * P + p];
                            if (yy >= 0 && yy < height && xx >= 0 && xx < width) v = x[(b * cin + ci) * P + yy * width + xx];
                        }
                        acc = fmaf(a, v, acc);
                    }
                    total = total + static_cast<double>(acc);
                }
                dw[(static_cast<size_t>(co) * cin + ci) * 9 + tap] = static_cast<float>(total);
            }
}

}  // namespace cvt
}  // namespace mz
