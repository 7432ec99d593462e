// wide_conv.hip -- relu(bn(conv3x3(x)) [+ skip]) for 11 x 11 boards with 128 output channels in ONE launch per layer:
// Gomoku's residual networks (reference models.py:213-229 conv3x3 and ResidualBlock.forward, 318-330, 399-420), whose
// two padded activation buffers do not fit the LDS of a workgroup as a one-launch tower (166 KB of 160), so the layer is
// the unit.  The arithmetic is board_tower_split_kernel's (board_conv.hip): every fp32 operand is carried as TWO fp16
// numbers, x * 2^s = h0 + h1, a product as three v_mfma_f32_16x16x32_f16 with fp32 accumulation,
//     hi += w0 a0,   lo += w1 a0,   lo += w0 a1                       (w1 a1 ~ 2^-22 dropped)
// with the powers of two (activations x 8, weights x 64) removed exactly in the epilogue.
//
// A workgroup owns one board.  Where a value of the board leaves the two-halves form's range (|x| * 8 >= 65504, inf, NaN:
// wide_conv.h wide_in_range) the WHOLE workgroup takes a plain fp32 branch instead -- one fmaf chain per output in k order
// (tap-major, then channel) from the fp32 input and the unpacked weight -- so the launch never stores a silently wrong
// number and needs no second launch or gate buffer.  That branch is slow and simple on purpose: hidden states are min-max
// rescaled and activations batch-normed, it is not expected to run.
//
// Geometry, packed-weight index rule and range rule: wide_conv.h; the launch: launch_plan.h plan_wide_conv.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mzmcts.h"
#include "board_launch.h"

namespace mz {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// wh[i] = half q of 64 * w[n][ci][tap] by wide_pack_source (board_conv_pack_split_kernel's index rule with
// cin_conv = cin_total: no constant-plane table, the dynamics input's action plane is an ordinary 129th plane)
__global__ __launch_bounds__(256) void wide_conv_pack_kernel(const float* __restrict__ w, _Float16* __restrict__ wh, int cin,
                                                             int cout) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= wide_packed_halfs(cin, cout)) return;
    const WidePackSource s = wide_pack_source(i, cin, cout);
    const float v = s.zero ? 0.f : w[(static_cast<size_t>(s.n) * cin + s.ci) * 9 + s.tap] * kWideWtScale;
    const _Float16 h0 = static_cast<_Float16>(v);
    const _Float16 h1 = static_cast<_Float16>(v - static_cast<float>(h0));
    wh[i] = s.q ? h1 : h0;
}

__global__ __launch_bounds__(kWideThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void wide_conv_split_kernel(
    const float* __restrict__ x, const _Float16* __restrict__ wh, const float* __restrict__ weight,
    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ residual,
    float* __restrict__ out, int32_t* __restrict__ exact_boards, int cin, int relu) {
    constexpr int P = kWideP;
    constexpr int COUT = kWideCout;
    constexpr int THREADS = kWideThreads;
    constexpr int RG = 2;                               // row groups; wave = (column pair, row group)
    constexpr int MTW = kWideRowTiles / RG;             // 4 row tiles x 2 column tiles per wavefront
    constexpr int LDM = kWideStageLdm;
    constexpr int TPP = THREADS / P;                    // planes a plane-wise pass walks at once (4)
    constexpr int WALKERS = TPP * P;                    // 484 threads: one board position each
    extern __shared__ __attribute__((aligned(16))) _Float16 hl[];   // [157][2][cph] halves, later float [128][LDM]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int ng = wide_groups(cin);
    const int CPH = wide_cph(cin);
    const float* xb = x + static_cast<size_t>(blockIdx.x) * cin * P;
    const size_t g0 = static_cast<size_t>(blockIdx.x) * COUT * P;
    // A thread of the plane-wise passes (fill, exact branch, stores) keeps ONE board position and walks over the channels,
    // TPP planes per pass: consecutive threads touch consecutive addresses of global memory.
    const int walker_p = tid % P;
    const int walker_c = tid / P;

    // ---- zero the buffer (borders, padding channels), then the board as h0 = fp16(8 x), h1 = fp16(8 x - h0) ---------------
    {
        const int bytes = kWidePP * 2 * CPH * 2;         // a multiple of 16
        float4* z = reinterpret_cast<float4*>(hl);
        for (int i = tid; i < bytes / 16; i += THREADS) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    int out_of_range = 0;
    if (tid < WALKERS) {
        const int at_p = wide_plane_pos(walker_p) * 2 * CPH;
        for (int c0 = walker_c; c0 < cin; c0 += 4 * TPP) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ci = c0 + k * TPP;
                v[k] = ci < cin ? xb[ci * P + walker_p] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ci = c0 + k * TPP;
                if (ci < cin) {
                    out_of_range |= !wide_in_range(v[k]);
                    const float vs = v[k] * kWideActScale;
                    const _Float16 h0 = static_cast<_Float16>(vs);
                    hl[at_p + ci] = h0;
                    hl[at_p + CPH + ci] = static_cast<_Float16>(vs - static_cast<float>(h0));
                }
            }
        }
    }
    const int exact = __syncthreads_or(out_of_range);   // (also the barrier between the fill and the main loop)

    if (exact) {
        // ---- the board left the two-halves form's range: plain fp32, the arithmetic of a scalar loop -----------------------
        if (tid == 0 && exact_boards) atomicAdd(exact_boards, 1);
        if (tid < WALKERS) {
            const int y = walker_p / kWideW, xx = walker_p % kWideW;
            for (int n = walker_c; n < COUT; n += TPP) {
                const float* wn = weight + static_cast<size_t>(n) * cin * 9;
                float acc = 0.f;
                for (int tap = 0; tap < 9; ++tap) {
                    const int ys = y + tap / 3 - 1, xs = xx + tap % 3 - 1;
                    const bool inside = ys >= 0 && ys < kWideH && xs >= 0 && xs < kWideW;
                    const float* src = xb + (inside ? ys * kWideW + xs : 0);
                    for (int ci = 0; ci < cin; ++ci)
                        acc = __builtin_fmaf(wn[ci * 9 + tap], inside ? src[ci * P] : 0.f, acc);
                }
                float v = acc * scale[n] + shift[n];
                if (residual) v = v + residual[g0 + n * P + walker_p];
                if (relu) v = v < 0.f ? 0.f : v;         // (a NaN stays a NaN, as torch.relu keeps it)
                out[g0 + n * P + walker_p] = v;
            }
        }
        return;
    }

    // ---- per-lane row addresses ----------------------------------------------------------------------------------------
    const int col_pair = wave & 3;                      // output channels col_pair * 32 .. + 31
    const int row_group = wave >> 2;
    const int i_row = lane & 15;
    const int kk = lane >> 4;
    int pos_a[MTW];
#pragma unroll
    for (int t = 0; t < MTW; ++t) pos_a[t] = wide_row_pos((row_group + t * RG) * 16 + i_row);

    f32x4 hi[MTW][2], lo[MTW][2];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) hi[t][c] = lo[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop: 9 taps x ng groups of 32 channels.  The products are issued as W x X^T (weights as the MFMA's first
    //      operand): a lane's four D values are four consecutive output channels (4 kk + r of its column tile) of one
    //      position (i_row of its row tile).  Two register sets (operands of an even / an odd iteration), each refilled
    //      for iteration + 2 right after its MFMAs have issued: LDS reads and weight loads stay one iteration ahead.
    const int iterations = 9 * ng;
    const h8* wlane = reinterpret_cast<const h8*>(wh) + kk * COUT + col_pair * 32 + i_row;
    auto wload = [&](int it, int c, int q) { return wlane[(static_cast<size_t>(it) * 2 + q) * 4 * COUT + 16 * c]; };
    int grp = 0, tap = 0;                               // the (tap, group) of the NEXT A fetch
    auto advance = [&]() {
        if (++grp == ng) {
            grp = 0;
            tap = tap < 8 ? tap + 1 : 8;                // (fetches past the last iteration re-read the last tap: unused)
        }
    };
    h8 a_even[MTW][2], a_odd[MTW][2], w_even[2][2], w_odd[2][2];
    auto fetch_a = [&](h8 (&a)[MTW][2]) {
        const int off = wide_tap_offset(tap) * 2 * CPH + grp * kWideGroup + 8 * kk;
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int q = 0; q < 2; ++q) a[t][q] = reinterpret_cast<const h8*>(hl)[(pos_a[t] * 2 * CPH + q * CPH + off) >> 3];
        advance();
    };
    auto fetch_b = [&](h8 (&b)[2][2], int it) {         // (two spare zero groups follow the last iteration's weights)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 2; ++q) b[c][q] = wload(it, c, q);
    };
    auto multiply = [&](const h8 (&a)[MTW][2], const h8 (&b)[2][2]) {
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) hi[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[c][0], a[t][0], hi[t][c], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) lo[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[c][1], a[t][0], lo[t][c], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < MTW; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) lo[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[c][0], a[t][1], lo[t][c], 0, 0, 0);
    };
    fetch_b(w_even, 0);
    fetch_b(w_odd, 1);
    fetch_a(a_even);
    fetch_a(a_odd);
    for (int it = 0; it < iterations; it += 2) {        // (an odd count runs one more iteration on the spare zero weights)
        multiply(a_even, w_even);
        fetch_a(a_even);
        fetch_b(w_even, min(it + 2, iterations + 1));
        multiply(a_odd, w_odd);
        fetch_a(a_odd);
        fetch_b(w_odd, min(it + 3, iterations + 1));
    }

    // ---- epilogue: (hi + lo) / 512 -> LDS tile [channel][position] over the now-free planes -> folded batch norm, skip,
    //      ReLU, NCHW stores with consecutive threads on consecutive addresses ----------------------------------------------
    constexpr float kDescale = 1.0f / (kWideActScale * kWideWtScale);
    float* stage = reinterpret_cast<float*>(hl);
    __syncthreads();                                    // every wavefront has finished reading the planes
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
        const int m = (row_group + t * RG) * 16 + i_row;
        if (m >= P) continue;                           // rows 121 .. 127 of the last tile
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n0 = col_pair * 32 + c * 16 + 4 * kk;
            const f32x4 conv = (hi[t][c] + lo[t][c]) * kDescale;
#pragma unroll
            for (int r = 0; r < 4; ++r) stage[(n0 + r) * LDM + m] = conv[r];
        }
    }
    __syncthreads();
    if (tid < WALKERS) {
        for (int n0 = walker_c; n0 < COUT; n0 += 4 * TPP) {   // COUT = 8 x (4 TPP): no ragged pass
            float skip[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) skip[k] = residual ? residual[g0 + (n0 + k * TPP) * P + walker_p] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int n = n0 + k * TPP;
                float v = stage[n * LDM + walker_p] * scale[n] + shift[n];
                if (residual) v = v + skip[k];
                if (relu) v = v < 0.f ? 0.f : v;         // (a NaN stays a NaN, as torch.relu keeps it)
                out[g0 + n * P + walker_p] = v;
            }
        }
    }
}

}  // namespace mz

extern "C" int mzmcts_board_conv_wide_supported(int32_t cin, int32_t cout, int32_t height, int32_t width) {
    return mz::wide_conv_supported(cin, cout, height, width) ? 1 : 0;
}

extern "C" int64_t mzmcts_board_conv_wide_halfs(int32_t cin, int32_t cout) {
    if (cin <= 0 || cout <= 0) return -1;
    return mz::wide_packed_halfs(cin, cout);
}

extern "C" int mzmcts_board_conv_wide_pack(const float* weight, void* packed, int32_t cin, int32_t cout, void* stream_) {
    if (!weight || !packed || !mz::wide_conv_supported(cin, cout, mz::kWideH, mz::kWideW)) return MZMCTS_ERR_INVALID;
    const int64_t total = mz::wide_packed_halfs(cin, cout);
    mz::wide_conv_pack_kernel<<<dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_)>>>(
        weight, static_cast<_Float16*>(packed), cin, cout);
    return hipGetLastError() == hipSuccess ? MZMCTS_OK : MZMCTS_ERR_HIP;
}

extern "C" int mzmcts_board_conv_wide(const float* x, const void* packed, const float* weight, const float* scale,
                                      const float* shift, const float* residual, float* out, int32_t* exact_boards,
                                      int64_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t relu,
                                      void* stream_) {
    if (!x || !packed || !weight || !scale || !shift || !out || out == x || out == residual ||
        (reinterpret_cast<uintptr_t>(packed) & 15u))    // (a lane reads eight halves at a time)
        return MZMCTS_ERR_INVALID;
    mz::WidePlan p;
    const int rc = mz::plan_wide_conv(batch, cin, cout, height, width, &p);
    if (rc != MZMCTS_OK || batch == 0) return rc;
    return mz::launch_with_lds(mz::wide_conv_split_kernel, dim3(p.grid), dim3(p.block), p.lds, static_cast<hipStream_t>(stream_), x,
                               static_cast<const _Float16*>(packed), weight, scale, shift, residual, out, exact_boards,
                               static_cast<int>(cin), static_cast<int>(relu));
}
