// conv_train.hip -- the 3 x 3 convolutions of a residual network in training as HIP launches (include/mztrain.h
// mztrain_conv_*): the rule and the order of every sum of csrc/conv_train.h.
//
//   conv_train_pack_kernel   the forward packing, the data-gradient packing (the transposed, flipped weight) and the ones |
//                            zeros pair of the raw epilogue in one launch, into caller-owned buffers
//   forward, data gradient   mzmcts_board_conv3x3 (board_conv.hip) on those packings: no convolution kernel of their own
//   conv_wgrad_kernel        dw as a GEMM [cout] x [cin * 9] over k = (sample, position) on v_mfma_f32_16x16x4_f32: a
//                            workgroup of 16 wavefronts owns one 16 x 16 tile of dw and walks the whole reduction, a
//                            wavefront per slice of 64 indices (16 MFMAs from a zero accumulator, both operands straight
//                            from global memory, border taps and the ragged last slice predicated to zero); after every
//                            round of 16 slices thread t < 256 adds the 16 slice sums of its entry, in ascending slice
//                            order, to its float64 total.  No atomics, no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "conv_train.h"
#include "engine_host.h"

namespace {

namespace cvt = mz::cvt;

typedef float f32x4 __attribute__((ext_vector_type(4)));

static_assert(cvt::kSlice == MZTRAIN_CONV_SLICE, "mztrain.h states the slice length");
static_assert(cvt::kAffine == MZTRAIN_CONV_AFFINE, "mztrain.h states the size of the ones | zeros pair");
static_assert(cvt::kSlice == 64, "a slice is 16 MFMAs of 4 indices");

__global__ __launch_bounds__(256) void conv_train_pack_kernel(const float* __restrict__ w, float* __restrict__ packed,
                                                              float* __restrict__ packed_dx, float* __restrict__ affine,
                                                              int cin, int cout, int dx_planes) {
    const int n_fwd = mz::conv_packed_floats(cin, cout);
    const int n_dx = dx_planes > 0 ? mz::conv_packed_floats(cout, dx_planes) : 0;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_fwd) {
        packed[i] = cvt::pack_forward_value(w, cin, cout, i);
        return;
    }
    i -= n_fwd;
    if (i < n_dx) {
        packed_dx[i] = cvt::pack_dgrad_value(w, cin, cout, dx_planes, i);
        return;
    }
    i -= n_dx;
    if (i < 2 * cvt::kAffine) affine[i] = i < cvt::kAffine ? 1.f : 0.f;
}

template <int H, int W>
__global__ __launch_bounds__(64 * cvt::kWgradWaves) void conv_wgrad_kernel(const float* __restrict__ x,
                                                                           const float* __restrict__ dy,
                                                                           float* __restrict__ dw, int batch, int cin,
                                                                           int cout) {
    constexpr int P = H * W;
    constexpr int STEPS = cvt::kSlice / 4;
    __shared__ float part[cvt::kWgradWaves][256];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int i = lane & 15;                            // A: row (output channel) of the tile; B: its column (ci, tap)
    const int kk = lane >> 4;                           // the lane's reduction index within an MFMA
    const int m_tiles = cout / 16;
    const int m_tile = blockIdx.x % m_tiles, n_tile = blockIdx.x / m_tiles;
    const int columns = cin * 9;
    const int co = m_tile * 16 + i;
    const int n = n_tile * 16 + i;
    const bool n_ok = n < columns;
    const int ci = n_ok ? n / 9 : 0;
    const int tap = n_ok ? n % 9 : 4;
    const int oy = tap / 3 - 1, ox = tap % 3 - 1;
    const int K = batch * P;
    const int slices = (K + cvt::kSlice - 1) / cvt::kSlice;

    double total = 0.0;
    for (int s0 = 0; s0 < slices; s0 += cvt::kWgradWaves) {
        const int slice = s0 + wave;                    // uniform in a wavefront
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if (slice < slices) {
            const int k0 = slice * cvt::kSlice + kk;
            float a[STEPS], v[STEPS];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {           // every load of the slice is asked for before the first MFMA
                const int k = k0 + 4 * s;
                const bool k_ok = k < K;
                const int b = k / P, p = k % P;
                const int yy = p / W + oy, xx = p % W + ox;
                const bool inside = k_ok && n_ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
                // 32-bit offsets (the plan keeps batch * P * channels within int32; unsigned: an index past K is formed, not read)
                a[s] = k_ok ? dy[(static_cast<unsigned>(b) * cout + co) * P + p] : 0.f;
                v[s] = inside ? x[(static_cast<unsigned>(b) * cin + ci) * P + yy * W + xx] : 0.f;
            }
#pragma unroll
            for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][(4 * kk + r) * 16 + i] = acc[r];   // D[row = 4 (lane >> 4) + r][col = lane & 15]
        __syncthreads();
        if (tid < 256) {
#pragma unroll
            for (int w = 0; w < cvt::kWgradWaves; ++w)
                if (s0 + w < slices) total = total + static_cast<double>(part[w][tid]);
        }
        __syncthreads();
    }
    if (tid < 256) {
        const int row = tid >> 4, col = n_tile * 16 + (tid & 15);
        if (col < columns) dw[static_cast<size_t>(m_tile * 16 + row) * columns + col] = static_cast<float>(total);
    }
}

int refuse(const char* entry, const std::string& msg) {
    return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg);
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int check_pack(const char* entry, const mztrain_conv_pack_args* a) {
    if (!a) return refuse(entry, "null args");
    if (!a->weight || !a->packed || !a->affine) return refuse(entry, "null pointer in args (packed_dx alone may be null)");
    if (a->cin < 1 || a->cin > 80 || (a->cout != 16 && a->cout != 64))
        return refuse(entry, "cin must lie in [1, 80] and cout must be 16 or 64");
    if (a->dx_planes < 0 || !cvt::dx_planes_ok(a->cin, a->dx_planes))
        return refuse(entry, "dx_planes must be 0, 16 or 64 and at most cin");
    if (a->dx_planes > 0 && !a->packed_dx) return refuse(entry, "dx_planes > 0 needs packed_dx");
    return MZMCTS_OK;
}

int check_shape(const char* entry, int64_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width) {
    if (!cvt::conv_launchable(cin, cout, height, width))
        return refuse(entry, "unsupported shape (boards 3 x 3, 6 x 6, 6 x 7; cout 16 or 64; 1 <= cin <= 80, and with cout 16 "
                             "at most 48, 32 or 64 by the board)");
    if (batch < 1 || batch > cvt::wgrad_max_batch(cin, cout, height, width))
        return refuse(entry, "batch must be positive and batch * H * W * max(cin, cout) must stay within int32");
    return MZMCTS_OK;
}

int check_forward(const char* entry, const mztrain_conv_forward_args* a, bool device) {
    if (!a) return refuse(entry, "null args");
    if (!a->x || !a->y || (device ? (!a->packed || !a->affine) : !a->weight))
        return refuse(entry, device ? "null x, packed, affine or y" : "null x, weight or y");
    if (a->x == a->y) return refuse(entry, "y must not be x");
    if (device && (!aligned16(a->x) || !aligned16(a->y) || !aligned16(a->packed)))
        return refuse(entry, "x, y and packed must be 16-byte aligned");
    return check_shape(entry, a->batch, a->cin, a->cout, a->height, a->width);
}

int check_dgrad(const char* entry, const mztrain_conv_dgrad_args* a, bool device) {
    if (!a) return refuse(entry, "null args");
    if (!a->dy || !a->dx || (device ? (!a->packed_dx || !a->affine) : !a->weight))
        return refuse(entry, device ? "null dy, packed_dx, affine or dx" : "null dy, weight or dx");
    if (a->dy == a->dx) return refuse(entry, "dx must not be dy");
    if (device && (!aligned16(a->dy) || !aligned16(a->dx) || !aligned16(a->packed_dx)))
        return refuse(entry, "dy, dx and packed_dx must be 16-byte aligned");
    const int rc = check_shape(entry, a->batch, a->cin, a->cout, a->height, a->width);
    if (rc != MZMCTS_OK) return rc;
    if (a->dx_planes < 1 || !cvt::dx_planes_ok(a->cin, a->dx_planes))
        return refuse(entry, "dx_planes must be 16 or 64 and at most cin");
    if (!cvt::conv_launchable(a->cout, a->dx_planes, a->height, a->width))
        return refuse(entry, "unsupported shape of the data gradient (the convolution cout -> dx_planes on this board)");
    return MZMCTS_OK;
}

int check_wgrad(const char* entry, const mztrain_conv_wgrad_args* a) {
    if (!a) return refuse(entry, "null args");
    if (!a->x || !a->dy || !a->dw) return refuse(entry, "null pointer in args");
    return check_shape(entry, a->batch, a->cin, a->cout, a->height, a->width);
}

}  // namespace

extern "C" {

int mztrain_conv_supported(int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t need_dx_planes) {
    return cvt::conv_supported(cin, cout, height, width, need_dx_planes) ? 1 : 0;
}

int32_t mztrain_conv_slice(void) { return cvt::kSlice; }

int64_t mztrain_conv_max_batch(int32_t cin, int32_t cout, int32_t height, int32_t width) {
    if (!cvt::conv_launchable(cin, cout, height, width)) return -1;
    return cvt::wgrad_max_batch(cin, cout, height, width);
}

int mztrain_conv_wgrad_plan(int64_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int64_t* out) {
    cvt::WgradPlan p;
    const int rc = cvt::plan_conv_wgrad(batch, cin, cout, height, width, &p);
    if (out) {
        out[0] = p.grid, out[1] = p.block, out[2] = static_cast<int64_t>(p.lds), out[3] = p.slices, out[4] = p.rounds;
    }
    return rc;
}

int mztrain_conv_pack(const mztrain_conv_pack_args* a, void* stream_) {
    const int rc = check_pack("mztrain_conv_pack", a);
    if (rc != MZMCTS_OK) return rc;
    const int total = mz::conv_packed_floats(a->cin, a->cout) +
                      (a->dx_planes > 0 ? mz::conv_packed_floats(a->cout, a->dx_planes) : 0) + 2 * cvt::kAffine;
    conv_train_pack_kernel<<<dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_)>>>(
        a->weight, a->packed, a->packed_dx, a->affine, a->cin, a->cout, a->dx_planes);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_conv_forward(const mztrain_conv_forward_args* a, void* stream) {
    const int rc = check_forward("mztrain_conv_forward", a, true);
    if (rc != MZMCTS_OK) return rc;
    return mzmcts_board_conv3x3(a->x, a->packed, a->affine, a->affine + cvt::kAffine, nullptr, a->y, a->batch, a->cin, a->cout,
                                a->height, a->width, 0, stream);
}

int mztrain_conv_dgrad(const mztrain_conv_dgrad_args* a, void* stream) {
    const int rc = check_dgrad("mztrain_conv_dgrad", a, true);
    if (rc != MZMCTS_OK) return rc;
    return mzmcts_board_conv3x3(a->dy, a->packed_dx, a->affine, a->affine + cvt::kAffine, nullptr, a->dx, a->batch, a->cout,
                                a->dx_planes, a->height, a->width, 0, stream);
}

int mztrain_conv_wgrad(const mztrain_conv_wgrad_args* a, void* stream_) {
    int rc = check_wgrad("mztrain_conv_wgrad", a);
    if (rc != MZMCTS_OK) return rc;
    cvt::WgradPlan p;
    rc = cvt::plan_conv_wgrad(a->batch, a->cin, a->cout, a->height, a->width, &p);
    if (rc != MZMCTS_OK) return refuse("mztrain_conv_wgrad", "no launch plan for this shape");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int b = static_cast<int>(a->batch);
    const dim3 grid(p.grid), block(p.block);
    if (p.w == 7)
        conv_wgrad_kernel<6, 7><<<grid, block, 0, stream>>>(a->x, a->dy, a->dw, b, a->cin, a->cout);
    else if (p.h == 6)
        conv_wgrad_kernel<6, 6><<<grid, block, 0, stream>>>(a->x, a->dy, a->dw, b, a->cin, a->cout);
    else
        conv_wgrad_kernel<3, 3><<<grid, block, 0, stream>>>(a->x, a->dy, a->dw, b, a->cin, a->cout);
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_conv_reference_pack(const mztrain_conv_pack_args* a) {
    const int rc = check_pack("mztrain_conv_reference_pack", a);
    if (rc != MZMCTS_OK) return rc;
    const int n_fwd = mz::conv_packed_floats(a->cin, a->cout);
    for (int i = 0; i < n_fwd; ++i) a->packed[i] = cvt::pack_forward_value(a->weight, a->cin, a->cout, i);
    const int n_dx = a->dx_planes > 0 ? mz::conv_packed_floats(a->cout, a->dx_planes) : 0;
    for (int i = 0; i < n_dx; ++i) a->packed_dx[i] = cvt::pack_dgrad_value(a->weight, a->cin, a->cout, a->dx_planes, i);
    for (int i = 0; i < 2 * cvt::kAffine; ++i) a->affine[i] = i < cvt::kAffine ? 1.f : 0.f;
    return MZMCTS_OK;
}

int mztrain_conv_reference_forward(const mztrain_conv_forward_args* a) {
    const int rc = check_forward("mztrain_conv_reference_forward", a, false);
    if (rc != MZMCTS_OK) return rc;
    cvt::reference_forward(a->x, a->weight, a->y, a->batch, a->cin, a->cout, a->height, a->width);
    return MZMCTS_OK;
}

int mztrain_conv_reference_dgrad(const mztrain_conv_dgrad_args* a) {
    const int rc = check_dgrad("mztrain_conv_reference_dgrad", a, false);
    if (rc != MZMCTS_OK) return rc;
    cvt::reference_dgrad(a->dy, a->weight, a->dx, a->batch, a->cin, a->cout, a->height, a->width, a->dx_planes);
    return MZMCTS_OK;
}

int mztrain_conv_reference_wgrad(const mztrain_conv_wgrad_args* a) {
    const int rc = check_wgrad("mztrain_conv_reference_wgrad", a);
    if (rc != MZMCTS_OK) return rc;
    cvt::reference_wgrad(a->x, a->dy, a->dw, a->batch, a->cin, a->cout, a->height, a->width);
    return MZMCTS_OK;
}

}  // extern "C"
