// rescale_train.hip -- the backward of the hidden state's per-plane min-max rescale in training as ONE launch
// (include/mztrain.h mztrain_rescale_*): the rule of csrc/rescale_train.h, whose forward is mzmcts_unit_rescale.
//
//   rescale_backward_kernel  a workgroup of 256 moves its rows of x and of g -- rst::Plan::rows_per_group of them, contiguous
//                            in memory -- into LDS with coalesced loads, a thread then owns a row (rst::row_backward: three
//                            sequential passes over its P floats, the sums in float64) and writes dx over g in LDS, and the
//                            workgroup writes the dx rows out with coalesced stores.
// Rows lie in LDS at an odd stride (rst::row_stride_of), so the row owners of a 32-lane half read 32 different banks.  Rows
// start at multiples of P floats, which need not be 16-byte aligned: every access is one float.  No atomics, nothing to zero,
// every dx entry written by every call; the bits are the host entry's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mztrain.h"
#include "engine_host.h"
#include "rescale_train.h"

namespace {

namespace rst = mz::rst;

// where element i of a group's contiguous rows lives in a tile, kept incrementally: one division per thread
struct TileCursor {
    uint32_t row, col;
};

__device__ inline uint32_t tile_index(const TileCursor& c, uint32_t stride) { return c.row * stride + c.col; }

__device__ inline void tile_advance(TileCursor* c, uint32_t drow, uint32_t dcol, uint32_t row_len) {
    c->row += drow;
    c->col += dcol;
    if (c->col >= row_len) {
        c->col -= row_len;
        c->row += 1;
    }
}

__global__ __launch_bounds__(rst::kBlock) void rescale_backward_kernel(const float* x, const float* g, float* dx, uint32_t rows,
                                                                       uint32_t row_len, uint32_t rows_per_group,
                                                                       uint32_t stride) {
    extern __shared__ float tile[];                     // x rows [rows_per_group][stride] | g rows, later dx rows, likewise
    float* tile_x = tile;
    float* tile_g = tile + rows_per_group * stride;
    const uint32_t first_row = blockIdx.x * rows_per_group;
    const uint32_t n_rows = min(rows_per_group, rows - first_row);
    const size_t base = static_cast<size_t>(first_row) * row_len;
    const uint32_t n = n_rows * row_len;
    const uint32_t drow = rst::kBlock / row_len, dcol = rst::kBlock % row_len;
    const TileCursor first{threadIdx.x / row_len, threadIdx.x % row_len};

    TileCursor at = first;
    for (uint32_t i = threadIdx.x; i < n; i += rst::kBlock) {
        const uint32_t slot = tile_index(at, stride);
        tile_x[slot] = x[base + i];
        tile_g[slot] = g[base + i];
        tile_advance(&at, drow, dcol, row_len);
    }
    __syncthreads();
    if (threadIdx.x < n_rows) {
        const uint32_t row = threadIdx.x * stride;
        rst::row_backward(tile_x + row, tile_g + row, tile_g + row, static_cast<int>(row_len));
    }
    __syncthreads();
    at = first;
    for (uint32_t i = threadIdx.x; i < n; i += rst::kBlock) {
        dx[base + i] = tile_g[tile_index(at, stride)];
        tile_advance(&at, drow, dcol, row_len);
    }
}

int refuse(const char* entry, const std::string& msg) {
    return fail(nullptr, MZMCTS_ERR_INVALID, std::string(entry) + ": " + msg);
}

int check_args(const char* entry, const mztrain_rescale_backward_args* a) {
    if (!a) return refuse(entry, "null args");
    if (!a->x || !a->grad_out || !a->grad_x) return refuse(entry, "null pointer in args");
    if (const char* why = rst::refusal(a->rows, a->row_len)) return refuse(entry, why);
    return MZMCTS_OK;
}

}  // namespace

extern "C" {

int mztrain_rescale_supported(int64_t rows, int32_t row_len) {
    const char* why = rst::refusal(rows, row_len);
    if (why) refuse("mztrain_rescale_supported", why);
    return why ? 0 : 1;
}

int mztrain_rescale_backward_plan(int64_t rows, int32_t row_len, int64_t* out) {
    if (!out) return refuse("mztrain_rescale_backward_plan", "null out");
    for (int i = 0; i < 5; ++i) out[i] = 0;
    rst::Plan plan;
    if (!rst::plan_rescale_backward(rows, row_len, &plan)) return refuse("mztrain_rescale_backward_plan", rst::refusal(rows, row_len));
    out[0] = plan.grid, out[1] = plan.block, out[2] = plan.rows_per_group, out[3] = plan.row_stride;
    out[4] = static_cast<int64_t>(plan.lds);
    return MZMCTS_OK;
}

int mztrain_rescale_backward(const mztrain_rescale_backward_args* a, void* stream_) {
    const int rc = check_args("mztrain_rescale_backward", a);
    if (rc != MZMCTS_OK) return rc;
    rst::Plan plan;
    rst::plan_rescale_backward(a->rows, a->row_len, &plan);
    if (plan.lds > 64 * 1024)
        MZ_HIP(nullptr, hipFuncSetAttribute(reinterpret_cast<const void*>(rescale_backward_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(plan.lds)));
    rescale_backward_kernel<<<dim3(plan.grid), dim3(plan.block), plan.lds, static_cast<hipStream_t>(stream_)>>>(
        a->x, a->grad_out, a->grad_x, static_cast<uint32_t>(a->rows), static_cast<uint32_t>(a->row_len),
        static_cast<uint32_t>(plan.rows_per_group), static_cast<uint32_t>(plan.row_stride));
    MZ_HIP(nullptr, hipGetLastError());
    return MZMCTS_OK;
}

int mztrain_rescale_reference_backward(const mztrain_rescale_backward_args* a) {
    const int rc = check_args("mztrain_rescale_reference_backward", a);
    if (rc != MZMCTS_OK) return rc;
    rst::reference_backward(a->x, a->grad_out, a->grad_x, a->rows, a->row_len);
    return MZMCTS_OK;
}

}  // extern "C"
