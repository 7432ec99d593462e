// board_launch.h -- the launch step board_conv.hip and net_kernels.hip share (HIP side; the decisions are launch_plan.h's).
#pragma once
#include <hip/hip_runtime.h>

#include "launch_plan.h"

namespace mz {

// Raises the kernel's dynamic LDS limit where the launch asks for more than the 64 KB every kernel may have, launches,
// and reports the launch error.
template <typename... Params, typename... Args>
inline int launch_with_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
    if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds)) != hipSuccess)
        return MZMCTS_ERR_HIP;
    kernel<<<grid, block, lds, stream>>>(args...);
    return hipGetLastError() == hipSuccess ? MZMCTS_OK : MZMCTS_ERR_HIP;
}

}  // namespace mz
