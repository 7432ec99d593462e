// obs_stack.hip -- the device frame stack (include/mzenv.h mzenv_stack_*): per env a ring of the n previous frames, each
// stored with its action plane filled, and the kernel that turns the environment kernels' plain observations into the
// stacked search input of config.stacked_observations = n.  The index rule and the slot arithmetic are csrc/obs_stack.h.
//
// One kernel serves reset and push.  A launch is a copy of E x stack_floats floats: every thread walks its workgroup's
// stretch of the output with consecutive lanes on consecutive floats (4-byte accesses: a TicTacToe frame is 27 floats, a
// SimpleGrid frame 9, so nothing wider is aligned in general), reading whole contiguous frames of the ring.
//
// The two hazards of pushing and emitting in one launch, and how they are designed out:
//  1. Heads and counts.  A workgroup owns WHOLE envs (envs_per_block of them).  Thread i of the group reads the head
//     and count of the group's env i once, keeps the old values in LDS for everybody, and is the only thread of the
//     launch that writes them back.  No thread reads metadata from global memory that another thread writes.
//  2. Frames.  Nothing written by the launch is read by it: after a push, previous frame 0 of the output comes from
//     the move's own inputs (obs_before, actions), frames k >= 1 from the slots of the old frames k - 1, and the slot
//     the push writes is the one after the old head -- free while the ring fills, the oldest frame (old k = n - 1,
//     which the new window no longer contains) once it is full.  obs_stack.h stack_move_source states this once.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mzenv.h"
#include "obs_stack.h"

namespace mz {

constexpr int kStackThreads = 256;
constexpr int kStackMaxEnvsPerBlock = 64;
constexpr int kStackBlockFloats = 16384;  // a workgroup takes fewer envs when their stacked observations are long

struct StackParams {
    StackShape s;
    int32_t E;
    int32_t envs_per_block;  // <= kStackMaxEnvsPerBlock, and envs_per_block * stack_floats fits int32
    float* ring;             // [E][n][(C + 1) * HW]
    int32_t* head;           // [E] slot of the newest frame
    int32_t* count;          // [E] frames held, <= n
};

// is_reset: `flags` is the reset mask (NULL = every env): masked envs are cleared, the others untouched; obs_before and
// actions are not read.  Otherwise `flags` is the move's done array and every env makes stack_move(action, done).
__global__ __launch_bounds__(kStackThreads) void stack_move_kernel(StackParams p, int is_reset, const uint8_t* flags,
                                                                   const float* obs_before, const int32_t* actions,
                                                                   const float* obs_next, float* stacked_out) {
    __shared__ int32_t s_head[kStackMaxEnvsPerBlock], s_count[kStackMaxEnvsPerBlock], s_move[kStackMaxEnvsPerBlock],
        s_action[kStackMaxEnvsPerBlock];
    const int e0 = blockIdx.x * p.envs_per_block;
    const int envs = min(p.envs_per_block, p.E - e0);
    const int tid = threadIdx.x;
    if (tid < envs) {
        const int e = e0 + tid;
        const StackState before{p.head[e], p.count[e]};
        int32_t action = 0, move;
        if (is_reset) {
            move = (!flags || flags[e]) ? kStackCleared : kStackUntouched;
        } else {
            action = actions[e];
            move = stack_move(action, flags[e]);
        }
        s_head[tid] = before.head, s_count[tid] = before.count, s_move[tid] = move, s_action[tid] = action;
        const StackState after = stack_after(before, move, p.s.n);
        p.head[e] = after.head, p.count[e] = after.count;  // (hazard 1: this thread alone touches env e's metadata)
    }
    __syncthreads();
    const int32_t cur = p.s.cur_floats, frame = stack_frame_floats(p.s), n = p.s.n;
    const int32_t width = static_cast<int32_t>(stack_floats(p.s));
    // the frames being pushed go into the ring, action plane filled
    for (int32_t i = tid; i < envs * frame; i += kStackThreads) {
        const int32_t el = i / frame, r = i - el * frame;
        if (s_move[el] != kStackPushed) continue;
        const size_t e = static_cast<size_t>(e0 + el);
        const float v = r < cur ? obs_before[e * cur + r] : static_cast<float>(s_action[el]);
        p.ring[(e * n + stack_push_slot(s_head[el], n)) * frame + r] = v;
    }
    // the stacked observations the next search reads
    for (int32_t i = tid; i < envs * width; i += kStackThreads) {
        const int32_t el = i / width, t = i - el * width;
        const size_t e = static_cast<size_t>(e0 + el);
        const StackMoveSource m = stack_move_source(t, p.s, StackState{s_head[el], s_count[el]}, s_move[el]);
        float v = 0.f;
        if (m.src.kind == kStackCurrent)
            v = obs_next[e * cur + m.src.offset];
        else if (m.src.kind != kStackZero && m.fresh)
            v = m.src.kind == kStackFrame ? obs_before[e * cur + m.src.offset] : static_cast<float>(s_action[el]);
        else if (m.src.kind != kStackZero)
            v = p.ring[(e * n + m.slot) * frame + stack_slot_offset(m.src, p.s)];
        stacked_out[e * width + t] = v;
    }
}

}  // namespace mz

struct mzenv_stack {
    mz::StackParams p{};
    int32_t device = 0;
    std::string error;
};

namespace {
thread_local std::string g_stack_error;
int stack_fail(mzenv_stack* stack, int code, const std::string& msg) {
    if (stack) stack->error = msg;
    g_stack_error = msg;
    return code;
}

int stack_launch(mzenv_stack* stack, int is_reset, const uint8_t* flags, const float* obs_before, const int32_t* actions,
                 const float* obs_next, float* stacked_out, void* stream, const char* what) {
    const mz::StackParams& p = stack->p;
    const unsigned blocks = static_cast<unsigned>((p.E + p.envs_per_block - 1) / p.envs_per_block);
    hipLaunchKernelGGL(mz::stack_move_kernel, dim3(blocks), dim3(mz::kStackThreads), 0, static_cast<hipStream_t>(stream), p,
                       is_reset, flags, obs_before, actions, obs_next, stacked_out);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return stack_fail(stack, -2, std::string(what) + ": " + hipGetErrorString(err));
    return 0;
}
}  // namespace

extern "C" {

const char* mzenv_stack_last_error(const mzenv_stack* stack) { return stack ? stack->error.c_str() : g_stack_error.c_str(); }

int mzenv_stack_create(int32_t num_envs, int32_t channels, int32_t height, int32_t width, int32_t n, int32_t device,
                       mzenv_stack** out) {
    if (!out) return stack_fail(nullptr, -1, "mzenv_stack_create: null output pointer");
    *out = nullptr;
    if (num_envs <= 0 || channels <= 0 || height <= 0 || width <= 0)
        return stack_fail(nullptr, -1, "mzenv_stack_create: envs and observation shape must be positive");
    if (n <= 0) return stack_fail(nullptr, -1, "mzenv_stack_create: a stack holds at least one previous frame (n = 0 needs none)");
    const int64_t hw = static_cast<int64_t>(height) * width;
    const int64_t floats = hw <= INT32_MAX && channels * hw <= INT32_MAX
                               ? channels * hw + static_cast<int64_t>(n) * (channels + 1) * hw
                               : static_cast<int64_t>(INT32_MAX) + 1;
    if (floats > INT32_MAX) return stack_fail(nullptr, -1, "mzenv_stack_create: the stacked observation's float count leaves int32");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return stack_fail(nullptr, -2, "mzenv_stack_create: no HIP device available; the frame stack has no CPU fallback");
    if (device < 0 || device >= n_dev) return stack_fail(nullptr, -1, "mzenv_stack_create: bad device ordinal");
    if (hipSetDevice(device) != hipSuccess) return stack_fail(nullptr, -2, "hipSetDevice failed");
    auto* stack = new mzenv_stack();
    stack->device = device;
    mz::StackParams& p = stack->p;
    p.s = mz::StackShape{static_cast<int32_t>(channels * hw), static_cast<int32_t>(hw), n};
    p.E = num_envs;
    int64_t per_block = mz::kStackBlockFloats / floats;
    per_block = per_block < 1 ? 1 : (per_block > mz::kStackMaxEnvsPerBlock ? mz::kStackMaxEnvsPerBlock : per_block);
    p.envs_per_block = static_cast<int32_t>(per_block);  // (per_block * floats <= max(floats, kStackBlockFloats): int32)
    const size_t ring_bytes = sizeof(float) * static_cast<size_t>(num_envs) * n * mz::stack_frame_floats(p.s);
    const size_t meta_bytes = sizeof(int32_t) * static_cast<size_t>(num_envs);
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.ring), ring_bytes);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p.head), meta_bytes);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p.count), meta_bytes);
    if (err == hipSuccess) err = hipMemset(p.ring, 0, ring_bytes);
    if (err == hipSuccess) err = hipMemset(p.head, 0, meta_bytes);
    if (err == hipSuccess) err = hipMemset(p.count, 0, meta_bytes);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) {
        stack_fail(nullptr, -2, std::string("mzenv_stack_create: ") + hipGetErrorString(err));
        mzenv_stack_destroy(stack);
        return -2;
    }
    *out = stack;
    return 0;
}

void mzenv_stack_destroy(mzenv_stack* stack) {
    if (!stack) return;
    (void)hipSetDevice(stack->device);
    (void)hipDeviceSynchronize();
    if (stack->p.ring) (void)hipFree(stack->p.ring);
    if (stack->p.head) (void)hipFree(stack->p.head);
    if (stack->p.count) (void)hipFree(stack->p.count);
    delete stack;
}

int64_t mzenv_stack_floats(const mzenv_stack* stack) { return stack ? mz::stack_floats(stack->p.s) : -1; }

int mzenv_stack_reset(mzenv_stack* stack, const uint8_t* mask, const float* obs, float* stacked_out, void* stream) {
    // (the arguments are judged before the handle: a wrong call reads the same with or without a device)
    if (!obs || !stacked_out) return stack_fail(stack, -1, "mzenv_stack_reset: null argument");
    if (!stack) return stack_fail(nullptr, -1, "mzenv_stack_reset: null handle");
    return stack_launch(stack, 1, mask, nullptr, nullptr, obs, stacked_out, stream, "mzenv_stack_reset");
}

int mzenv_stack_push(mzenv_stack* stack, const float* obs_before, const int32_t* actions, const uint8_t* done,
                     const float* obs_next, float* stacked_out, void* stream) {
    if (!obs_before || !actions || !done || !obs_next || !stacked_out)
        return stack_fail(stack, -1, "mzenv_stack_push: null argument");
    if (!stack) return stack_fail(nullptr, -1, "mzenv_stack_push: null handle");
    return stack_launch(stack, 0, done, obs_before, actions, obs_next, stacked_out, stream, "mzenv_stack_push");
}

}  // extern "C"
