// obs_stack.h -- the index rule of a stacked observation and the slot arithmetic of the per-env frame ring.
//
// GameHistory.get_stacked_observations(-1, n) (reference self_play.py:514-548) is the current frame (C planes) followed
// by the n previous frames, newest first; previous frame k (k = 0 the newest) is its C planes and one constant plane
// holding the action played FROM it (action_history[past + 1]); positions before the game's start are zeros.  Per env
// that is  C * HW  +  n * (C + 1) * HW  floats.
//
// The ring keeps, per env, n slots of (C + 1) * HW floats -- a frame with its action plane already filled -- a head
// (the slot of the newest frame) and a count (frames held, saturating at n).  Host and device compile this text:
// obs_stack.hip runs it one thread per output float, tests/obs_stack_check.cpp drives a host ring through it with g++.
// No HIP include.
#pragma once
#include <cstdint>

#ifndef MZ_HD
#if defined(__HIPCC__)
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {

struct StackShape {
    int32_t cur_floats;    // C * HW: the current frame
    int32_t plane_floats;  // HW
    int32_t n;             // previous frames in a stacked observation = slots of the ring
};

MZ_HD inline int32_t stack_frame_floats(const StackShape& s) { return s.cur_floats + s.plane_floats; }  // (C + 1) * HW
MZ_HD inline int64_t stack_floats(const StackShape& s) {
    return static_cast<int64_t>(s.cur_floats) + static_cast<int64_t>(s.n) * stack_frame_floats(s);
}

// ---- the ring ---------------------------------------------------------------------------------------------------------
// slot of the frame k steps back from the newest (k < count <= n)
MZ_HD inline int32_t stack_slot(int32_t head, int32_t k, int32_t n) {
    const int32_t s = head - k;
    return s < 0 ? s + n : s;
}
// where a push writes: the slot after the head, which holds the OLDEST frame once the ring is full
MZ_HD inline int32_t stack_push_slot(int32_t head, int32_t n) { return head + 1 == n ? 0 : head + 1; }
MZ_HD inline int32_t stack_count_after_push(int32_t count, int32_t n) { return count < n ? count + 1 : n; }

// ---- where float t of a stacked observation comes from ------------------------------------------------------------------
enum StackSourceKind : int32_t {
    kStackCurrent = 0,  // the current frame, float `offset`
    kStackFrame = 1,    // previous frame k, float `offset` of its C planes (channel offset / HW, pixel offset % HW)
    kStackAction = 2,   // previous frame k, its action plane, pixel `offset`
    kStackZero = 3,     // before the game's start (k >= count)
};

struct StackSource {
    int32_t kind;
    int32_t k;       // which previous frame (0 = newest); 0 for kStackCurrent
    int32_t offset;  // see the kinds
};

// `count`: previous frames the env holds (0 .. n)
MZ_HD inline StackSource stack_source(int32_t t, const StackShape& s, int32_t count) {
    if (t < s.cur_floats) return StackSource{kStackCurrent, 0, t};
    const int32_t u = t - s.cur_floats, frame = stack_frame_floats(s);
    const int32_t k = u / frame, r = u - k * frame;
    if (k >= count) return StackSource{kStackZero, k, 0};
    if (r < s.cur_floats) return StackSource{kStackFrame, k, r};
    return StackSource{kStackAction, k, r - s.cur_floats};
}

// offset of a source inside a ring slot (the slot stores the C planes, then the filled action plane)
MZ_HD inline int32_t stack_slot_offset(const StackSource& src, const StackShape& s) {
    return src.kind == kStackAction ? s.cur_floats + src.offset : src.offset;
}

// ---- one self-play move of an env ---------------------------------------------------------------------------------------
// What a move does to an env's ring: action < 0 = the env was left untouched (nothing changes); otherwise done != 0 =
// the game is over (the env forgets its frames); otherwise the frame the move was played from is pushed.
enum StackMove : int32_t { kStackUntouched = 0, kStackCleared = 1, kStackPushed = 2 };

MZ_HD inline int32_t stack_move(int32_t action, int32_t done) {
    return action < 0 ? kStackUntouched : (done ? kStackCleared : kStackPushed);
}

struct StackState {
    int32_t head, count;
};

MZ_HD inline StackState stack_after(const StackState& before, int32_t move, int32_t n) {
    if (move == kStackCleared) return StackState{0, 0};
    if (move == kStackPushed) return StackState{stack_push_slot(before.head, n), stack_count_after_push(before.count, n)};
    return before;
}

// The stacked observation AFTER the move, expressed in the ring as it stood BEFORE the move, so that a launch that
// pushes and emits at once reads nothing it writes: after a push frame 0 is the (frame, action) being pushed -- taken
// from the move's own inputs (`fresh` set) -- and frame k >= 1 is the old frame k - 1; the slot the push overwrites held
// the old frame n - 1, which would be frame n of the new window: outside it.
struct StackMoveSource {
    StackSource src;  // kind / offset as above; for a ring read `slot` is the slot to read
    int32_t slot;     // valid for kStackFrame / kStackAction with fresh == 0
    int32_t fresh;    // 1: previous frame 0 is the frame being pushed (obs_before / float(action)), not a ring slot
};

MZ_HD inline StackMoveSource stack_move_source(int32_t t, const StackShape& s, const StackState& before, int32_t move) {
    const int32_t pushed = move == kStackPushed ? 1 : 0;
    const int32_t held = move == kStackCleared ? 0 : before.count;  // old frames still in the window's reach
    StackMoveSource out{stack_source(t, s, held + pushed), 0, 0};
    if (out.src.kind == kStackFrame || out.src.kind == kStackAction) {
        if (pushed && out.src.k == 0)
            out.fresh = 1;
        else  // (k < n and k - pushed < held <= n: with a full ring and a push the oldest frame is never asked for)
            out.slot = stack_slot(before.head, out.src.k - pushed, s.n);
    }
    return out;
}

}  // namespace mz
