// Host-side run of csrc/obs_stack.h (the text the frame-stack kernel compiles).  One env per run; floats travel as their
// 32-bit patterns in decimal, so every comparison the caller makes is exact.  stdin:
//     C HW n                     the shape; n = 0 is allowed here (no ring: the stacked observation is the frame itself)
//     F f_0 .. f_{C*HW-1}        the first observation: a reset of the env, as mzenv_stack_reset does it
//     P action done f_0 ..       one self-play move, as mzenv_stack_push does it: the frame before is the current one,
//                                f is the observation the next search sees
//     R mask f_0 ..              a masked reset in mid-script (mask 0: the env keeps its frames)
// and after every F / P / R line one line of output: the (C + n (C + 1)) HW floats of the stacked observation.
//
// A move is run the way the kernel may run it in the worst case: the pushed frame is written into the ring FIRST and
// the output is gathered afterwards, through stack_move_source on the state before the move.  The output is gathered a
// second time from a copy of the ring taken before the write; if the two differ, something read what the move wrote
// (exit status 3).
// Built and run by tests/test_obs_stack_cpu.py:   g++ -O2 -std=c++17 obs_stack_check.cpp
// Stand-alone: it can be built once more with -fsanitize=address,undefined and run by hand on the same input.
#include <cstdio>
#include <cstring>
#include <vector>

#include "obs_stack.h"

namespace {
bool read_floats(std::vector<float>& out) {
    for (float& f : out) {
        unsigned bits;
        if (std::scanf("%u", &bits) != 1) return false;
        std::memcpy(&f, &bits, sizeof f);
    }
    return true;
}

void gather(const mz::StackShape& s, const std::vector<float>& ring, const mz::StackState& before, int move,
            const std::vector<float>& obs_before, int action, const std::vector<float>& obs_next, std::vector<float>& out) {
    const int frame = mz::stack_frame_floats(s);
    for (int t = 0; t < static_cast<int>(out.size()); ++t) {
        const mz::StackMoveSource m = mz::stack_move_source(t, s, before, move);
        float v = 0.f;
        if (m.src.kind == mz::kStackCurrent)
            v = obs_next[m.src.offset];
        else if (m.src.kind != mz::kStackZero && m.fresh)
            v = m.src.kind == mz::kStackFrame ? obs_before[m.src.offset] : static_cast<float>(action);
        else if (m.src.kind != mz::kStackZero)
            v = ring.at(static_cast<size_t>(m.slot) * frame + mz::stack_slot_offset(m.src, s));
        out[t] = v;
    }
}
}  // namespace

int main() {
    int C, HW, n;
    if (std::scanf("%d %d %d", &C, &HW, &n) != 3 || C <= 0 || HW <= 0 || n < 0) return 2;
    const mz::StackShape s{C * HW, HW, n};
    const int frame = mz::stack_frame_floats(s);
    std::vector<float> ring(static_cast<size_t>(n) * frame, 0.f), current(s.cur_floats, 0.f), next(s.cur_floats);
    std::vector<float> out(static_cast<size_t>(mz::stack_floats(s))), twin(out.size());
    mz::StackState state{0, 0};
    char kind;
    bool first = true;
    while (std::scanf(" %c", &kind) == 1) {
        int action = 0, move;
        if (kind == 'F' && first) {
            move = mz::kStackCleared;
        } else if (kind == 'P' && !first) {
            int done;
            if (std::scanf("%d %d", &action, &done) != 2) return 2;
            move = mz::stack_move(action, done);
        } else if (kind == 'R' && !first) {
            int mask;
            if (std::scanf("%d", &mask) != 1) return 2;
            move = mask ? mz::kStackCleared : mz::kStackUntouched;
        } else {
            return 2;
        }
        first = false;
        if (!read_floats(next)) return 2;
        const std::vector<float> ring_before = ring;
        if (move == mz::kStackPushed && n > 0) {
            float* slot = &ring.at(static_cast<size_t>(mz::stack_push_slot(state.head, n)) * frame);
            for (int r = 0; r < frame; ++r) slot[r] = r < s.cur_floats ? current[r] : static_cast<float>(action);
        }
        // (n = 0: stack_floats is the frame alone, every float is kStackCurrent and no slot is ever computed)
        gather(s, ring, state, n > 0 ? move : mz::kStackUntouched, current, action, next, out);
        gather(s, ring_before, state, n > 0 ? move : mz::kStackUntouched, current, action, next, twin);
        if (std::memcmp(out.data(), twin.data(), out.size() * sizeof(float)) != 0) return 3;
        if (n > 0) state = mz::stack_after(state, move, n);
        current = next;
        for (float f : out) {
            unsigned bits;
            std::memcpy(&bits, &f, sizeof bits);
            std::printf("%u ", bits);
        }
        std::printf("\n");
    }
    return 0;
}
