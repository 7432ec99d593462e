// grad_fold.h -- the weight gradients of one residual training step folded and the optimizer applied (include/mztrain.h
// mztrain_fold_*), written once for the HIP kernel of grad_fold.hip and for a host compiler (mztrain_fold_reference,
// tests/grad_fold_check.cpp).  No HIP include; built with -ffp-contract=off like everything else.
//
// A segment is one parameter tensor: `count` floats at `offset` of the flat weight / moment / gradient buffers.  Every use of
// the parameter in a step wrote its weight gradient into a slot of the staging buffer; slot s of a segment starts at
// slot_base + s * slot_stride.  Per element i of a segment with uses >= 1, float32:
//   g = slot[0][i];  g = g + slot[s][i] for s = 1 .. uses - 1, ascending        (autograd's AccumulateGrad order)
//   grads[offset + i] = g
//   w, m, v updated by fc_optimizer.h's adam_element / sgd_element               (the functions mztrain_opt_step calls)
// A segment with uses == 0 is left alone (weights, moments, gradient): torch skips a parameter whose grad is None.  Slots at
// index uses or above are never read; floats of the flat buffers outside every segment are never written.
//
// The launch plan is here too (launch_plan.h's way): segments are cut into chunks of kChunk floats, a chunk lies within one
// segment, a workgroup of kThreads walks chunks grid-stride, at most kMaxBlocks workgroups.
#pragma once
#include <cstdint>

#include "fc_optimizer.h"

namespace mz {
namespace gfold {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kChunk = 4 * kThreads;      // floats of a chunk: one float4 per thread
constexpr int kSlotAlign = 128;           // floats (512 bytes): what the trainer rounds slot_stride up to

struct Segment {                          // the layout of mztrain_fold_segment
    int64_t offset, count, slot_base, slot_stride;
    int32_t capacity, reserved;
};

struct Chunk {
    int64_t first;                        // first element of the chunk within its segment, a multiple of kChunk
    int32_t segment;
    int32_t count;                        // 1 .. kChunk
};

MZ_HD inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
MZ_HD inline int64_t segment_chunks(int64_t count) { return (count + kChunk - 1) / kChunk; }

// whether a segment's chunks may move 16 bytes per lane, given that every base pointer is 16-byte aligned
MZ_HD inline bool segment_vector(const Segment& s) { return s.offset % 4 == 0 && s.slot_base % 4 == 0 && s.slot_stride % 4 == 0; }

// ---- refusals decided on the segment list alone: nullptr, or what is wrong (`*at`: the segment) ----------------------------
inline const char* check_segments(const Segment* seg, int32_t n_segments, int64_t n, int64_t staging_floats, int32_t* at) {
    *at = -1;
    if (!seg) return "null segments";
    if (n_segments <= 0) return "n_segments must be positive";
    if (n <= 0 || staging_floats <= 0) return "n and staging_floats must be positive";
    for (int32_t k = 0; k < n_segments; ++k) {
        const Segment& s = seg[k];
        *at = k;
        if (s.count <= 0) return "a segment's count must be positive";
        if (s.offset < 0 || s.offset > n || s.count > n - s.offset) return "a segment lies outside the flat buffer";
        if (s.slot_stride < s.count) return "slot_stride below count";
        if (s.slot_stride % 4 != 0) return "slot_stride must be a multiple of 4";
        if (s.capacity < 1) return "a segment's capacity must be positive";
        if (s.slot_base < 0 || s.slot_base > staging_floats) return "a segment's slots lie outside the staging buffer";
        const int64_t room = staging_floats - s.slot_base;                // slots [0, capacity): the last one ends at count
        if (s.count > room || (s.capacity - 1) > (room - s.count) / s.slot_stride)
            return "a segment's slots lie outside the staging buffer";
    }
    // overlap in the flat buffer: n_segments is a network's tensor count, the quadratic walk is nothing
    for (int32_t a = 0; a < n_segments; ++a)
        for (int32_t b = a + 1; b < n_segments; ++b)
            if (seg[a].offset < seg[b].offset + seg[b].count && seg[b].offset < seg[a].offset + seg[a].count) {
                *at = b;
                return "a segment overlaps another";
            }
    *at = -1;
    return nullptr;
}

inline const char* check_uses(const Segment* seg, const int32_t* uses, int32_t n_segments, int32_t* at) {
    *at = -1;
    if (!uses) return "null uses";
    for (int32_t k = 0; k < n_segments; ++k)
        if (uses[k] < 0 || uses[k] > seg[k].capacity) {
            *at = k;
            return "uses outside [0, capacity]";
        }
    return nullptr;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------
struct FoldPlan {
    int64_t chunks;
    unsigned grid, block;
};

inline FoldPlan plan_fold(const Segment* seg, int32_t n_segments) {
    FoldPlan p{};
    for (int32_t k = 0; k < n_segments; ++k) p.chunks += segment_chunks(seg[k].count);
    p.block = kThreads;
    p.grid = static_cast<unsigned>(p.chunks < kMaxBlocks ? p.chunks : kMaxBlocks);
    return p;
}

// `out` holds plan_fold(...).chunks entries: segment by segment, ascending within a segment
inline void fill_chunks(const Segment* seg, int32_t n_segments, Chunk* out) {
    int64_t c = 0;
    for (int32_t k = 0; k < n_segments; ++k)
        for (int64_t first = 0; first < seg[k].count; first += kChunk) {
            const int64_t left = seg[k].count - first;
            out[c++] = Chunk{first, k, static_cast<int32_t>(left < kChunk ? left : kChunk)};
        }
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------
// `slot0` points at element i of slot 0; plain float32 additions in ascending slot order
MZ_HD inline float fold_slots(const float* slot0, int64_t slot_stride, int32_t uses) {
    float g = slot0[0];
    for (int32_t s = 1; s < uses; ++s) g = g + slot0[s * slot_stride];
    return g;
}

// the update of one element by the folded gradient g; `m` null: SGD without a buffer; `v` null for SGD
template <int kKind>
MZ_HD inline void apply_element(const fco::Step& s, float g, float* w, float* m, float* v) {
    if (kKind == fco::kAdam)
        fco::adam_element(s, g, w, m, v);
    else
        fco::sgd_element(s, g, w, m);
}

// One whole step on arrays the caller can index: what mztrain_fold_reference runs on host arrays.
inline void reference_step(int kind, const Segment* seg, const int32_t* uses, int32_t n_segments, const float* staging,
                           float* weights, float* grads, float* moment1, float* moment2, double lr, int64_t t, double beta1,
                           double beta2, double eps, double weight_decay, double momentum) {
    const fco::Step st = fco::make_step(kind, lr, t, beta1, beta2, eps, weight_decay, momentum);
    const bool with_buffer = momentum != 0.0;
    for (int32_t k = 0; k < n_segments; ++k) {
        const Segment& s = seg[k];
        if (uses[k] == 0) continue;
        for (int64_t i = 0; i < s.count; ++i) {
            const float g = fold_slots(staging + s.slot_base + i, s.slot_stride, uses[k]);
            const int64_t at = s.offset + i;
            grads[at] = g;
            if (kind == fco::kAdam)
                apply_element<fco::kAdam>(st, g, weights + at, moment1 + at, moment2 + at);
            else
                apply_element<fco::kSgd>(st, g, weights + at, with_buffer ? moment1 + at : nullptr, nullptr);
        }
    }
}

}  // namespace gfold
}  // namespace mz
