// staging_layout.h -- the five packed byte blocks the search engine moves between host and GPU: where each field sits (one
// offset chain per block, written here and nowhere else) and typed pointers into a block at any base, the pinned host copy
// or the device copy.  Host-only and free of HIP: tests/staging_layout_check.cpp builds it with g++ and checks every shape.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mz {
struct MinMax;                                // kernel_common.h: two doubles ...
constexpr size_t kMinMaxBytes = 16;           // ... (engine_host.h holds this to the struct)
constexpr size_t round_to(size_t v, size_t step) { return (v + step - 1) / step * step; }
constexpr size_t step256(size_t v) { return round_to(v, 256); }   // the three move-batch blocks place every field, and end, on one
// An address inside a block, as a pointer to whatever element type the field it initialises declares: a field's type is
// written once, in its Block struct below.
struct Carved {
    uint8_t* at;
    template <typename T>
    operator T*() const { return reinterpret_cast<T*>(at); }
};

// ---- per-move upload: what a search is begun with.  No padding but before the doubles.  The noise rows are LAST: a
// search whose noise the host did not draw uploads [0, noise) only.
struct UploadBlock {
    int32_t *legal, *num_legal, *to_play;     // [E][A], [E], [E]
    uint32_t* rng_skip;                       // [E]
    double* noise;                            // [E][A]
};
struct UploadLayout {
    size_t legal = 0, num_legal, to_play, rng_skip, noise, bytes;
    constexpr UploadLayout(size_t E = 0, size_t A = 0)
        : num_legal(4 * E * A), to_play(num_legal + 4 * E), rng_skip(to_play + 4 * E), noise(round_to(rng_skip + 4 * E, 8)),
          bytes(noise + 8 * E * A) {}
    constexpr size_t bytes_no_noise() const { return noise; }
    UploadBlock views(uint8_t* base) const {
        return {Carved{base + legal}, Carved{base + num_legal}, Carved{base + to_play}, Carved{base + rng_skip}, Carved{base + noise}};
    }
};

// ---- per-tree download: what a search leaves for mzmcts_readout.  No padding: the 8-byte fields come first.
struct DownloadBlock {
    double* root_value_sum;                   // [E]
    MinMax* min_max;                          // [E]
    int64_t* depth_sum;                       // [E]
    float* root_predicted;                    // [E]
    int32_t* max_depth;                       // [E]
    uint32_t *tie_words, *noise_words;        // [E], [E]
    int32_t* error_flag;                      // [4]
};
struct DownloadLayout {
    size_t root_value_sum = 0, min_max, depth_sum, root_predicted, max_depth, tie_words, noise_words, error_flag, bytes;
    constexpr DownloadLayout(size_t E = 0)
        : min_max(8 * E), depth_sum(min_max + kMinMaxBytes * E), root_predicted(depth_sum + 8 * E), max_depth(root_predicted + 4 * E),
          tie_words(max_depth + 4 * E), noise_words(tie_words + 4 * E), error_flag(noise_words + 4 * E), bytes(error_flag + 4 * 4) {}
    DownloadBlock views(uint8_t* base) const {
        return {Carved{base + root_value_sum}, Carved{base + min_max}, Carved{base + depth_sum}, Carved{base + root_predicted},
                Carved{base + max_depth}, Carved{base + tie_words}, Carved{base + noise_words}, Carved{base + error_flag}};
    }
};

// ---- move-batch control: one block per batch.  The noise rows are FIRST and everything else follows them as one
// contiguous range [rng_skip, bytes): a batch whose noise is drawn on the device uploads that range in one copy.
struct MoveControlBlock {
    double* noise;                            // [M][E][A]
    uint32_t* rng_skip;                       // [M][E]
    double* temperature;                      // [E]
    int32_t* move_limit;                      // [E]
    uint32_t* expected_ties;                  // [E]
};
struct MoveControlLayout {
    size_t noise = 0, rng_skip, temperature, move_limit, expected_ties, bytes;
    constexpr MoveControlLayout(size_t E = 0, size_t A = 0, size_t M = 0)
        : rng_skip(step256(8 * M * E * A)), temperature(step256(rng_skip + 4 * M * E)), move_limit(step256(temperature + 8 * E)),
          expected_ties(step256(move_limit + 4 * E)), bytes(step256(expected_ties + 4 * E)) {}
    MoveControlBlock views(uint8_t* base) const {
        return {Carved{base + noise}, Carved{base + rng_skip}, Carved{base + temperature}, Carved{base + move_limit}, Carved{base + expected_ties}};
    }
};

// ---- move-batch output ring: one block per move, `stride` bytes apart.
struct MoveOutputBlock {
    int32_t *actions, *visits;                // [E], [E][A]
    double* root_value_sum;                   // [E]
    float* root_predicted;                    // [E]
    int32_t* max_depth;                       // [E]
    uint32_t *tie_words, *sample_words;       // [E], [E]
    int32_t* depth_sum;                       // [E]
};
struct MoveOutputLayout {
    size_t actions = 0, visits, root_value_sum, root_predicted, max_depth, tie_words, sample_words, depth_sum, stride;
    constexpr MoveOutputLayout(size_t E = 0, size_t A = 0)
        : visits(step256(4 * E)), root_value_sum(step256(visits + 4 * E * A)), root_predicted(step256(root_value_sum + 8 * E)),
          max_depth(step256(root_predicted + 4 * E)), tie_words(step256(max_depth + 4 * E)), sample_words(step256(tie_words + 4 * E)),
          depth_sum(step256(sample_words + 4 * E)), stride(step256(depth_sum + 4 * E)) {}
    MoveOutputBlock views(uint8_t* base, size_t move) const {
        base += stride * move;
        return {Carved{base + actions}, Carved{base + visits}, Carved{base + root_value_sum}, Carved{base + root_predicted},
                Carved{base + max_depth}, Carved{base + tie_words}, Carved{base + sample_words}, Carved{base + depth_sum}};
    }
};

// ---- move-batch inputs ring (device-input batches): what each move was searched with, one block per move.
struct MoveInputsBlock {
    int32_t *num_legal, *to_play;             // [E], [E]
    uint32_t* noise_words;                    // [E]
    int32_t* legal;                           // [E][A]
};
struct MoveInputsLayout {
    size_t num_legal = 0, to_play, noise_words, legal, stride;
    constexpr MoveInputsLayout(size_t E = 0, size_t A = 0)
        : to_play(step256(4 * E)), noise_words(step256(to_play + 4 * E)), legal(step256(noise_words + 4 * E)),
          stride(step256(legal + 4 * E * A)) {}
    MoveInputsBlock views(uint8_t* base, size_t move) const {
        base += stride * move;
        return {Carved{base + num_legal}, Carved{base + to_play}, Carved{base + noise_words}, Carved{base + legal}};
    }
};

// the orderings the copies rely on, at a shape with padding in every block (E = 3, A = 3, M = 2)
static_assert(UploadLayout(3, 3).noise == 72 && UploadLayout(3, 3).bytes_no_noise() == 72 && UploadLayout(3, 3).bytes == 144, "noise last, on 8 bytes");
static_assert(DownloadLayout(3).bytes == 3 * (8 + kMinMaxBytes + 8 + 4 * 4) + 16, "download block: no padding");
static_assert(MoveControlLayout(3, 3, 2).noise == 0 && MoveControlLayout(3, 3, 2).rng_skip == 256 && MoveControlLayout(3, 3, 2).bytes == 1280, "noise first");
static_assert(MoveOutputLayout(3, 3).stride == 2048 && MoveInputsLayout(3, 3).stride == 1024, "rings: 256-byte steps");
}  // namespace mz
