// Host check of the phase form of the MT19937 regeneration (csrc/np_legacy_rng.h mt_twist_*), as the narrow kernel's
// rows run it (narrow_device.h mt_regenerate_row): 16 emulated lanes, lane `l` owns the elements begin + 16 t + l of a
// phase; within a phase every lane takes its sources before any lane stores.  Built and run by
// tests/test_mt_twist_cpu.py:
//     g++ -O2 -std=c++17 -I muzero-hypermodel_amd/csrc mt_twist_check.cpp
// argv[1]: file that receives the regenerated blocks, uint32 [34][3][624] (seeds 0..31, the all-zero block, the
// all-ones block; three successive blocks each), for the comparison with numpy's own state.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "np_legacy_rng.h"

namespace {
constexpr int kLanes = 16;

void twist_by_lanes(uint32_t* key, const int* lane_order) {
    constexpr int kPerLane = (mz::kMtTwistPhaseMax + kLanes - 1) / kLanes;
    for (int phase = 0; phase < mz::kMtTwistPhases; ++phase) {
        const int begin = mz::mt_twist_phase_begin(phase), end = mz::mt_twist_phase_end(phase);
        mz::MtTwistSources src[kLanes][kPerLane];
        for (int i = 0; i < kLanes; ++i) {
            const int lane = lane_order[i];
            for (int t = 0; t < kPerLane; ++t) {
                const int k = begin + t * kLanes + lane;
                if (k < end) src[lane][t] = mz::mt_twist_load(key, k);
            }
        }
        for (int i = 0; i < kLanes; ++i) {
            const int lane = lane_order[i];
            for (int t = 0; t < kPerLane; ++t) {
                const int k = begin + t * kLanes + lane;
                if (k < end) key[k] = mz::mt_twist_word(src[lane][t]);
            }
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    int orders[3][kLanes];
    for (int l = 0; l < kLanes; ++l) {
        orders[0][l] = l;
        orders[1][l] = kLanes - 1 - l;
        orders[2][l] = l;
    }
    std::mt19937 shuffle_rng(12345u);
    std::shuffle(orders[2], orders[2] + kLanes, shuffle_rng);

    // every element belongs to exactly one phase, the phases tile the block in order
    int covered = 0;
    bool tiling = mz::mt_twist_phase_begin(0) == 0 && mz::mt_twist_phase_end(mz::kMtTwistPhases - 1) == mz::kMtN;
    for (int phase = 0; phase < mz::kMtTwistPhases; ++phase) {
        const int n = mz::mt_twist_phase_end(phase) - mz::mt_twist_phase_begin(phase);
        tiling = tiling && n > 0 && n <= mz::kMtTwistPhaseMax &&
                 (phase == 0 || mz::mt_twist_phase_begin(phase) == mz::mt_twist_phase_end(phase - 1));
        covered += n;
    }
    tiling = tiling && covered == mz::kMtN;

    std::vector<uint32_t> out;
    long mismatches = 0, blocks = 0;
    for (int input = 0; input < 34; ++input) {
        uint32_t serial[mz::kMtN];
        if (input < 32) {
            int32_t pos;
            mz::mt_seed(serial, &pos, static_cast<uint32_t>(input));
        } else {
            std::memset(serial, input == 32 ? 0x00 : 0xff, sizeof(serial));
        }
        for (int block = 0; block < 3; ++block) {
            uint32_t before[mz::kMtN];
            std::memcpy(before, serial, sizeof(serial));
            mz::mt_regenerate(serial);
            for (int o = 0; o < 3; ++o) {
                uint32_t lanes[mz::kMtN];
                std::memcpy(lanes, before, sizeof(before));
                twist_by_lanes(lanes, orders[o]);
                if (std::memcmp(lanes, serial, sizeof(serial)) != 0) ++mismatches;
                ++blocks;
                if (o == 2) out.insert(out.end(), lanes, lanes + mz::kMtN);
            }
        }
    }
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size()) return 2;
        std::fclose(f);
    }
    std::printf("{\"blocks\": %ld, \"mismatches\": %ld, \"tiling\": %s}\n", blocks, mismatches, tiling ? "true" : "false");
    return mismatches == 0 && tiling ? 0 : 1;
}
