// wide_conv_check.cpp -- csrc/wide_conv.h and plan_wide_conv of csrc/launch_plan.h built for the host (g++, no HIP) and
// printed for tests/test_wide_conv_cpu.py, which holds them to a restatement in Python.
//   wide_conv_check geometry           -> one JSON line: constants, row map, tap offsets, plane positions
//   wide_conv_check range  FILE        -> FILE: int32 count, then count float bit patterns; JSON list of 0 / 1
//   wide_conv_check plan   FILE        -> FILE: int32 count, then rows [batch, cin, cout, h, w]; FILE.out: int64 rows
//                                         [rc, groups, cph, grid, block, lds, wide_conv_supported]
//   wide_conv_check pack   CIN COUT OUT -> OUT: int32 rows [n, ci, tap, q, zero] for every packed half; JSON: the sizes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "launch_plan.h"

static std::vector<int32_t> read_rows(const char* path, int fields) {
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    int32_t count = 0;
    if (std::fread(&count, sizeof(count), 1, f) != 1 || count < 0) std::exit(2);
    std::vector<int32_t> rows(static_cast<size_t>(count) * fields);
    if (!rows.empty() && std::fread(rows.data(), sizeof(int32_t), rows.size(), f) != rows.size()) std::exit(2);
    std::fclose(f);
    return rows;
}

template <typename T>
static void write_rows(const std::string& path, const std::vector<T>& rows) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(2);
    if (!rows.empty() && std::fwrite(rows.data(), sizeof(T), rows.size(), f) != rows.size()) std::exit(2);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "geometry") {
        std::printf("{\"P\": %d, \"PW\": %d, \"PP\": %d, \"cout\": %d, \"max_cin\": %d, \"threads\": %d, \"row_tiles\": %d, "
                    "\"zero_pos\": %d, \"stage_ldm\": %d, \"padded_plane\": %d, \"stage_bytes\": %zu, \"row_pos\": [",
                    mz::kWideP, mz::kWidePW, mz::kWidePP, mz::kWideCout, mz::kWideMaxCin, mz::kWideThreads, mz::kWideRowTiles,
                    mz::kWideZeroPos, mz::kWideStageLdm, mz::padded_plane(11, 11), mz::wide_stage_bytes());
        for (int m = 0; m < 16 * mz::kWideRowTiles; ++m) std::printf("%s%d", m ? ", " : "", mz::wide_row_pos(m));
        std::printf("], \"tap_offset\": [");
        for (int tap = 0; tap < 9; ++tap) std::printf("%s%d", tap ? ", " : "", mz::wide_tap_offset(tap));
        std::printf("], \"plane_pos\": [");
        for (int p = 0; p < mz::kWideP; ++p) std::printf("%s%d", p ? ", " : "", mz::wide_plane_pos(p));
        std::printf("], \"lds_bytes\": [");
        for (int cin = 1; cin <= mz::kWideMaxCin; ++cin) std::printf("%s%zu", cin > 1 ? ", " : "", mz::wide_lds_bytes(cin));
        std::printf("]}\n");
        return 0;
    }
    if (mode == "range" && argc >= 3) {
        const std::vector<int32_t> bits = read_rows(argv[2], 1);
        std::printf("[");
        for (size_t i = 0; i < bits.size(); ++i) {
            float x;
            std::memcpy(&x, &bits[i], sizeof(x));
            std::printf("%s%d", i ? ", " : "", mz::wide_in_range(x) ? 1 : 0);
        }
        std::printf("]\n");
        return 0;
    }
    if (mode == "plan" && argc >= 3) {
        const std::vector<int32_t> rows = read_rows(argv[2], 5);
        std::vector<int64_t> out;
        for (size_t i = 0; i + 4 < rows.size(); i += 5) {
            mz::WidePlan p;
            const int rc = mz::plan_wide_conv(rows[i], rows[i + 1], rows[i + 2], rows[i + 3], rows[i + 4], &p);
            const bool supported = mz::wide_conv_supported(rows[i + 1], rows[i + 2], rows[i + 3], rows[i + 4]);
            out.insert(out.end(), {rc, p.groups, p.cph, static_cast<int64_t>(p.grid), static_cast<int64_t>(p.block),
                                   static_cast<int64_t>(p.lds), supported ? 1 : 0});
        }
        write_rows(std::string(argv[2]) + ".out", out);
        std::printf("{\"rows\": %zu, \"fields\": 7}\n", rows.size() / 5);
        return 0;
    }
    if (mode == "pack" && argc >= 5) {
        const int cin = std::atoi(argv[2]), cout = std::atoi(argv[3]);
        const int64_t halfs = mz::wide_packed_halfs(cin, cout);
        std::vector<int32_t> out;
        out.reserve(static_cast<size_t>(halfs) * 5);
        for (int64_t i = 0; i < halfs; ++i) {
            const mz::WidePackSource s = mz::wide_pack_source(i, cin, cout);
            out.insert(out.end(), {s.n, s.ci, s.tap, s.q, s.zero ? 1 : 0});
        }
        write_rows(argv[4], out);
        std::printf("{\"halfs\": %lld, \"split_halfs\": %lld}\n", static_cast<long long>(halfs),
                    static_cast<long long>(mz::split_packed_halfs(cin, cout)));
        return 0;
    }
    return 2;
}
