// Host-side check of csrc/launch_plan.h (the launch plans of board_conv.hip and net_kernels.hip), built and driven by
// tests/test_launch_plan_cpu.py:
//     g++ -O2 -std=c++17 launch_plan_check.cpp        (once more with -fsanitize=address,undefined)
// The input is a little-endian binary file written by the test: i32 rows, then `rows` records of i32 fields.  The plans
// go to FILE.out as `rows` records of i64 fields; one JSON object on the last line says how many of each.
//
//   launch_plan_check tower FILE    batch, cin0, channels, height, width, n_layers, split, const_plane, gated, n_heads,
//                                   cols_on, weights_aligned16, split_boards, layer1_skip, bad_layer (-1: none; else that
//                                   layer states one input channel too many)
//                                   -> rc, kernel, nt, sb, waves, samples, cp0, cp1, grid, block, lds, gate_samples
//   launch_plan_check conv FILE     batch, cin, cout, height, width -> rc, nt, sb, grid, block, lds
//   launch_plan_check blocks FILE   batch, channels, height, width, split_boards -> mzmcts_board_tower_blocks
//   launch_plan_check heads FILE    n_heads, batch, cols_on, use_mfma, then (C, P, R, Hd, O) x 3
//                                   -> rc, kernel, lds, per_cu, grid_x, grid_y, block, then per head: NT1, NT2, KS, G of the
//                                   plan (zeros unless the kernel is mfma), MfmaHeadShape::total(), HeadShape::total(),
//                                   wave_head_split
//   launch_plan_check heads_product FILE   the values C, P, n_heads, cols_on, use_mfma, batch, n_tails, then n_tails x
//                                   (R, Hd, O): every ORDERED launch of n_heads heads drawn from the tails (the last head
//                                   varies fastest) -> i32 x 3 per launch in FILE.out:
//                                   kernel | per_cu << 2 | refused << 6 | lds << 7 (lds 0 when refused);
//                                   per head h, << 7 h: 4 bits of form (0: none; else 1 + (NT1 == 4) + 2 (NT2 == 2) +
//                                   4 (KS == 16), G following KS) | 3 bits log2(split) of the wave layout; grid_x
//   launch_plan_check sizes FILE    (no rows) -> JSON only: the LDS bytes of the two forms 64 channels on 3 x 3 boards would
//                                   take, and of the board-column launches
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "launch_plan.h"

namespace {

std::vector<int32_t> read_rows(const char* path, int fields, int32_t* rows) {
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(rows, sizeof(int32_t), 1, f) != 1 || *rows < 0) {
        std::perror(path);
        std::exit(2);
    }
    std::vector<int32_t> data(static_cast<size_t>(*rows) * fields);
    if (!data.empty() && std::fread(data.data(), sizeof(int32_t), data.size(), f) != data.size()) std::exit(3);
    std::fclose(f);
    return data;
}

int write_rows(const char* path, const std::vector<int64_t>& out, int32_t rows, int fields) {
    const std::string name = std::string(path) + ".out";
    FILE* f = std::fopen(name.c_str(), "wb");
    if (!f || (!out.empty() && std::fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size())) return 4;
    std::fclose(f);
    std::printf("{\"rows\": %d, \"fields\": %d}\n", rows, fields);
    return 0;
}

int tower(const char* path) {
    constexpr int kIn = 15, kOut = 12;
    int32_t rows;
    const std::vector<int32_t> in = read_rows(path, kIn, &rows);
    std::vector<int64_t> out(static_cast<size_t>(rows) * kOut);
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t* a = in.data() + static_cast<size_t>(r) * kIn;
        int32_t cin[16];
        for (int l = 0; l < 16; ++l) cin[l] = (l == 0 ? a[1] : a[2]) + (l == a[14] ? 1 : 0);
        mz::TowerShape s{};
        s.batch = a[0];
        s.cin0 = a[1];
        s.channels = a[2];
        s.height = a[3];
        s.width = a[4];
        s.n_layers = a[5];
        s.layer_cin = cin;
        s.split = a[6] != 0;
        s.const_plane = a[7] != 0;
        s.gated = a[8] != 0;
        s.n_heads = a[9];
        s.cols_on = a[10] != 0;
        s.weights_aligned16 = a[11] != 0;
        s.split_boards = a[12];
        s.layer1_skip = a[13] != 0;
        mz::TowerPlan p;
        const int rc = mz::plan_tower(s, &p);
        int64_t* o = out.data() + static_cast<size_t>(r) * kOut;
        const int64_t fields[kOut] = {rc,    static_cast<int64_t>(p.kernel), p.nt,    p.sb, p.waves, p.samples, p.cp0,
                                      p.cp1, p.grid, p.block, static_cast<int64_t>(p.lds), p.gate_samples};
        std::memcpy(o, fields, sizeof(fields));
    }
    return write_rows(path, out, rows, kOut);
}

int conv(const char* path) {
    constexpr int kIn = 5, kOut = 6;
    int32_t rows;
    const std::vector<int32_t> in = read_rows(path, kIn, &rows);
    std::vector<int64_t> out(static_cast<size_t>(rows) * kOut);
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t* a = in.data() + static_cast<size_t>(r) * kIn;
        mz::ConvPlan p;
        const int rc = mz::plan_board_conv(a[0], a[1], a[2], a[3], a[4], &p);
        const int64_t fields[kOut] = {rc, p.nt, p.sb, p.grid, p.block, static_cast<int64_t>(p.lds)};
        std::memcpy(out.data() + static_cast<size_t>(r) * kOut, fields, sizeof(fields));
    }
    return write_rows(path, out, rows, kOut);
}

int blocks(const char* path) {
    constexpr int kIn = 5;
    int32_t rows;
    const std::vector<int32_t> in = read_rows(path, kIn, &rows);
    std::vector<int64_t> out(static_cast<size_t>(rows));
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t* a = in.data() + static_cast<size_t>(r) * kIn;
        out[r] = mz::board_tower_blocks(a[0], a[1], a[2], a[3], a[4]);
    }
    return write_rows(path, out, rows, 1);
}

int heads(const char* path) {
    constexpr int kIn = 4 + 5 * mz::kMaxHeads, kPer = 7, kOut = 7 + kPer * mz::kMaxHeads;
    int32_t rows;
    const std::vector<int32_t> in = read_rows(path, kIn, &rows);
    std::vector<int64_t> out(static_cast<size_t>(rows) * kOut);
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t* a = in.data() + static_cast<size_t>(r) * kIn;
        mz::HeadDims dims[mz::kMaxHeads];
        for (int h = 0; h < mz::kMaxHeads; ++h) dims[h] = mz::HeadDims{a[4 + 5 * h], a[5 + 5 * h], a[6 + 5 * h], a[7 + 5 * h], a[8 + 5 * h]};
        mz::HeadsPlan p;
        const int rc = mz::plan_heads(dims, a[0], a[1], a[2] != 0, a[3] != 0, &p);
        int64_t* o = out.data() + static_cast<size_t>(r) * kOut;
        const int64_t launch[7] = {rc, static_cast<int64_t>(p.kernel), static_cast<int64_t>(p.lds), p.per_cu, p.grid_x, p.grid_y, p.block};
        std::memcpy(o, launch, sizeof(launch));
        for (int h = 0; h < a[0] && h < mz::kMaxHeads; ++h) {
            const mz::HeadDims& d = dims[h];
            if (d.C < 1 || d.P < 1 || d.R < 1 || d.Hd < 1 || d.O < 1) continue;     // (refused: no layout to report)
            const int split = mz::wave_head_split(d.Hd);
            const int64_t per[kPer] = {p.form[h].nt1, p.form[h].nt2, p.form[h].ks, p.form[h].g,
                                       mz::MfmaHeadShape{d.C, d.P, d.R, d.Hd, d.O}.total(),
                                       mz::HeadShape{d.C, d.P, d.R, d.Hd, d.O, split}.total(), split};
            std::memcpy(o + 7 + kPer * h, per, sizeof(per));
        }
    }
    return write_rows(path, out, rows, kOut);
}

int heads_product(const char* path) {
    FILE* f = std::fopen(path, "rb");
    int32_t head[8];
    if (!f || std::fread(head, sizeof(int32_t), 8, f) != 8 || head[0] < 7 || head[3] < 1 || head[3] > mz::kMaxHeads || head[7] < 1) return 2;
    const int C = head[1], P = head[2], n = head[3], n_tails = head[7];
    std::vector<int32_t> tails(static_cast<size_t>(n_tails) * 3);
    if (std::fread(tails.data(), sizeof(int32_t), tails.size(), f) != tails.size()) return 3;
    std::fclose(f);
    size_t launches = 1;
    for (int h = 0; h < n; ++h) launches *= n_tails;
    std::vector<int32_t> out(launches * 3);
    for (size_t i = 0; i < launches; ++i) {
        mz::HeadDims dims[mz::kMaxHeads] = {};
        size_t rest = i;
        for (int h = n - 1; h >= 0; --h, rest /= n_tails) {
            const int32_t* t = tails.data() + (rest % n_tails) * 3;
            dims[h] = mz::HeadDims{C, P, t[0], t[1], t[2]};
        }
        mz::HeadsPlan p;
        const int rc = mz::plan_heads(dims, n, head[6], head[4] != 0, head[5] != 0, &p);
        const int32_t lds = rc == MZMCTS_OK ? static_cast<int32_t>(p.lds) : 0;
        if (lds >= (1 << 24) || p.per_cu > 15) return 5;
        int32_t per_head = 0;
        for (int h = 0; h < n && rc == MZMCTS_OK; ++h) {              // (refused: no layout to report)
            const mz::MfmaForm& m = p.form[h];
            int form = 0, log_split = 0;
            if (m.nt1 || m.nt2 || m.ks || m.g) {
                const bool known = (m.nt1 == 1 || m.nt1 == 4) && (m.nt2 == 1 || m.nt2 == 2) && ((m.ks == 4 && m.g == 6) || (m.ks == 16 && m.g == 2));
                if (!known) return 6;
                form = 1 + (m.nt1 == 4) + 2 * (m.nt2 == 2) + 4 * (m.ks == 16);
            }
            for (int v = p.wave[h].split; v > 1; v >>= 1) ++log_split;
            per_head |= (form | log_split << 4) << (7 * h);
        }
        out[3 * i] = static_cast<int32_t>(p.kernel) | p.per_cu << 2 | (rc != MZMCTS_OK) << 6 | lds << 7;
        out[3 * i + 1] = per_head;
        out[3 * i + 2] = static_cast<int32_t>(p.grid_x);
    }
    const std::string name = std::string(path) + ".out";
    FILE* g = std::fopen(name.c_str(), "wb");
    if (!g || std::fwrite(out.data(), sizeof(int32_t), out.size(), g) != out.size()) return 4;
    std::fclose(g);
    std::printf("{\"rows\": %zu, \"fields\": 3}\n", launches);
    return 0;
}

int sizes() {
    std::printf("{\"row_tile_4_3_3_16\": %zu, \"split_3_3_16\": %zu, \"patch_boards\": %d, \"col_wave_floats\": %d, \"col_head_w1_floats\": %d}\n",
                mz::row_tile_lds_bytes(3, 3, 16, 64 + 4, 64 + 4), mz::split_lds_bytes(3, 3, 16, 64 + 8, 64 + 8),
                mz::PatchGeometry<6, 6>::BPW * mz::kColWaves, mz::kColWaveFloats, mz::kColHeadW1Floats);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    if (!std::strcmp(argv[1], "tower")) return tower(argv[2]);
    if (!std::strcmp(argv[1], "conv")) return conv(argv[2]);
    if (!std::strcmp(argv[1], "blocks")) return blocks(argv[2]);
    if (!std::strcmp(argv[1], "heads")) return heads(argv[2]);
    if (!std::strcmp(argv[1], "heads_product")) return heads_product(argv[2]);
    if (!std::strcmp(argv[1], "sizes")) return sizes();
    return 1;
}
