// fused_narrow.hip -- whole-move search kernel for "narrow" fully-connected networks (every layer fits a
// 16-lane DPP row: CartPole's 8/16-wide MLPs) and the matching lock-step inference kernels.
//
// One tree per DPP row, four trees per wavefront, `waves` wavefronts per workgroup sharing the staged
// weights; trees, paths, hidden states and the (N, n) exploration table live in LDS for the whole move,
// activations live in registers.  See narrow_device.h for the device functions and the arithmetic contract,
// mcts_kernels.hip for the generic fused kernel this one specialises.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

#include "fc_net_device.h"
#include "kernel_common.h"
#include "narrow_device.h"
#include "np_legacy_rng.h"
#include "tree_device.h"
#include "tree_layout.h"

namespace mz {

constexpr int kNarrowMaxThreads = 256;

// lanes of the row that can hold a child (the kernel's SPAN template argument): 2 (exactly two actions and block
// indices that fit a byte: the windowed descent), 4, 8 or 16
static inline int narrow_span(int A, int S) {
    if (A == 2 && S <= 254) return 2;
    int span = 4;
    while (span < A) span <<= 1;
    return span;
}

// Does this (engine, network) pair qualify for the narrow path?
bool narrow_supported(const TreeParams& p, const FcNet& net) {
    auto one_hidden = [](const FcMlp& m) { return m.n_layers == 2 && m.layer[0].out <= kRow; };
    if (p.group != kRow || p.A > kRow || p.chunks != 1) return false;
    if (net.enc + net.A > kRow || net.obs > kRow || net.F > 2 * kRow) return false;
    if (!(net.repr.n_layers == 1 || one_hidden(net.repr))) return false;
    if (!one_hidden(net.dyn) || !one_hidden(net.reward) || !one_hidden(net.value) || !one_hidden(net.policy)) return false;
    if (p.S < 1 || p.S >= 32768) return false;
    return true;
}

// LDS plan; prefers 4 wavefronts (16 trees) per workgroup, i.e. one workgroup per CU at 4096 trees, and the
// (N, n) table when it fits.  First pass: plans that let a CU keep four wavefronts of the kernel (one per
// SIMD); second pass: anything that fits a workgroup's 160 KB.  Returns false when nothing does.
bool plan_narrow_layout(const TreeParams& p, const FcNet& net, size_t lds_limit, NarrowLayout* out) {
    auto align16 = [](size_t v) { return (v + 15) / 16 * 16; };
    auto align64 = [](size_t v) { return (v + 63) / 64 * 64; };
    int rows = 4;
    if (const char* env = std::getenv("MZMCTS_NARROW_ROWS")) rows = std::max(1, std::min(4, std::atoi(env)));
    int max_mode = 2;
    if (const char* env = std::getenv("MZMCTS_NARROW_PBC2")) max_mode = std::max(0, std::min(2, std::atoi(env)));
    const size_t span = static_cast<size_t>(narrow_span(p.A, p.S));
    for (int pass = 0; pass < 2; ++pass)
    for (int mode = max_mode; mode >= 0; --mode) {
        if (mode == 2 && p.S > 63) continue;   // rows of 64 entries: n <= N <= S
        for (int waves = 4; waves >= 1; waves >>= 1) {
            NarrowLayout lay{};
            size_t off = 0;
            lay.off_pbc = 0;
            lay.pbc2_mode = mode;
            if (const char* env = std::getenv("MZMCTS_NARROW_EXACT_DIV")) lay.exact_division = std::atoi(env) != 0;
            off = align16(sizeof(double) * 2 * (static_cast<size_t>(p.S) + 1));
            if (mode == 2) {
                lay.off_pbc2 = static_cast<uint32_t>(off);
                off = align16(off + sizeof(double) * (static_cast<size_t>(p.S) + 1) * 64);
            } else if (mode == 1) {
                lay.off_pbc2 = static_cast<uint32_t>(off);
                off = align16(off + sizeof(double) * (static_cast<size_t>(p.S) + 1) * (static_cast<size_t>(p.S) + 2) / 2);
            } else {
                lay.off_pbc2 = 0xffffffffu;
            }
            lay.off_units = static_cast<uint32_t>(off);
            off += sizeof(float) * 4 * 4 * kRow * kNarrowUnits;
            lay.off_bias = static_cast<uint32_t>(off);
            off = align64(off + sizeof(float) * kRow * kNarrowUnits);
            lay.off_trees = static_cast<uint32_t>(off);   // 64-byte aligned (descend_pair flips address bits)
            size_t t = static_cast<size_t>(p.S + 1) * 32 * span;   // LdsTreeV<SPAN>::kBlockStride
            lay.off_side = static_cast<uint32_t>(t);
            t = align16(t + sizeof(SideStats) * static_cast<size_t>(p.S + 1) * span);
            lay.off_path = static_cast<uint32_t>(t);
            t = align16(t + sizeof(int32_t) * static_cast<size_t>(p.S));
            lay.off_hidden = static_cast<uint32_t>(t);
            t = align16(t + sizeof(float) * static_cast<size_t>(p.S + 1) * net.enc);
            lay.off_misc = static_cast<uint32_t>(t);
            t = align16(t + 4 * 2 * kRow);
            lay.off_desc = static_cast<uint32_t>(t);
            if (span == 2) t += 16 * static_cast<size_t>(p.S + 1);
            t = align64(t);
            lay.tree_bytes = static_cast<uint32_t>(t);
            lay.waves = waves;
            lay.rows = rows;
            const size_t total = off + static_cast<size_t>(waves) * rows * t;
            lay.total_bytes = static_cast<uint32_t>(total);
            // pass 0: a CU keeps 16 trees resident: 16 / (waves * rows) workgroups share its LDS
            if (total <= (pass == 0 ? lds_limit * waves * rows / 16 : lds_limit)) {
                *out = lay;
                return true;
            }
        }
    }
    return false;
}

// doubles of the (N, n) table of `mode`, rounded up to whole 16-byte words (0: the mode has no table at this S)
size_t narrow_table_doubles(int S, int mode) {
    const size_t K = static_cast<size_t>(S) + 1;
    size_t n = 0;
    if (mode == 2 && S <= 63) n = K * 64;
    if (mode == 1) n = K * (K + 1) / 2;
    return (n + 1) / 2 * 2;
}

// The table in device memory, once per engine: entry by entry what stage_narrow_tables computes in a launch (the same
// two IEEE operations on the same operands; entries the kernel never reads stay zero).
__global__ void narrow_table_kernel(const double* __restrict__ pbc_log, const double* __restrict__ pbc_sqrt, int S, int mode,
                                    double* __restrict__ out) {
    const int K = S + 1;
    const int total = mode == 2 ? K * 64 : K * (K + 1) / 2;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        int N, n;
        if (mode == 2) {
            N = t >> 6;
            n = t & 63;
            if (n > N) continue;
        } else {
            N = 0;
            int row = 0;  // N(N+1)/2
            while (row + N + 1 <= t) {
                row += N + 1;
                ++N;
            }
            n = t - row;
        }
        out[t] = pbc_log[N] * (pbc_sqrt[N] / static_cast<double>(n + 1));
    }
}

hipError_t build_narrow_table(const TreeParams& p, int mode, double* out, hipStream_t stream) {
    narrow_table_kernel<<<dim3(16), dim3(256), 0, stream>>>(p.pbc_log, p.pbc_sqrt, p.S, mode, out);
    return hipGetLastError();
}

__device__ __forceinline__ void stage_narrow_tables(const TreeParams& p, const NarrowLayout& lay, uint8_t* smem, int tid,
                                                    int nthreads) {
    double* pbc = reinterpret_cast<double*>(smem + lay.off_pbc);
    for (int i = tid; i <= p.S; i += nthreads) {
        pbc[i] = p.pbc_log[i];
        pbc[p.S + 1 + i] = p.pbc_sqrt[i];
    }
    if (lay.pbc2_table && lay.pbc2_mode != 0) {
        // the engine's copy: 16-byte loads, a batch of them in flight per thread, then the LDS stores
        const int K = p.S + 1;
        const int doubles = lay.pbc2_mode == 2 ? K * 64 : K * (K + 1) / 2;
        const int n16 = (doubles + 1) / 2;
        const uint4* src = reinterpret_cast<const uint4*>(lay.pbc2_table);
        uint4* dst = reinterpret_cast<uint4*>(smem + lay.off_pbc2);
        constexpr int kBatch = 8;
        for (int base = tid; base < n16; base += nthreads * kBatch) {
            uint4 v[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const int i = base + b * nthreads;
                v[b] = src[i < n16 ? i : n16 - 1];
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const int i = base + b * nthreads;
                if (i < n16) dst[i] = v[b];
            }
        }
    } else if (lay.pbc2_mode == 2) {
        // rows of 64: entry (N << 6) + n, n <= N -- the triangular table's values, addressed by shifts
        double* pbc2 = reinterpret_cast<double*>(smem + lay.off_pbc2);
        for (int t = tid; t < (p.S + 1) * 64; t += nthreads) {
            const int N = t >> 6, n = t & 63;
            if (n <= N) pbc2[t] = p.pbc_log[N] * (p.pbc_sqrt[N] / static_cast<double>(n + 1));
        }
    } else if (lay.pbc2_mode == 1) {
        // [N][n], n <= N: (log(..)+init) * (sqrt(N) / (n+1)) -- ucb_score's two operations (self_play.py:385-390)
        double* pbc2 = reinterpret_cast<double*>(smem + lay.off_pbc2);
        const int total = (p.S + 1) * (p.S + 2) / 2;
        int N = 0, row = 0;  // row = N(N+1)/2
        for (int t = tid; t < total; t += nthreads) {
            while (row + N + 1 <= t) {
                row += N + 1;
                ++N;
            }
            const int n = t - row;
            pbc2[t] = p.pbc_log[N] * (p.pbc_sqrt[N] / static_cast<double>(n + 1));
        }
    }
}

// -------------------------------------------------------------------------------------------------
// one launch per move: root inference + expansion + noise, S simulations, publish
// -------------------------------------------------------------------------------------------------
// Shape: GenericShape (the network's shape read at run time) or FlagshipShape (CartPole's, every value a constant; SPAN 2
// only) -- see narrow_device.h.  The launcher picks the form; both compute the same.
template <int SPAN, int PBC2, typename Shape>
__global__ __launch_bounds__(kNarrowMaxThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_fused_narrow_kernel(
    TreeParams p, FcNet net, NarrowLayout lay, const float* __restrict__ weights,
    const float* __restrict__ observations,  // [E][obs]
    MoveCtl ctl, int n_sims, int publish_tree) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    MZ_STAMP_DECL
    const double* pbc = reinterpret_cast<const double*>(smem + lay.off_pbc);
    const double* pbc2 = reinterpret_cast<const double*>(smem + (PBC2 ? lay.off_pbc2 : 0u));
    float4* units = reinterpret_cast<float4*>(smem + lay.off_units);
    float* bias = reinterpret_cast<float*>(smem + lay.off_bias);
    const int j = threadIdx.x % kRow;
    const int group_base = (threadIdx.x & 63) - j;  // lane of the row's first lane inside its wavefront
    const int row = group_base / kRow;
    const int tree_in_block = (threadIdx.x / 64) * lay.rows + row;
    const int e = blockIdx.x * (blockDim.x / 64) * lay.rows + tree_in_block;
    const bool prefetch = lay.prefetch != 0;
    NarrowInputs in{};
    // (a lane without a tree asks for env 0's: it stages with the others and leaves after the barrier)
    if (prefetch) in = narrow_load_inputs(p, net, ctl, observations, (row < lay.rows && e < p.E) ? e : 0, j);
    stage_narrow_tables(p, lay, smem, threadIdx.x, blockDim.x);
    stage_narrow_units(net, weights, units, bias, threadIdx.x, blockDim.x);
    __syncthreads();
    MZ_STAMP(0);

    if (row >= lay.rows) return;                    // this wavefront carries fewer than four trees
    if (e >= p.E) return;
    const int n_root = prefetch ? in.n_root : p.root_children[e];
    if (prefetch ? narrow_move_stalled(ctl, in, e, j) : move_stalled(p, ctl, e, j)) return;
    const double* noise = ctl.noise;
    const bool row_rng = lay.row_rng != 0;
    uint32_t* mt_key = p.mt_key + static_cast<size_t>(e) * kMtN;
    int32_t mt_pos = 0;   // row_rng: in every lane of the row; else lane 0's
    if (row_rng) {
        // the words the host mirror consumed (reset_search_state's loop), stepped over by the row: every lane reads
        // the position, the block is regenerated by all of them when the skip crosses its end
        const uint32_t skip = prefetch ? in.skip : (ctl.rng_skip ? ctl.rng_skip[e] : 0u);
        mt_pos = mt_skip_row(mt_key, prefetch ? in.mt_pos : p.mt_pos[e], skip, j);
        if (j == 0) {
            if (skip) p.mt_pos[e] = mt_pos;
            reset_search_state(p, e, nullptr);
        }
    } else if (j == 0) {
        reset_search_state(p, e, ctl.rng_skip);
    }
    if (n_root == 0) {
        if (j == 0 && ctl.actions) ctl.actions[e] = -1;
        return;
    }
    // the DPP lane mappings the code below relies on (a wrong assumption must not pass silently)
    if (row_shl1_bits(j) != ((j + 1 < kRow) ? j + 1 : 0) || row_ror_bits<1>(j) != ((j + kRow - 1) & (kRow - 1))) {
        if (j == 0) atomicOr(p.error_flag, 8);
        return;
    }

    uint8_t* region = smem + lay.off_trees + static_cast<size_t>(tree_in_block) * lay.tree_bytes;
    const LdsTreeV<SPAN> tree{region, reinterpret_cast<SideStats*>(region + lay.off_side),
                              reinterpret_cast<int32_t*>(region + lay.off_path)};
    float* hidden_lds = reinterpret_cast<float*>(region + lay.off_hidden);
    int32_t* root_action_lds = reinterpret_cast<int32_t*>(region + lay.off_misc);
    float* root_logit_lds = reinterpret_cast<float*>(region + lay.off_misc) + kRow;
    static_assert(!Shape::kFixed || SPAN == 2, "the fixed shape has two actions");
    const Shape shape(p, net);
    const int enc = shape.enc(), A = shape.actions(), F = shape.features(), support = shape.support();
    const bool two_player = shape.two_player();
    const bool wide_support = F > kRow;

    // ---- root: initial inference, root.expand over the legal actions, exploration noise ----------
    float predicted;
    {
        const float obs = prefetch ? in.obs : ((j < net.obs) ? observations[static_cast<size_t>(e) * net.obs + j] : 0.f);
        const NarrowHeads h = narrow_initial(units, bias, enc, wide_support, net.repr.n_layers == 2, obs, j);
        float unused;
        narrow_support_pair(h.value_a, h.value_b, h.value_a, h.value_b, F, support, j, predicted, unused);
        // child slot c of the root is action root_action[c]: fetch its logit across the lanes through LDS
        const int my_action = (j < n_root) ? (prefetch ? in.root_action : p.root_action[static_cast<size_t>(e) * A + j]) : 0;
        root_action_lds[j] = my_action;
        root_logit_lds[j] = h.policy;
        if (j < enc) hidden_lds[j] = h.norm;  // slab 0
        group_memory_fence();
        const bool valid = j < n_root;
        double prior[1] = {narrow_softmax(valid ? root_logit_lds[my_action] : 0.f, valid)};
        if (prefetch)
            write_root_children_row(tree, A, n_root, prior[0], noise != nullptr, in.noise, p.noise_frac, j);
        else
            write_root_children<kRow, 1>(tree, A, n_root, prior, noise ? noise + static_cast<size_t>(e) * A : nullptr,
                                         p.noise_frac, j);
        if constexpr (SPAN == 2) {  // the prior moves aside; the block holds table[0][0] * prior (see LdsTreeV)
            if (j == 0) *reinterpret_cast<uint4*>(region + lay.off_desc) = uint4{0u, 0u, 0u, 0u};   // (the root, at position 1 of its own table)
            if (j < A) {
                const double pr = tree.stats(0)[j].prior;
                tree.side(0)[j].prior = pr;
                tree.stats(0)[j].prior = exploration_factor<PBC2>(pbc, pbc2, p.S, 0, 0) * pr;
            }
        }
        group_memory_fence();
    }
    // prior_score factor of the children of a node expanded by this search: it has one visit when they are first scored
    const double leaf_factor = exploration_factor<PBC2>(pbc, pbc2, p.S, 1, 0);

    MinMax mm{INFINITY, -INFINITY};  // replicated in every lane of the row
    double root_value_sum = 0.0;     // lane 0
    const double root_reward = 0.0;  // log(one_hot(centre)) decodes to exactly 0
    if (!row_rng) mt_pos = (j == 0) ? p.mt_pos[e] : 0;
    uint32_t words = 0;
    int max_depth = 0;
    int64_t depth_sum = 0;
    unsigned long long exotic = lay.exact_division ? 1ull : 0ull;   // (per wavefront) a backed-up value left normalized_value's plain range
    MZ_STAMP(1);

    const ResidentWeights resident = load_resident_weights(units, bias, j);
    const float transform_reciprocal = inverse_transform_reciprocal();
    int root_entry = 0;
    if constexpr (SPAN == 2) root_entry = window_root_entry(region + lay.off_desc, j);
    // ---- S simulations, entirely inside the CU -----------------------------------------------------
    for (int sim = 0; sim < n_sims; ++sim) {
        Descent d;
        float state;
        if constexpr (SPAN == 2)
            d = descend_window(tree, region + lay.off_desc, root_entry, sim, n_root, mm, exotic, mt_key, mt_pos, words, row_rng, j,
                               group_base, p.error_flag);
        else
            d = descend_row<SPAN, PBC2>(tree, pbc, pbc2, p.S, A, sim, n_root, mm, exotic, mt_key, mt_pos, words, row_rng,
                                        j, group_base, p.error_flag MZ_DSTAMP_ARGS);
        state = hidden_lds[d.parent * enc + (j < enc ? j : 0)];
        // the backup's operands (leaf-side round) and the path entries the new node is linked under: asked for here and
        // between the layers of the network, needed after it
        BackupRound<SPAN> round = backup_fetch_path(tree, d.depth, ((d.depth - 1) >> 4) << 4, j);
        int link_entry = 0;
        if constexpr (SPAN == 2) link_entry = link_fetch_path(tree, d.depth, j);
        MZ_STAMP(2);
        const int action = (d.depth == 1) ? root_action_lds[d.slot] : d.slot;
        const float x0 = (j < enc) ? state : ((j - enc == action) ? 1.f : 0.f);
        const NarrowHeads h = narrow_recurrent(
            units, bias, enc, wide_support, x0, j, resident, [&]() { backup_fetch_records(tree, round, j); },
            [&]() { backup_fetch_factors<SPAN, PBC2>(round, pbc, pbc2, p.S, sim, j); });
        MZ_STAMP(3);
        float value_f, reward_f;
        double prior[1];
        if constexpr (Shape::kFixed) {   // the same decode with its short vectors packed (narrow_decode_flagship)
            narrow_decode_flagship(h, j, transform_reciprocal, value_f, reward_f, prior[0]);
        } else {
            narrow_support_pair<true>(h.value_a, h.value_b, h.reward_a, h.reward_b, F, support, j, value_f, reward_f,
                                      transform_reciprocal);
            prior[0] = narrow_softmax<SPAN, true>(h.policy, j < A);
        }
        MZ_STAMP(4);
        const int k_new = sim + 1;
        if constexpr (SPAN == 2) {
            write_pair_children(tree, k_new, A, prior[0], leaf_factor, j);
            link_new_node(region + lay.off_desc, link_entry, d.depth, k_new, j);
            root_entry = window_root_entry(region + lay.off_desc, j);
        } else {
            write_children<kRow, 1>(tree, k_new, A, prior, j);
        }
        if (j < enc) hidden_lds[k_new * enc + j] = h.norm;
        MZ_STAMP(5);
        backup_row<SPAN, PBC2>(tree, round, d.depth, sim, static_cast<double>(value_f), reward_f, two_player, p.discount, mm,
                               root_value_sum, root_reward, exotic, pbc, pbc2, p.S, j);
        group_memory_fence();
        if (d.depth > max_depth) max_depth = d.depth;
        depth_sum += d.depth;
        MZ_STAMP(6);
    }

    // ---- publish: per-tree statistics, the root's child block, and on request the whole tree -----------
    uint32_t sample_words = 0;
    int slot = 0;
    if (ctl.temperature && row_rng) {
        // SelfPlay.select_action on the tree's own stream (kernel_common.h), by every lane of the row alike: its words
        // are drawn row-wide, a block that ends here is regenerated by the row
        const ChildLinks* root_links = tree.links(0);
        slot = device_select_action_from([&](int i) { return root_links[i].visits; }, n_root,
                                         prefetch ? narrow_move_temperature(ctl, in) : move_temperature(ctl, e),
                                         [&]() { return mt_next_row(mt_key, mt_pos, j); }, &sample_words);
    }
    if (j == 0) {
        p.root_reward[e] = root_reward;
        p.root_predicted[e] = predicted;
        p.root_value_sum[e] = root_value_sum;
        p.min_max[e] = mm;
        p.max_depth[e] = max_depth;
        p.depth_sum[e] = depth_sum;
        if (ctl.temperature) {
            if (!row_rng) {
                const ChildLinks* root_links = tree.links(0);
                slot = device_select_action([&](int i) { return root_links[i].visits; }, n_root, move_temperature(ctl, e),
                                            mt_key, &mt_pos, &sample_words);
            }
            if (ctl.actions) ctl.actions[e] = slot >= 0 ? root_action_lds[slot] : slot;
            if (ctl.game_moves) ctl.game_moves[e] += 1;        // this env's game is one move longer
        }
        if (words | sample_words) p.mt_pos[e] = mt_pos;
        if (words) p.tie_words[e] = words;
        if (ctl.tie_words) ctl.tie_words[e] = words;
        if (ctl.sample_words) ctl.sample_words[e] = sample_words;
        if (ctl.root_value_sum) ctl.root_value_sum[e] = root_value_sum;
        if (ctl.root_predicted) ctl.root_predicted[e] = predicted;
        if (ctl.max_depth) ctl.max_depth[e] = max_depth;
        if (ctl.depth_sum) ctl.depth_sum[e] = static_cast<int32_t>(depth_sum);
    }
    if (ctl.visits && j < A) ctl.visits[static_cast<size_t>(e) * A + j] = (j < n_root) ? tree.links(0)[j].visits : 0;
    // (in LDS a block is two member arrays with the value sums apart, in HBM an array of 32-byte child records: 16-byte
    // word 2 c / 2 c + 1 of a record block are the stats / links of child c; a child never visited has value_sum 0)
    const int block_words = 2 * A;
    const int n_blocks = publish_tree ? n_sims + 1 : 1;
    for (int t = j; t < n_blocks * block_words; t += kRow) {
        const int k = t / block_words, i = t - k * block_words;
        uint4* dst = reinterpret_cast<uint4*>(p.blocks + (static_cast<size_t>(k) * p.E + e) * p.line_stride);   // own line, half 0
        if (i < A) {
            ChildStats st = tree.stats(k)[i];
            const SideStats sd = tree.side(k)[i];
            st.value_sum = tree.links(k)[i].visits > 0 ? sd.value_sum : 0.0;
            if constexpr (SPAN == 2) st.prior = sd.prior;
            *reinterpret_cast<ChildStats*>(dst + 2 * i) = st;
        } else {
            *reinterpret_cast<ChildLinks*>(dst + 2 * (i - A) + 1) = tree.links(k)[i - A];
        }
    }
    for (int t = j; t < n_blocks * enc; t += kRow) {
        const int k = t / enc, i = t - k * enc;
        p.hidden[(static_cast<size_t>(k) * p.E + e) * enc + i] = hidden_lds[t];
    }
    MZ_STAMP(7);
    MZ_STAMP_FLUSH;
}

// -------------------------------------------------------------------------------------------------
// lock-step form of the same network functions (one launch per inference over the [E, .] batch), so the
// fused kernel can be compared with the lock-step search bit for bit
// -------------------------------------------------------------------------------------------------
template <bool INITIAL>
__global__ __launch_bounds__(kNarrowMaxThreads) void fc_inference_narrow_kernel(
    FcNet net, const float* __restrict__ weights, int E, const float* __restrict__ in, const int64_t* __restrict__ action,
    float* __restrict__ value_logits, float* __restrict__ reward_logits, float* __restrict__ policy_logits,
    float* __restrict__ hidden_out) {
    __shared__ float4 units[kNarrowUnits * 4 * kRow];
    __shared__ float bias[kNarrowUnits * kRow];
    stage_narrow_units(net, weights, units, bias, threadIdx.x, blockDim.x);
    __syncthreads();
    const int e = blockIdx.x * (blockDim.x / kRow) + threadIdx.x / kRow;
    const int j = threadIdx.x % kRow;
    if (e >= E) return;
    const bool wide_support = net.F > kRow;
    NarrowHeads h;
    if (INITIAL) {
        const float obs = (j < net.obs) ? in[static_cast<size_t>(e) * net.obs + j] : 0.f;
        h = narrow_initial(units, bias, net.enc, wide_support, net.repr.n_layers == 2, obs, j);
    } else {
        const int a = static_cast<int>(action[e]);
        const float state = in[static_cast<size_t>(e) * net.enc + (j < net.enc ? j : 0)];
        const float x0 = (j < net.enc) ? state : ((j - net.enc == a) ? 1.f : 0.f);
        h = narrow_recurrent(units, bias, net.enc, wide_support, x0, j, load_resident_weights(units, bias, j));
    }
    if (j < net.enc) hidden_out[static_cast<size_t>(e) * net.enc + j] = h.norm;
    if (j < net.A) policy_logits[static_cast<size_t>(e) * net.A + j] = h.policy;
    const int centre = net.F / 2;
    if (j < net.F) {
        value_logits[static_cast<size_t>(e) * net.F + j] = h.value_a;
        // initial reward = log(one_hot(centre)): -inf everywhere but 0 at the centre (models.py:176-186)
        reward_logits[static_cast<size_t>(e) * net.F + j] = INITIAL ? (j == centre ? 0.f : -INFINITY) : h.reward_a;
    }
    if (kRow + j < net.F) {
        value_logits[static_cast<size_t>(e) * net.F + kRow + j] = h.value_b;
        reward_logits[static_cast<size_t>(e) * net.F + kRow + j] =
            INITIAL ? (kRow + j == centre ? 0.f : -INFINITY) : h.reward_b;
    }
}

#ifdef MZ_STAMPS
hipError_t read_stamp_sums_narrow(unsigned long long* out, bool reset) {
    hipError_t err = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp_sums), sizeof(unsigned long long) * 16);
    if (err == hipSuccess && reset) {
        unsigned long long zeros[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        err = hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_sums), zeros, sizeof(zeros));
    }
    return err;
}
#endif

// -------------------------------------------------------------------------------------------------
// launchers
// -------------------------------------------------------------------------------------------------
template <int SPAN>
static hipError_t launch_narrow_span(const TreeParams& p, const FcNet& net, const NarrowLayout& lay, const float* weights,
                                     const float* observations, const MoveCtl& ctl, int n_sims, int publish_tree,
                                     hipStream_t stream, const LaunchTiming* timing) {
    const int threads = 64 * lay.waves;
    const int trees = lay.waves * lay.rows;
    const int grid = (p.E + trees - 1) / trees;
    auto go = [&](auto kernel) {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lay.total_bytes));
        if (err != hipSuccess) return err;
        launch_kernel(kernel, dim3(grid), dim3(threads), lay.total_bytes, stream, timing, p, net, lay, weights, observations,
                      ctl, n_sims, publish_tree);
        return hipGetLastError();
    };
    // the constant-shape form exists for the two-action kernels with an exploration table (every CartPole search at
    // S <= 254); any other shape, and lay.generic_shape, take the run-time form
    if constexpr (SPAN == 2) {
        if (!lay.generic_shape && FlagshipShape::matches(p, net)) {
            if (lay.pbc2_mode == 2) return go(search_fused_narrow_kernel<2, 2, FlagshipShape>);
            if (lay.pbc2_mode == 1) return go(search_fused_narrow_kernel<2, 1, FlagshipShape>);
        }
    }
    if (lay.pbc2_mode == 2) return go(search_fused_narrow_kernel<SPAN, 2, GenericShape>);
    if (lay.pbc2_mode == 1) return go(search_fused_narrow_kernel<SPAN, 1, GenericShape>);
    return go(search_fused_narrow_kernel<SPAN, 0, GenericShape>);
}

hipError_t launch_search_fused_narrow(const TreeParams& p, const FcNet& net, const NarrowLayout& lay, const float* weights,
                                      const float* observations, const MoveCtl& ctl, int n_sims, int publish_tree,
                                      hipStream_t stream, const LaunchTiming* timing) {
    if (narrow_span(p.A, p.S) == 2) return launch_narrow_span<2>(p, net, lay, weights, observations, ctl, n_sims, publish_tree, stream, timing);
    if (p.A <= 4) return launch_narrow_span<4>(p, net, lay, weights, observations, ctl, n_sims, publish_tree, stream, timing);
    if (p.A <= 8) return launch_narrow_span<8>(p, net, lay, weights, observations, ctl, n_sims, publish_tree, stream, timing);
    return launch_narrow_span<16>(p, net, lay, weights, observations, ctl, n_sims, publish_tree, stream, timing);
}

hipError_t launch_fc_inference_narrow(const TreeParams& p, const FcNet& net, const float* weights, bool initial,
                                      const float* in, const int64_t* action, float* value_logits, float* reward_logits,
                                      float* policy_logits, float* hidden_out, hipStream_t stream) {
    const int threads = kNarrowMaxThreads;
    const int trees = threads / kRow;
    const int grid = (p.E + trees - 1) / trees;
    if (initial)
        fc_inference_narrow_kernel<true><<<dim3(grid), dim3(threads), 0, stream>>>(net, weights, p.E, in, action, value_logits,
                                                                                 reward_logits, policy_logits, hidden_out);
    else
        fc_inference_narrow_kernel<false><<<dim3(grid), dim3(threads), 0, stream>>>(net, weights, p.E, in, action, value_logits,
                                                                                  reward_logits, policy_logits, hidden_out);
    return hipGetLastError();
}

}  // namespace mz
