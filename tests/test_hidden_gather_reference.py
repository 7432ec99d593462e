"""The model behind tests/test_gpu_hidden_gather.py, checked without a GPU: the tags, the parent model against the C
oracle's recorded paths, the conditions that keep the GPU tests from passing on root-only parents, the short-row
kernel's multiply-shift division over its whole domain, and that the case tables reach every form of the gathers and
pool writes of csrc/mcts_kernels.hip."""
import numpy as np
import pytest

import hidden_gather_cases as hg
from parity_helpers import run_injected_on_oracle

STREAM_ACTIONS = (2, 3, 7, 9, 121)
CASE_ACTIONS = sorted({c[0] for c in hg.SELECT_CASES} | {c[3] for c in hg.PLANES_CASES})


def _oracle_paths(oracle, A, E=hg.E_MAIN, S=hg.S_MAIN):
    want = run_injected_on_oracle(oracle, hg.fc_config(A, 4, S), hg.streams_for(A, E, S))
    return want["sim_depth"], want["sim_actions"]


def test_tags_are_distinct_finite_floats():
    pool = hg.tagged_pool(3, 5, 7)
    assert pool.shape == (4, 5, 7) and pool.dtype == np.float32
    raw = hg.bits(pool).ravel()
    assert np.array_equal(raw, hg.TAG_BASE + np.arange(raw.size)) and np.isfinite(pool).all()
    assert len(np.unique(pool)) == pool.size                      # distinct as floats too, not only as bit patterns
    assert not (raw == hg.CANARY).any() and np.isnan(np.int32(hg.CANARY).view(np.float32))
    for S, E, H in [(12, 70, 15488), (24, 70, 8196), (2, 70, 30000)]:       # the largest pools of the GPU tests
        assert hg.TAG_BASE + (S + 1) * E * H < 0x7F800000
    with pytest.raises(AssertionError):
        hg.tagged_pool(1, 1 << 15, 1 << 15)


def test_expected_rows_come_from_the_parent_slab():
    pool = hg.tagged_pool(2, 3, 4)
    rows = hg.expected_hidden(pool, [2, 0, 1])
    assert np.array_equal(hg.bits(rows), hg.TAG_BASE + np.array([[24 + 0, 25, 26, 27], [4, 5, 6, 7], [12 + 8, 21, 22, 23]]))
    planes = hg.expected_planes(pool, [2, 0, 1], [0, 2, 1], 2, 3)
    assert planes.shape == (3, 6) and planes.dtype == np.float32 and np.array_equal(planes[:, :4], rows)
    assert np.array_equal(planes[:, 4:], np.array([[0, 0], [2, 2], [1, 1]], np.float32) / np.float32(3))


def test_parent_model_on_a_hand_made_tree():
    # root -a2-> n1 -a0-> n2; root -a1-> n3; n1 -a1-> n4; n2 -a2-> n5
    depth = np.array([1, 2, 1, 2, 3])
    actions = np.array([[2, -1, -1], [2, 0, -1], [1, -1, -1], [2, 1, -1], [2, 0, 2]])
    parents, picked = hg.parents_from_paths(depth, actions)
    assert parents.tolist() == [0, 1, 0, 1, 2] and picked.tolist() == [2, 0, 1, 1, 2]
    with pytest.raises(AssertionError):
        hg.parents_from_paths(np.array([1, 1]), np.array([[2, -1], [2, -1]]))       # the same child expanded twice
    with pytest.raises(KeyError):
        hg.parents_from_paths(np.array([2]), np.array([[2, 0]]))                    # a path through an unexpanded node


@pytest.mark.parametrize("A", sorted(set(STREAM_ACTIONS) | set(CASE_ACTIONS)))
def test_parent_model_against_the_oracle(oracle, A):
    """Every stream set the GPU tests replay: the model is consistent with the oracle's paths (parents_from_paths itself
    refuses a (parent, action) pair expanded twice and a path through a node nobody expanded), and the parents are not
    the easy ones -- conditions, so that a gather that always reads slab 0, or never the slab written just before, fails."""
    depth, actions = _oracle_paths(oracle, A)
    parents, picked = hg.parents_of_envs(depth, actions)
    s = np.arange(hg.S_MAIN)[None, :]
    assert (parents <= s).all() and (parents >= 0).all()
    assert np.array_equal(parents == 0, depth == 1)
    assert (picked >= 0).all() and (picked < A).all()
    moved, fresh, slabs = hg.coverage(parents)
    assert moved >= 0.5 and fresh >= 0.2, (moved, fresh)
    assert slabs == set(range(hg.S_MAIN)), sorted(slabs)


@pytest.mark.parametrize("case", hg.PLANES_CASES, ids=hg.planes_case_id)
def test_planes_streams_reach_every_action_and_slab(oracle, case):
    """The dynamics-input cases at their own env and simulation counts: the same conditions (for Gomoku's 12 simulations
    the slabs that exist), and every action value 0 .. A - 1 is reported at some simulation, so every plane value occurs."""
    _, _, _, A, E, S = case
    depth, actions = _oracle_paths(oracle, A, E, S)
    parents, picked = hg.parents_of_envs(depth, actions)
    moved, fresh, slabs = hg.coverage(parents)
    assert moved >= 0.5 and fresh >= 0.2, (moved, fresh)
    assert slabs == set(range(S))
    assert set(np.unique(picked).tolist()) == set(range(A))


def test_short_row_division_is_exact():
    """launch_gather_dynamics_input (mcts_kernels.hip, `if (row <= 512)`): per_block = max(1, 2048 / row) envs per block,
    magic = ceil(2^20 / row); gather_dynamics_rows_kernel divides t < per_block * row by row as (t * magic) >> 20 in
    32-bit arithmetic."""
    for row in range(2, 513):
        per_block = max(1, 2048 // row)
        magic = ((1 << 20) + row - 1) // row
        t = np.arange(per_block * row, dtype=np.uint64)
        assert int(t[-1]) * magic < 2 ** 32, row
        assert np.array_equal((t * np.uint64(magic)) >> np.uint64(20), t // np.uint64(row)), row


def test_action_planes_tell_a_division_from_a_reciprocal_multiply():
    """For every action count of the planes table some action a has fl(a * fl(1 / A)) != fl(a / A) in float32: a kernel
    that multiplies by the reciprocal fails the bitwise comparison."""
    for A in sorted({c[3] for c in hg.PLANES_CASES}):
        a = np.arange(A, dtype=np.float32)
        reciprocal = np.float32(1) / np.float32(A)
        assert ((a * reciprocal).astype(np.float32) != a / np.float32(A)).any(), A


# ---- the launchers' predicates, restated --------------------------------------------------------------------------------
def _select_form(A, H, queue=0, per_wave=1):
    """launch_select / launch_expand_backup_select (mcts_kernels.hip)."""
    fused = H <= 64                                   # `const bool fuse = p.H <= kFuseGatherMaxFloats;`
    queued = A <= 64 and queue > per_wave             # select_queue_trees: `if (p.A > 64 || requested <= per_wave)`
    if fused:
        vector = H % 4 == 0                           # select_tree / select_queue_kernel: `if ((p.H & 3) == 0)`
        return ("queue" if queued else "in-kernel", "float4" if vector else "scalar")
    vector = H % 4 == 0                               # gather_hidden_kernel: `if ((p.H & 3) == 0)`
    per_row = (H + 3) // 4                            # `const int per_row = (p.H + 3) / 4;`
    blocks = (per_row + 255) // 256                   # `int gy = (per_row + 255) / 256;`
    capped = blocks > 8                               # `if (gy > 8) gy = 8;`
    return ("gather_hidden", "float4" if vector else "scalar", min(blocks, 8), capped)


def _planes_form(H, plane, E):
    """launch_gather_dynamics_input (mcts_kernels.hip)."""
    row = H + plane
    if row <= 512:                                    # `if (row <= 512)`
        per_block = max(1, 2048 // row)               # `const int per_block = std::max(1, 2048 / row);`
        return ("rows", per_block, E % per_block)     # (envs of a ragged last block; 0: the last block is full)
    vector = ((H | row) & 1) == 0                     # gather_dynamics_input_kernel: `if (((p.H | row) & 1) == 0)`
    blocks = (row + 255) // 256                       # `int gy = (row + 255) / 256;`
    return ("input", "float2" if vector else "scalar", H & 1, blocks > 8)      # `if (gy > 8) gy = 8;`


def _copy_slab_form(E, H, slab, source_offset):
    """launch_copy_slab / copy_slab_kernel (mcts_kernels.hip); the pool and every source tensor start on a 256-byte
    boundary (the allocator's granularity), the slab `slab` of the pool E * H * slab floats further."""
    n = E * H
    whole = n % 4 == 0                                # `(n & 3) == 0`
    source_aligned = (4 * source_offset) % 16 == 0    # `(reinterpret_cast<uintptr_t>(src) & 15) == 0`
    target_aligned = (4 * n * slab) % 16 == 0         # `(reinterpret_cast<uintptr_t>(dst) & 15) == 0`
    blocks = max(1, (n // 4 + 255) // 256)            # `size_t blocks = (n / 4 + 255) / 256; if (blocks < 1) blocks = 1;`
    vector = whole and source_aligned and target_aligned
    pieces = n // 4 if vector else n
    return (whole, source_aligned, target_aligned, blocks > 2048, pieces > min(blocks, 2048) * 256)   # `if (blocks > 2048)`


def test_every_form_is_reached():
    """The case tables reach every code shape of the two movements: each lane-group shape of the in-kernel gather in its
    float4 and scalar form, the queue's rewrite of both, gather_hidden_kernel's forms below and under its grid cap, the
    short-row kernel with a ragged last block, gather_dynamics_input_kernel's three parities and its cap, copy_slab's
    three conditions and its cap."""
    groups = {(1, 1), (1, 2), (2, 1), (4, 1), (4, 2), (8, 1), (8, 2), (16, 1), (32, 1), (64, 1), (64, 4)}
    assert set(hg.GROUP_SHAPES) == groups
    seen = {(G, CH, _select_form(A, H)) for A, gw, G, CH, H in hg.SELECT_CASES}
    for G, CH in groups:
        assert (G, CH, ("in-kernel", "float4")) in seen and (G, CH, ("in-kernel", "scalar")) in seen
    for G, CH in ((1, 1), (16, 1), (64, 4)):          # rows shorter than a float4, than the group, of one float4
        assert {H for _, _, g, ch, H in hg.FUSED_GATHER_CASES if (g, ch) == (G, CH)} >= {1, 3, 4, 63, 64}
    for queue in hg.QUEUES:
        queued = {(G, CH, _select_form(A, H, queue, 64 // G)) for A, gw, G, CH, H in hg.QUEUE_CASES}
        for G, CH in groups - {(64, 4)}:
            if queue > 64 // G:                       # (one tree per lane and 64 lanes: a queue of 40 is no queue)
                assert (G, CH, ("queue", "float4")) in queued and (G, CH, ("queue", "scalar")) in queued
        assert all(A <= 64 for A, *_ in hg.QUEUE_CASES)
    assert {(G, CH) for _, _, G, CH, _ in hg.QUEUE_CASES} == groups - {(64, 4)}
    stand_alone = {_select_form(A, H) for A, gw, G, CH, H in hg.GATHER_HIDDEN_CASES}
    assert stand_alone >= {("gather_hidden", "scalar", 1, False), ("gather_hidden", "float4", 1, False),
                           ("gather_hidden", "float4", 2, False), ("gather_hidden", "float4", 8, True),
                           ("gather_hidden", "scalar", 8, True)}
    assert any(H > 64 and (H + 3) // 4 > 2048 for *_, H in hg.SELECT_CASES)

    planes = {}
    for case in hg.PLANES_CASES:
        c, h, w, A, E, S = case
        planes[hg.planes_row(case)] = _planes_form(c * h * w, h * w, E)
    assert sorted(planes) == [2, 153, 511, 512, 513, 514, 540, 2730, 15609]
    assert planes[2] == ("rows", 1024, 1)             # 1025 envs: the second block holds one
    assert all(planes[row][0] == "rows" for row in (153, 511, 512)) and planes[512][1] == 4 and planes[512][2] == 2
    assert planes[153][1] == 13 and planes[153][2] == 70 % 13 != 0
    assert planes[513] == ("input", "scalar", 0, False)          # H even, row odd
    assert planes[540] == ("input", "scalar", 1, False)          # H odd, row even
    assert planes[514] == ("input", "float2", 0, False)
    assert planes[2730] == ("input", "float2", 0, True)          # row > 2048: the capped grid
    assert planes[15609] == ("input", "scalar", 0, True)
    assert set(hg.FUSED_PLANES_ROWS) <= set(planes) and set(hg.INACTIVE_PLANES_ROWS) <= set(planes)
    assert {planes[row][0] for row in hg.INACTIVE_PLANES_ROWS} == {"rows", "input"}

    copies = {}
    for E, H, S, offset in hg.COPY_SLAB_CASES:
        for slab in range(1, S + 1):
            copies.setdefault((E, H, offset), set()).add(_copy_slab_form(E, H, slab, offset))
    assert copies[(1, 3, 0)] == {(False, True, False, False, False)}                  # n < 4: one block, one lap
    assert (False, True, False, False, False) in copies[(7, 3, 0)]               # n % 4 != 0, and a target off 16 bytes
    assert copies[(70, 64, 0)] == {(True, True, True, False, False)}             # float4: 1120 pieces over 5 blocks
    assert copies[(70, 64, 1)] == {(True, False, True, False, True)}             # only the source pointer says scalar; laps
    assert copies[(70, 30000, 0)] == {(True, True, True, True, True)}            # 2051 blocks wanted, 2048 given
    # (a whole number of float4s per slab puts every slab on a 16-byte boundary: the target's own test can only fail
    # together with n % 4 != 0 through this interface)
    assert all(form[2] or not form[0] for forms in copies.values() for form in forms)
    assert {(H % 4 == 0, G) for H, G in hg.ROOT_COPY_CASES} == {(v, G) for v in (False, True) for G in (1, 16, 64)}
