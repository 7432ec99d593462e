"""What the lock-step kernels MOVE, held to a model bit for bit: the hidden-state gathers of a descent and the writes into
the pool f32[S+1][E][H] (csrc/mcts_kernels.hip), in every form the launchers choose between.

The pool holds tags (tests/hidden_gather_cases.py: every float distinct), outputs sit between canary guards, and the slab
a gathered row must come from is worked out from the C oracle's recorded paths (from the engine's own last_paths() where
only the native entries exist; other tests pin those paths to the oracle) -- never from the engine's leaf_parent.  A row
from a wrong slab, env or offset, a tail element left out, a plane value computed another way or a store past the end
cannot compare equal: all comparisons are on the int32 views.  tests/test_hidden_gather_reference.py checks the model,
the streams' coverage of deep and freshly written parents, and that the tables reach every form, on the CPU."""
import importlib

import numpy as np
import pytest
import torch

import hidden_gather_cases as hg
from lockstep_decode_cases import policy_cases, value_rows
from parity_helpers import run_injected_on_oracle

pytestmark = pytest.mark.gpu

SUPPORT = 10


@pytest.fixture(scope="module")
def eng(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.engine")


_MODEL = {}


def _model(oracle, A, E=hg.E_MAIN, S=hg.S_MAIN):
    """(streams, parent[E, S], action[E, S]) of one stream set, computed once from the oracle and left unchanged."""
    key = (A, E, S)
    if key not in _MODEL:
        streams = hg.streams_for(A, E, S)
        want = run_injected_on_oracle(oracle, hg.fc_config(A, 4, S), streams)
        parents, picked = hg.parents_of_envs(want["sim_depth"], want["sim_actions"])
        parents.setflags(write=False)
        picked.setflags(write=False)
        _MODEL[key] = (streams, parents, picked)
    return _MODEL[key]


def _inactive_envs(E):
    return sorted(e % E for e in hg.INACTIVE)


def _assert_bits(got, want, what):
    got, want = hg.bits(got), hg.bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    rows, cols = np.nonzero(got != want)
    e, i = int(rows[0]), int(cols[0])
    raise AssertionError(f"{what}: {len(rows)} elements differ, first at row {e}, offset {i}: got 0x{int(got[e, i]) & 0xFFFFFFFF:08x}, "
                         f"want 0x{int(want[e, i]) & 0xFFFFFFFF:08x} (tag = 0x{hg.TAG_BASE:08x} + (slab * E + env) * H + offset)")


def _fill_canary(tensor):
    tensor.view(torch.int32).fill_(hg.CANARY)


def _pool_bits(engine):
    return engine.pool.cpu().numpy().view(np.int32)


def _injected_search(engine, streams, driver, inactive, select, after_select):
    """begin_search + injected roots, then S simulations: `select` (mzmcts_select or mzmcts_select_planes), `after_select(s)`,
    expand_backup -- or, for driver "fused", one plain select, then the one-launch step with its gather on, and a plain
    expand_backup for the last simulation."""
    legal = [[] if e in inactive else actions for e, actions in enumerate(streams["legal"])]
    engine.begin_search(legal, streams["to_play"], True)
    engine.expand_roots_injected(streams["root_reward"], streams["root_priors"])
    S = engine.S
    for s in range(S):
        if s == 0 or driver != "fused":
            select()
        after_select(s)
        step = (streams["value"][:, s], streams["reward"][:, s], streams["priors"][:, s, :])
        if driver == "fused" and s + 1 < S:
            engine.expand_backup_select_injected(*step, gather=True)
        else:
            engine.expand_backup_injected(*step)


# ---- part A: mzmcts_select's gathers ---------------------------------------------------------------------------------
def _run_select_case(eng, oracle, case, driver, inactive=False):
    A, gw, G, CH, H = case
    E, S = hg.E_MAIN, hg.S_MAIN
    streams, parents, picked = _model(oracle, A)
    out = _inactive_envs(E) if inactive else []
    pool = hg.tagged_pool(S, E, H)
    engine = eng.BatchedMCTS(hg.fc_config(A, H), E, seeds=streams["seeds"], group_width=gw)
    try:
        assert engine.group_width() == G and engine.pool.shape == pool.shape and engine.pool.data_ptr() % 16 == 0
        if driver.startswith("queue"):
            assert A <= 64
            engine.set_select_queue(int(driver[5:]))
        engine.pool.copy_(torch.from_numpy(pool))
        whole, engine.batch_hidden = hg.guarded(E, H)

        def after_select(s):
            want = hg.expected_hidden(pool, parents[:, s])
            want_action = picked[:, s].copy()
            # inactive envs: zeros from the in-kernel gather, slab 0's row from gather_hidden_kernel; action 0 from both
            want[out] = 0.0 if H <= 64 else pool[0, out]
            want_action[out] = 0
            _assert_bits(engine.batch_hidden.cpu().numpy(), want, f"simulation {s}: batch_hidden")
            got_action = engine.batch_action.cpu().numpy()[:, 0]
            assert np.array_equal(got_action, want_action), (s, np.nonzero(got_action != want_action)[0][:8].tolist())
            assert hg.guards_intact(whole), f"simulation {s}: a store outside batch_hidden"

        _injected_search(engine, streams, driver, out, engine.select, after_select)
        assert np.array_equal(_pool_bits(engine), hg.bits(pool)), "the search wrote into the hidden-state pool"
    finally:
        engine.close()


@pytest.mark.parametrize("case", hg.SELECT_CASES, ids=hg.select_case_id)
def test_select_gathers_the_parent_rows(eng, oracle, case):
    """mzmcts_select: select_tree's gather for H <= 64 (float4 and scalar, every lane-group shape), gather_hidden_kernel
    above (both forms, one block per row, two, and the capped grid's second lap)."""
    _run_select_case(eng, oracle, case, "select")


@pytest.mark.parametrize("queue", hg.QUEUES)
@pytest.mark.parametrize("case", hg.QUEUE_CASES, ids=hg.select_case_id)
def test_select_queue_gathers_the_parent_rows(eng, oracle, case, queue):
    """The same through select_queue_kernel: its own gather over the wavefront's trees for H <= 64 (70 envs: a second,
    ragged wavefront at 40 trees per wavefront, one ragged wavefront at 256), gather_hidden_kernel behind it above."""
    _run_select_case(eng, oracle, case, f"queue{queue}")


@pytest.mark.parametrize("case", hg.SELECT_CASES, ids=hg.select_case_id)
def test_fused_step_gathers_the_parent_rows(eng, oracle, case):
    """The same through expand_backup_select_kernel, whose gather may read the node its own launch has just expanded."""
    _run_select_case(eng, oracle, case, "fused")


# ---- part B: dynamics-input rows --------------------------------------------------------------------------------------
def _planes_engine(eng, case, seeds=None):
    c, h, w, A, E, S = case
    engine = eng.BatchedMCTS(hg.planes_config(A, c, h, w, S), E, seeds=seeds)
    assert engine.H == c * h * w and engine.state_shape == (c, h, w)
    return engine


def _run_planes_case(eng, oracle, case, inactive=False):
    c, h, w, A, E, S = case
    H, plane = c * h * w, h * w
    streams, parents, picked = _model(oracle, A, E, S)
    out = _inactive_envs(E) if inactive else []
    pool = hg.tagged_pool(S, E, H)
    engine = _planes_engine(eng, case, streams["seeds"])
    try:
        engine.pool.copy_(torch.from_numpy(pool))
        whole, engine.batch_planes = hg.guarded(E, H + plane)
        seen = set()

        def after_select(s):
            parent, action = parents[:, s].copy(), picked[:, s].copy()
            parent[out] = 0           # inactive envs: slab 0's row followed by a plane of zeros, from both kernels
            action[out] = 0
            _assert_bits(engine.batch_planes.cpu().numpy(), hg.expected_planes(pool, parent, action, plane, A),
                         f"simulation {s}: batch_planes")
            assert np.array_equal(engine.batch_action.cpu().numpy()[:, 0], action), s
            assert hg.guards_intact(whole), f"simulation {s}: a store outside batch_planes"
            seen.update(action.tolist())

        _injected_search(engine, streams, "select", out, engine.select_planes, after_select)
        assert np.array_equal(_pool_bits(engine), hg.bits(pool)), "the search wrote into the hidden-state pool"
        if not inactive:
            assert seen == set(range(A)), f"action planes never held {sorted(set(range(A)) - seen)}"
    finally:
        engine.close()


@pytest.mark.parametrize("case", hg.PLANES_CASES, ids=hg.planes_case_id)
def test_select_planes_lays_out_parent_rows_and_action_planes(eng, oracle, case):
    """mzmcts_select_planes: gather_dynamics_rows_kernel for rows <= 512 floats (ragged last block, the tightest
    multiply-shift division, the last short row), gather_dynamics_input_kernel above (float2, both scalar parities, the
    capped grid)."""
    _run_planes_case(eng, oracle, case)


def _native_inputs(A, E, G, seed):
    """Device logits of tests/lockstep_decode_cases.py for E envs (the same rows every simulation), legal actions."""
    rows, _ = value_rows(SUPPORT, G, max(E, 40), seed=seed)
    rows = rows[:E]
    reward_rows = rows[np.random.RandomState(seed + 1).permutation(E)]
    legal, policy, _ = policy_cases(A, E, seed=seed + 2)
    to_device = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    return to_device(rows), to_device(reward_rows), to_device(policy), legal


@pytest.mark.parametrize("row", hg.FUSED_PLANES_ROWS)
def test_fused_step_lays_out_the_dynamics_input(eng, row):
    """mzmcts_expand_backup_select_planes has no injected form: native logits, the pool filled the way a search fills it
    (slab 0 through expand_roots, slab s + 1 written in place into next_slab() before step s; what nobody wrote holds the
    canary), and the expected parents from the model over the engine's own recorded paths."""
    case = next(c for c in hg.PLANES_CASES if hg.planes_row(c) == row)
    c, h, w, A, E, S = case
    H, plane = c * h * w, h * w
    pool = hg.tagged_pool(S, E, H)
    engine = _planes_engine(eng, case)
    try:
        value, reward, policy, legal = _native_inputs(A, E, engine.group_width(), seed=row)
        _fill_canary(engine.pool)
        whole, engine.batch_planes = hg.guarded(E, H + plane)
        depth = np.zeros((E, S), np.int32)
        actions = np.full((E, S, S), -1, np.int32)
        engine.begin_search(legal, [e % hg.players_for(A) for e in range(E)], True)
        engine.expand_roots(value, reward, policy, torch.from_numpy(pool[0]).cuda())
        engine.select_planes()
        deep = 0
        for s in range(S):
            depth[:, s], actions[:, s, :], _ = engine.last_paths()
            parents, picked = hg.parents_of_envs(depth[:, :s + 1], actions[:, :s + 1])
            assert (parents[:, s] <= s).all()
            deep += int((parents[:, s] != 0).sum())
            _assert_bits(engine.batch_planes.cpu().numpy(), hg.expected_planes(pool, parents[:, s], picked[:, s], plane, A),
                         f"simulation {s}: batch_planes")
            assert np.array_equal(engine.batch_action.cpu().numpy()[:, 0], picked[:, s]), s
            assert hg.guards_intact(whole), f"simulation {s}: a store outside batch_planes"
            slab = engine.next_slab()
            assert slab.shape == (E, c, h, w) and slab.data_ptr() == engine.pool[s + 1].data_ptr()
            slab.copy_(torch.from_numpy(pool[s + 1]).cuda().view(E, c, h, w))
            if s + 1 < S:
                engine.expand_backup_select_planes(value, reward, policy)
            else:
                engine.expand_backup(value, reward, policy, None)
        assert deep > 0, "every parent was the root: the run says nothing about the slabs written on the way"
        assert np.array_equal(_pool_bits(engine), hg.bits(pool)), "a step wrote into the hidden-state pool"
    finally:
        engine.close()


# ---- part C: writes into the pool --------------------------------------------------------------------------------------
def _assert_pool(engine, want, what):
    got = _pool_bits(engine)
    if not np.array_equal(got, want):
        slabs = sorted(set(np.nonzero(got != want)[0].tolist()))
        raise AssertionError(f"{what}: pool slabs {slabs} are not what they should be "
                             f"({int((got != want).sum())} elements; 0x{hg.CANARY:08x} marks what nobody wrote)")


@pytest.mark.parametrize("case", hg.COPY_SLAB_CASES, ids=hg.copy_slab_case_id)
def test_network_outputs_land_in_their_slab(eng, case):
    """mzmcts_expand_roots(root_hidden), mzmcts_expand_backup_select(next_hidden), mzmcts_expand_backup(next_hidden): the
    root copy of expand_roots_kernel into slab 0 and copy_slab_kernel into slabs 1 and 2 -- fewer than four floats, a
    count that is no multiple of four, whole float4s, a source one float off a 16-byte boundary (the kernel's own
    alignment test sends it to the scalar loop), and more float4s than the capped grid has threads.  After each call the
    target slab is the source and every other slab what it was."""
    E, H, S, offset = case
    A = 3
    tags = hg.tagged_pool(S, E, H)
    engine = eng.BatchedMCTS(hg.fc_config(A, H, S), E)
    try:
        assert engine.pool.data_ptr() % 16 == 0
        value, reward, policy, legal = _native_inputs(A, E, engine.group_width(), seed=E + H)
        sources = []

        def source(k):
            base = torch.empty(E * H + offset, dtype=torch.float32, device="cuda")
            view = base[offset:].view(E, H)
            view.copy_(torch.from_numpy(tags[k]))
            assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
            sources.append(base)
            return view

        _fill_canary(engine.pool)
        want = np.full(tags.shape, hg.CANARY, np.int32)
        engine.begin_search(legal, [0] * E, False)
        engine.expand_roots(value, reward, policy, source(0))
        want[0] = hg.bits(tags[0])
        _assert_pool(engine, want, "expand_roots")
        engine.select()
        engine.expand_backup_select(value, reward, policy, source(1))
        want[1] = hg.bits(tags[1])
        _assert_pool(engine, want, "expand_backup_select")
        engine.expand_backup(value, reward, policy, source(2))
        want[2] = hg.bits(tags[2])
        _assert_pool(engine, want, "expand_backup")
    finally:
        engine.close()


@pytest.mark.parametrize("H,G", hg.ROOT_COPY_CASES)
def test_root_states_land_in_slab_0(eng, H, G):
    """The copy at the end of expand_roots_kernel, lanes j, j + G, ... of a tree's lane group: rows shorter than, equal to
    and longer than the group; the rows of inactive envs and every other slab keep the canary."""
    A, gw = {1: (2, 1), 16: (9, 0), 64: (9, 64)}[G]
    E, S = hg.E_MAIN, 2
    out = [0, 33]
    tags = hg.tagged_pool(S, E, H)
    engine = eng.BatchedMCTS(hg.fc_config(A, H, S), E, group_width=gw)
    try:
        assert engine.group_width() == G
        value, reward, policy, legal = _native_inputs(A, E, G, seed=H + G)
        for e in out:
            legal[e] = []
        _fill_canary(engine.pool)
        want = np.full(tags.shape, hg.CANARY, np.int32)
        want[0] = hg.bits(tags[0])
        want[0, out] = hg.CANARY
        engine.begin_search(legal, [0] * E, False)
        engine.expand_roots(value, reward, policy, torch.from_numpy(tags[0]).cuda())
        _assert_pool(engine, want, "expand_roots")
    finally:
        engine.close()


# ---- part D: what a batch row of an inactive env holds ---------------------------------------------------------------------
@pytest.mark.parametrize("driver,case", hg.INACTIVE_SELECT_CASES,
                         ids=[f"{d}-{hg.select_case_id(c)}" for d, c in hg.INACTIVE_SELECT_CASES])
def test_inactive_envs_get_a_defined_hidden_row(eng, oracle, driver, case):
    """include/mzmcts.h mzmcts_select: envs 0, 33 and E - 1 inactive (num_legal = 0) -- zeros from the in-kernel gather
    (with and without a select queue, and in the fused step), slab 0's row from gather_hidden_kernel, action 0 from all;
    every other env's row as before."""
    _run_select_case(eng, oracle, case, driver, inactive=True)


@pytest.mark.parametrize("row", hg.INACTIVE_PLANES_ROWS)
def test_inactive_envs_get_a_defined_planes_row(eng, oracle, row):
    """include/mzmcts.h mzmcts_select_planes: slab 0's row followed by a plane of zeros, from the short-row kernel and
    from gather_dynamics_input_kernel."""
    _run_planes_case(eng, oracle, next(c for c in hg.PLANES_CASES if hg.planes_row(c) == row), inactive=True)
