"""The decode inside the lock-step tree kernels against float64, at every lane-group width.

expand_roots_kernel / expand_backup_kernel / expand_backup_select_kernel (csrc/mcts_kernels.hip) turn network logits into
tree statistics with support_to_scalar_group / support_to_scalar_pair / group_softmax (csrc/tree_device.h), instantiated
for G = 1 ... 64 lanes per tree and CH = 1, 2, 4 children per lane.  The bit-exact parity tests run the INJECTED
instantiations, where that code is compiled out; here the native entries are driven directly, without a network: after
one simulation the tree states every number the decode produced (floats widened to doubles), and each is held to the
float64 value of the same float32 logits within a bound derived from the arithmetic (parity_helpers
categorical_mean_rounding -> value_transform_bound, softmax_rounding_bound), at support sizes on both sides of the
register-resident form's limit F <= 4 G and on the rows where such code goes wrong (tests/lockstep_decode_cases.py).
What needs no tolerance is asserted bit for bit.  The worst error / bound ratio of every case is printed (-s shows it)
and collected in measure_out/lockstep_decode_report.json.

Indexing: mzmcts_readout's child_* rows and the ROOT row of mzmcts_export_tree are indexed by child SLOT (slot i is the
i-th legal action the caller handed over; entries from num_legal on are 0 / -1); every other row of export_tree is
indexed by action."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from lockstep_decode_cases import SHAPES, players_for, policy_cases, shape_id, supports_for, value_rows
from parity_helpers import (F32_UNIT, categorical_mean_rounding, make_search_config, softmax64, softmax_rounding_bound,
                            support_to_scalar64, value_transform_bound)

pytestmark = pytest.mark.gpu

DISCOUNT = 0.997
E_MAIN = 203
REPORT = {}


@pytest.fixture(scope="module")
def eng(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd.engine")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "lockstep_decode_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


CASES = [(A, gw, G, CH, s) for A, gw, G, CH in SHAPES for s in supports_for(G)]


def _engine(eng, A, gw, G, s, E, simulations=2):
    cfg = make_search_config(A, simulations, players_for(A), DISCOUNT, support=s, H=4)
    engine = eng.BatchedMCTS(cfg, E, group_width=gw)
    assert engine.group_width() == G or (gw == 0 and A > 64 and G == 64)
    return engine


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _is_f32(x):
    with np.errstate(over="ignore"):
        return np.array_equal(x.astype(np.float32).astype(np.float64), x)


def _trees(engine, E):
    """export_tree of every env, stacked: {key: [E, S + 1, A]}."""
    trees = [engine.export_tree(e) for e in range(E)]
    return {k: np.stack([t[k] for t in trees]) for k in trees[0]}


def _check_decoded(what, got, rows, kinds, s, G):
    """Decoded scalars of `rows` against float64 within the derived bound; returns the worst error / bound."""
    want = support_to_scalar64(rows, s)
    bound = value_transform_bound(want, categorical_mean_rounding(rows, s, G))
    assert np.isfinite(got).all(), (what, [k for k, g in zip(kinds, got) if not np.isfinite(g)])
    assert _is_f32(got), what
    ratio = np.abs(got - want) / bound
    worst = int(ratio.argmax())
    assert ratio[worst] <= 1.0, (what, kinds[worst], float(got[worst]), float(want[worst]), float(ratio[worst]))
    for kind, g in zip(kinds, got):
        if kind == "log_onehot_centre" or s == 0:
            assert g == 0.0, (what, kind, float(g))        # a probability of one on the support value 0: nothing rounds
    return float(ratio[worst])


def _check_priors(what, got, logits, kind, G, CH):
    """One soft-max row (float64-widened float32 priors) against float64; returns the worst error / bound."""
    n = len(logits)
    want = softmax64(logits)
    bound = softmax_rounding_bound(logits, G, CH)
    assert np.isfinite(got).all() and _is_f32(got), (what, kind, got)
    err = np.abs(got - want)
    assert (err <= bound).all(), (what, kind, int(np.argmax(err - bound)), got, want)
    # exp(l_i - max) / fl-sum of the same numbers: the sum misses 1 only by the roundings of that sum (CH - 1 additions in
    # a lane, log2(G) in the butterfly), of the reciprocal and of one product per entry
    assert abs(got.sum() - 1.0) <= 1.01 * (CH + np.log2(G) + 2) * F32_UNIT, (what, kind, got.sum())
    assert (got[np.isneginf(logits)] == 0.0).all(), (what, kind)
    if n == 1:
        assert got[0] == 1.0, (what, kind)
    if len(set(logits.tolist())) == 1 and n in (2, 4, 8):
        assert np.array_equal(got, np.full(n, 1.0 / n)), (what, kind, got)
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("A,gw,G,CH,s", CASES, ids=[shape_id(*c) for c in CASES])
def test_decode_and_priors_vs_float64(eng, A, gw, G, CH, s):
    E = E_MAIN
    two_player = players_for(A) == 2
    rows, row_kinds = value_rows(s, G, E, seed=10 * A + s)
    legal, policy, policy_kinds = policy_cases(A, E, seed=7 * A + gw + 1)
    # the reward vector of env e is the value vector of env perm[e]: a decode must not depend on the vector it is paired with
    perm = np.random.RandomState(s + 1).permutation(E)
    reward_rows = rows[perm]
    v_dev, r_dev, p_dev = _cuda(rows), _cuda(reward_rows), _cuda(policy)
    ratios = {}
    engine = _engine(eng, A, gw, G, s, E)
    try:
        engine.begin_search(legal, [e % players_for(A) for e in range(E)], False)
        engine.expand_roots(v_dev, r_dev, p_dev, torch.zeros(E, 4, device="cuda"))
        st = engine.readout()
        predicted = st["root_predicted_value"].copy()
        ratios["root value"] = _check_decoded("root value", predicted, rows, row_kinds, s, G)
        ratios["root prior"] = 0.0
        for e in range(E):
            n = len(legal[e])
            got = st["child_prior"][e]
            assert (got[n:] == 0.0).all() and (st["child_expanded"][e] == 0).all() and (st["visits"][e] == 0).all()
            # slot i holds the prior of action legal[e][i]: the kernel gathers the logits through root_action
            ratios["root prior"] = max(ratios["root prior"],
                                       _check_priors(f"root prior, env {e}", got[:n], policy[e][legal[e]], policy_kinds[e], G, CH))

        engine.select()
        picked = engine.batch_action.cpu().numpy()[:, 0]
        engine.expand_backup(v_dev, r_dev, p_dev, torch.zeros(E, 4, device="cuda"))
        st = engine.readout()
        depth, actions, _ = engine.last_paths()
        tree = _trees(engine, E)
        assert (depth == 1).all() and np.array_equal(actions[:, 0], picked)
        slot = tree["visits"][:, 0, :].argmax(axis=1)
        assert (tree["visits"][:, 0, :].sum(axis=1) == 1).all()
        assert np.array_equal(np.array([legal[e][slot[e]] for e in range(E)]), picked)
        env = np.arange(E)
        assert (tree["child_node"][env, 0, slot] == 1).all()
        value = tree["value_sum"][env, 0, slot]
        reward = tree["reward"][env, 0, slot]
        ratios["leaf value"] = _check_decoded("leaf value", value, rows, row_kinds, s, G)
        ratios["leaf reward"] = _check_decoded("leaf reward", reward, reward_rows, [row_kinds[i] for i in perm], s, G)
        # no tolerance: support_to_scalar_pair at the leaf and support_to_scalar_group at the root give the same bits for
        # the same vector, whichever vector shares the launch with it and whichever env it sits in
        assert np.array_equal(value, predicted), "a value vector decodes differently at the leaf"
        assert np.array_equal(reward, predicted[perm]), "a vector decodes differently as the reward of another env"
        assert np.array_equal(st["child_value_sum"][env, slot], value) and np.array_equal(st["child_reward"][env, slot], reward)
        # the backup is float64 (self_play.py:407-431): exact in the exported numbers
        backed_up = (reward - DISCOUNT * value) if two_player else (reward + DISCOUNT * value)
        assert np.array_equal(st["root_value_sum"], backed_up), "root value_sum is not reward +- discount * value"
        # min-max statistics: the leaf's and the root's value; the root's reward is the decode of its reward vector
        seen_leaf = reward + DISCOUNT * (-value if two_player else value)
        seen_root = predicted[perm] + DISCOUNT * (-backed_up if two_player else backed_up)
        assert np.array_equal(st["min_max"][:, 0], np.minimum(seen_leaf, seen_root)), "root reward / min-max"
        assert np.array_equal(st["min_max"][:, 1], np.maximum(seen_leaf, seen_root)), "root reward / min-max"
        ratios["leaf prior"] = 0.0
        for e in range(E):
            ratios["leaf prior"] = max(ratios["leaf prior"],
                                       _check_priors(f"leaf prior, env {e}", tree["prior"][e, 1], policy[e], policy_kinds[e], G, CH))
            assert (tree["visits"][e, 1] == 0).all() and (tree["child_node"][e, 1] == -1).all()
    finally:
        engine.close()
    REPORT[shape_id(A, gw, G, CH, s)] = ratios
    print(f"\n{shape_id(A, gw, G, CH, s)}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


PLACEMENT_CASES = [(A, gw, G, CH, s) for A, gw, G, CH in SHAPES for s in (10, 2 * G)]


@pytest.mark.parametrize("A,gw,G,CH,s", PLACEMENT_CASES, ids=[shape_id(*c) for c in PLACEMENT_CASES])
def test_bits_do_not_depend_on_where_an_env_sits(eng, A, gw, G, CH, s):
    """The same vectors at env 0, at the last env of a full workgroup (64 / G trees) and at the last env of a ragged
    tail, in launches of 64 / G - 1, 64 / G + 1 and 203 envs, between other envs' rows: the same bits everywhere."""
    per_group = 64 // G
    F = 2 * s + 1
    rs = np.random.RandomState(A + s)
    marked_value, marked_reward = (rs.standard_normal((2, F)) * 3).astype(np.float32)
    marked_policy = (rs.standard_normal(A) * 3).astype(np.float32)
    marked_legal = rs.permutation(A)[:max(1, A - 1)].astype(np.int32)
    seen = []
    for E in sorted({per_group - 1, per_group + 1, E_MAIN} - {0}):
        rows, _ = value_rows(s, G, max(E, 40), seed=E)
        rows, reward_rows = rows[:E].copy(), rows[:E][::-1].copy()
        legal, policy, _ = policy_cases(A, E, seed=E + 1)
        spots = sorted({0, E - 1} | ({per_group - 1} if per_group <= E else set()))
        for e in spots:
            rows[e], reward_rows[e], policy[e], legal[e] = marked_value, marked_reward, marked_policy, marked_legal
        engine = _engine(eng, A, gw, G, s, E)
        try:
            engine.begin_search(legal, [0] * E, False)
            engine.expand_roots(_cuda(rows), _cuda(reward_rows), _cuda(policy), torch.zeros(E, 4, device="cuda"))
            st = engine.readout()
            root = [(st["root_predicted_value"][e], st["child_prior"][e].copy()) for e in spots]
            engine.select()
            engine.expand_backup(_cuda(rows), _cuda(reward_rows), _cuda(policy), torch.zeros(E, 4, device="cuda"))
            for (predicted, prior), e in zip(root, spots):
                tree = engine.export_tree(e)
                slot = int(tree["visits"][0].argmax())
                seen.append((E, e, predicted, prior, tree["value_sum"][0, slot], tree["reward"][0, slot], tree["prior"][1].copy()))
        finally:
            engine.close()
    first = seen[0]
    for other in seen[1:]:
        for a, b, what in zip(first[2:], other[2:], ("root value", "root priors", "leaf value", "leaf reward", "leaf priors")):
            assert np.array_equal(a, b), f"{what}: env {other[1]} of {other[0]} differs from env {first[1]} of {first[0]}"


FUSED_STEP_CASES = [(2, 1, 1, 2, 10), (9, 8, 8, 2, 16), (9, 0, 16, 1, 10), (16, 0, 16, 1, 32), (121, 0, 64, 4, 10),
                    (121, 0, 64, 4, 128)]


@pytest.mark.parametrize("A,gw,G,CH,s", FUSED_STEP_CASES, ids=[shape_id(*c) for c in FUSED_STEP_CASES])
def test_fused_step_leaves_the_tree_of_expand_backup_then_select(eng, A, gw, G, CH, s):
    """expand_backup_select_kernel (the MZ_FUSED_STEP path) against expand_backup_kernel followed by select -- the latter
    through the wavefront-local queue of 256 trees: the same exported trees, paths and gathered actions, bit for bit."""
    E = E_MAIN
    rows, _ = value_rows(s, G, E, seed=A + 3 * s)
    reward_rows = rows[np.random.RandomState(1).permutation(E)]
    legal, policy, _ = policy_cases(A, E, seed=A + 5)
    to_play = [e % players_for(A) for e in range(E)]
    v_dev, r_dev, p_dev = _cuda(rows), _cuda(reward_rows), _cuda(policy)
    hidden = torch.zeros(E, 4, device="cuda")
    results = []
    for fused in (False, True):
        engine = _engine(eng, A, gw, G, s, E, simulations=3)
        try:
            if not fused:
                engine.set_select_queue(256)
            engine.begin_search(legal, to_play, False)
            engine.expand_roots(v_dev, r_dev, p_dev, hidden)
            engine.select()
            for _ in range(2):
                if fused:
                    engine.expand_backup_select(v_dev, r_dev, p_dev, hidden)
                else:
                    engine.expand_backup(v_dev, r_dev, p_dev, hidden)
                    engine.select()
            torch.cuda.synchronize()
            depth, actions, _ = engine.last_paths()
            results.append((_trees(engine, E), depth, actions, engine.batch_action.cpu().numpy().copy(),
                            {k: v.copy() for k, v in engine.readout().items()}))
        finally:
            engine.close()
    (tree_a, depth_a, actions_a, picked_a, st_a), (tree_b, depth_b, actions_b, picked_b, st_b) = results
    assert (tree_a["visits"][:, 0].sum(axis=1) == 2).all() and (depth_a >= 1).all()
    for key in tree_a:
        assert np.array_equal(tree_a[key], tree_b[key]), f"exported {key} differs"
    assert np.array_equal(depth_a, depth_b) and np.array_equal(actions_a, actions_b) and np.array_equal(picked_a, picked_b)
    for key in ("visits", "child_value_sum", "child_prior", "child_reward", "root_value_sum", "min_max", "max_tree_depth",
                "root_predicted_value", "depth_sum", "tie_break_words"):
        assert np.array_equal(st_a[key], st_b[key]), f"readout {key} differs"


def test_every_group_shape_is_reached():
    """The matrix covers every (G, CH) mcts_kernels.hip dispatch_group can produce, each on both sides of F <= 4 G."""
    want = {(1, 1), (1, 2), (2, 1), (4, 1), (4, 2), (8, 1), (8, 2), (16, 1), (32, 1), (64, 1), (64, 4)}
    assert {(G, CH) for _, _, G, CH, _ in CASES} == want
    for G, CH in want:
        sizes = {s for _, _, g, ch, s in CASES if (g, ch) == (G, CH)}
        assert any(0 < 2 * s + 1 <= 4 * G and 2 * s + 1 >= 4 * G - 1 for s in sizes) and any(2 * s + 1 == 4 * G + 1 for s in sizes)
