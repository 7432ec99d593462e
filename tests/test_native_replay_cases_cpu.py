"""What the native replay cases reach, shown by the reference alone (no GPU): the logits of every shape decoded in
float64 (native_replay.reference_streams) and searched on the C oracle must give deep backups, tie-breaks, tie storms
whose normaliser never separates, and both players -- test_gpu_native_replay.py is about exactly those.  And
native_replay.decoded_streams, the reading the GPU test rests on, against trees whose streams are known."""
import numpy as np
import pytest

from lockstep_decode_cases import SHAPES, shape_id
from native_replay import decoded_streams, dirichlet_words, oracle_exports, reference_streams, search_config
from native_replay_cases import S, T, cases, inputs
from parity_helpers import run_injected_on_oracle

SHAPE_SUPPORTS = sorted({(A, gw, G, CH, s) for A, gw, G, CH, s, _ in cases()})


def test_case_matrix():
    """Every shape at support 10 in every form it has and at 2 G in the three-step form; all eleven (G, CH)."""
    listed = cases()
    assert len(set(listed)) == len(listed)
    for A, gw, G, CH in SHAPES:
        forms = {(s, form) for a, w, _, _, s, form in listed if (a, w) == (A, gw)}
        want = {(10, "steps"), (10, "fused"), (2 * G, "steps")} | ({(10, "queue40"), (10, "queue256")} if A <= 64 else set())
        assert forms == want, (A, gw, forms)
    assert len({(G, CH) for _, _, G, CH, _, _ in listed}) == 11


@pytest.mark.parametrize("A,gw,G,CH,s", SHAPE_SUPPORTS, ids=[shape_id(*c) for c in SHAPE_SUPPORTS])
def test_cases_reach_deep_backups_ties_and_storms(oracle, A, gw, G, CH, s):
    case = inputs(A, gw, s)
    streams = reference_streams(case)
    got = run_injected_on_oracle(oracle, search_config(case), streams, temperature=case["temperature"])
    deep = int((got["max_tree_depth"] >= 3).sum())
    words = int((got["rng_words_run"] - dirichlet_words(oracle, case)).sum())
    tie_nodes = int((got["sim_ties"] > 1).sum())
    print(f"\n{shape_id(A, gw, G, CH, s)}: depth >= 3 in {deep} of {T} trees, {tie_nodes} tie nodes, {words} tie-break words")
    assert 2 * deep >= T, f"only {deep} of {T} trees reach depth 3"
    if A > 1:
        assert words >= 100, f"{words} tie-break words"
    else:
        assert (got["max_tree_depth"] == S).all()
    storms = case["storm"]
    assert storms.sum() >= T // 3
    assert (got["min_max"][storms, 0] == got["min_max"][storms, 1]).all(), "a tie storm's normaliser bounds separated"
    assert (got["min_max"][~storms, 0] < got["min_max"][~storms, 1]).all()
    assert set(case["to_play"]) == set(range(case["players"]))
    assert (got["visits"].sum(axis=1) == S).all()


READING_SHAPES = [(2, 1, 10), (5, 4, 8), (9, 0, 10), (17, 0, 10)]


@pytest.mark.parametrize("A,gw,s", READING_SHAPES)
def test_decoded_streams_returns_what_the_oracle_was_fed(oracle, A, gw, s):
    """Trees laid out as mzmcts_export_tree lays them out, built from Tree.node_stats along the oracle's own paths:
    decoded_streams must hand back the value, reward and prior streams the oracle was fed -- and refuse a path, a
    simulation index or a root indexing that is not the tree's."""
    case = inputs(A, gw, s)
    streams = reference_streams(case)
    cfg = search_config(case)
    for t in (0, 1, 2, 7):                    # (0: a storm tree)
        exports, depth, actions = oracle_exports(oracle, cfg, streams, t)
        legal = [streams["legal"][t]]
        value, reward, priors = decoded_streams(exports, depth, actions, legal)
        assert np.array_equal(value[0], streams["value"][t]) and np.array_equal(reward[0], streams["reward"][t])
        assert np.array_equal(priors[0], streams["priors"][t])
        # the root's row holds what reset gave it, by slot, noise mixed in: not a stream row
        n = len(legal[0])
        assert (exports[-1]["visits"][0, 0, :n].sum() == S) and (exports[-1]["visits"][0, 0, n:] == 0).all()
        with pytest.raises(AssertionError):   # the exports one simulation late
            decoded_streams(exports[1:], depth[:, :-1], actions[:, :-1], legal)
        with pytest.raises(AssertionError):   # the paths of the simulations one late
            decoded_streams(exports[:-1], depth[:, 1:], actions[:, 1:], legal)
        deep = np.flatnonzero(depth[0] >= 2)
        if len(deep):                         # a path cut short: an edge visited more than once, expanded long ago
            cut = depth.copy()
            cut[0, deep[0]] -= 1
            with pytest.raises(AssertionError):
                decoded_streams(exports, cut, actions, legal)
        if n >= 2 and legal[0] != list(range(n)):
            with pytest.raises((AssertionError, ValueError)):      # the root's row read by action instead of by slot
                decoded_streams(exports, depth, actions, [list(range(A))])
