"""The two kernels that DRAW the exploration noise on the GPU -- root_noise_kernel (single searches after
set_device_noise) and move_inputs_kernel (device-input move batches), csrc/mcts_kernels.hip -- at every position of
their trees' MT19937 streams.  Both step over the host's pending words, stage up to 96 untempered words of the block in
LDS and draw through np_legacy_rng.h DeviceStream with that window; the reference is numpy.random.RandomState itself
(tests/noise_stream_cases.py: set_state, skip, dirichlet, get_state), and everything is compared bit for bit: the rows,
the device copy of each stream (key block and position) and its host mirror.

E = 625, one env per start position 0..624 (nine full workgroups of 64 threads and one of 49), env e on the second block
of RandomState(1000 + e).  What each parametrization reaches, as tests/noise_stream_cases.py classifies numpy's own word
counts (computed by that module; the tests recompute it and assert the categories they are there for):

    (alpha, k)    words/draw   inside  window_out  block_end (p = 623 / odd window)  exact_end  two_regen  empty
    (0.25, 2)        8 - 20      615        -           8      (1 / 5)                    1          -        1
    (0.1, 9)        36 - 48      586        -          37      (1 / 19)                   1          -        1
    (0.3, 7)        28 - 48      592        -          31      (1 / 16)                   1          -        1
    (0.3, 121)     496 - 592       -       80         542      (1 / 48)                   2          -        1
    (0.3, 256)    1084 - 1216      -        -         111      (0 / 0)                    -        513        1
    (1.0, 3)             6       618        -           5      (1 / 3)                    1          -        1

  * layout "sweep": every env draws k entries -- the table above.  A window that survives the regeneration of its block
    can only be met again by a draw of more than 624 words: (0.3, 256) is the shape that holds `win_hi = 0`.
  * layout "ragged": env e draws 1 + (e mod k) entries (a row of one entry is numpy's x * (1 / x), 1.0 or the double below it, and still consumes words),
    every seventh env is inactive: lanes of one wavefront run different trip counts, some return before the staging.
    For (0.3, 256) this layout meets all six categories in one launch (inside 55, window_out 120, block_end 271,
    two_regen 89, empty 1 and, by the sweep's accident, no exact end).
  * layout "exact_end" (k <= 9): every env starts where its draw ends at 624 exactly, constructed with numpy from 16
    fixed keys -- the position stays lazily at 624, the block is not regenerated.
  * the skip in front of the draw (test_skip_in_front_of_the_draw): the pending words come from sample_actions on the host, as in
    production, at T = 1 (two words) and T = inf (a bounded draw); the states are chosen with numpy so that the skip
    ends at 623, ends at 624 (nothing to stage), crosses the block end, and ends inside the last 96 positions.
  * move_inputs_kernel: three-move device-input batches from the sweep's states against a twin engine that plays one
    search at a time through root_noise_kernel, and against numpy's accounting (per move: skip + noise words + tie-break
    words + sampling words); the rows of a batch's last move are read on the device (engine.noise_rows()) and held to
    numpy directly, single-move batches with ragged roots included.  The envs the kernel must leave alone: an empty
    legal set without sit-out (nothing stepped over, nothing drawn) and with moves_sit_out (pending words stepped over,
    nothing drawn, the ply counted: seen through the temperature-threshold rule).  Its two other early returns -- a
    stalled env, an env past its move limit -- cannot be produced in a device-input batch through the public API
    (mzmcts_moves_prepare_device sets every move limit to the batch length and assumes no tie-break counts), so no
    test reaches them."""
import importlib

import numpy as np
import pytest
import torch

import noise_stream_cases as cases
from parity_helpers import cartpole_model_and_weights, make_search_config, synthetic_model

pytestmark = pytest.mark.gpu

E = cases.E
S = 2                                           # injected searches: 625 trees x 2 simulations
BOARD_GAMES = {9: "tictactoe", 7: "connect4", 121: "gomoku"}
MOVE_SHAPES = [(0.25, 2), (0.1, 9), (0.3, 7), (0.3, 121)]      # fused CartPole FC; lock-step board games
SKIP_SHAPES = [(0.25, 2), (0.1, 9), (0.3, 121)]
PLACES = ("at_623", "at_624", "crosses", "middle")


@pytest.fixture(scope="module")
def eng(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd.engine")


# ---- reading an engine's streams -----------------------------------------------------------------------------------
def device_streams(eng, engine):
    key, pos = engine.rng_streams()
    torch.cuda.synchronize()
    n = engine.E
    keys = eng._device_view(key, n * 624, torch.int32, engine.device).cpu().numpy().view(np.uint32).reshape(n, 624)
    return keys, eng._device_view(pos, n, torch.int32, engine.device).cpu().numpy()


def assert_streams(eng, engine, want, device_want=None, what=""):
    """the host mirrors stand at the numpy states `want`; the device copies at `device_want` (default: the same)"""
    keys, pos = device_streams(eng, engine)
    for e, state in enumerate(want):
        dev = state if device_want is None else device_want[e]
        assert pos[e] == dev[2] and np.array_equal(keys[e], dev[1]), (what, "device stream", e, int(pos[e]), dev[2])
        mirror = engine.get_rng_state(e)
        assert mirror[2:] == (state[2], 0, 0.0) and np.array_equal(mirror[1], state[1]), (what, "host mirror", e, mirror[2], state[2])


def assert_rows(got, draws, A, what=""):
    """got [E, A]: numpy's row in front, 0.0 behind it; an env that drew nothing (None) holds zeros"""
    for e, d in enumerate(draws):
        n = 0 if d is None else len(d.row)
        if n:
            assert np.array_equal(got[e, :n].view(np.uint64), d.row.view(np.uint64)), (what, e, d.p, d.category)
        assert not got[e, n:].view(np.uint64).any(), (what, e)


# ---- root_noise_kernel: injected searches ----------------------------------------------------------------------------
def injected_inputs(n_envs, A, nlegal):
    """distinct priors everywhere, so that only the unavoidable tie of a search's first descent draws words"""
    rank = np.arange(1, A + 1, dtype=np.float64)
    root = np.zeros((n_envs, A))
    for e in range(n_envs):
        n = int(nlegal[e])
        if n:
            root[e, :n] = rank[:n][::-1] / rank[:n].sum()
    sims = [np.tile(np.roll(rank, s + 1) / rank.sum(), (n_envs, 1)) for s in range(S)]
    return root, sims


def injected_search(engine, nlegal, inputs):
    n_envs, A = engine.E, engine.A
    legal = np.tile(np.arange(A, dtype=np.int32), (n_envs, 1))
    root, sims = inputs
    engine.begin_search(legal, np.zeros(n_envs, np.int32), True, num_legal=np.asarray(nlegal, dtype=np.int32))
    engine.expand_roots_injected(np.zeros(n_envs), root)
    for s in range(S):
        engine.select(gather=False)
        engine.expand_backup_injected(np.full(n_envs, 0.25 * (s + 1)), np.zeros(n_envs), sims[s])
    stats = engine.readout()
    return engine.noise.copy(), stats["tie_break_words"].copy()


def injected_engine(eng, alpha, k, n_envs, states):
    config = make_search_config(k, S, 1, 0.997, alpha=alpha)
    engine = eng.BatchedMCTS(config, n_envs, seeds=list(range(n_envs)))
    engine.set_device_noise(True)
    for e, state in enumerate(states):
        engine.set_rng_state(e, state)
    return engine


def layout(name, alpha, k):
    """(start states, legal counts, numpy's draws) of a parametrization"""
    if name == "sweep":
        return [cases.sweep_state(e) for e in range(E)], [k] * E, list(cases.sweep(alpha, k))
    if name == "ragged":
        return [cases.sweep_state(e) for e in range(E)], [cases.ragged_n(e, k) for e in range(E)], list(cases.ragged_sweep(alpha, k))
    assert name == "exact_end"
    built = [cases.exact_end_state(alpha, k, 0, 5000 + 64 * i) for i in range(16)]
    states = [built[e % 16] for e in range(E)]
    return states, [k] * E, [cases.draw(s, alpha, k) for s in built] * (E // 16 + 1)


LAYOUTS = [("sweep", a, k) for a, k in cases.SHAPES] + [("ragged", a, k) for a, k in cases.SHAPES] + \
          [("exact_end", a, k) for a, k in cases.SHAPES if k <= 9]


@pytest.mark.parametrize("name,alpha,k", LAYOUTS, ids=lambda v: str(v))
def test_root_noise_kernel_equals_numpy_from_every_start_position(eng, name, alpha, k):
    states, nlegal, draws = layout(name, alpha, k)
    draws = draws[:E]
    # coverage is a condition of the test: from numpy's word accounting of these very states
    counts, (from_623, odd_window) = cases.counts(draws), cases.block_end_subcases(draws)
    if name == "sweep":
        assert counts == cases.counts(cases.sweep(alpha, k))
        cases.assert_coverage({(alpha, k): counts}, {(alpha, k): (from_623, odd_window)})
    elif name == "ragged":
        inactive = [e for e in range(E) if nlegal[e] == 0]
        assert len(inactive) == E // 7 and sum(n == 1 for n in nlegal) >= E // (2 * k)
        assert all(0 < sum(nlegal[e] == 0 for e in range(w, min(w + 64, E))) < 64 for w in range(0, E, 64))   # in every wavefront
        assert counts["empty"] == 1 and counts["inside"] and counts["block_end"] and from_623 == 1 and odd_window >= 1
        if k == 256:
            assert counts["window_out"] and counts["two_regen"]
    else:
        assert counts["exact_end"] == E and all(d.p + d.words == cases.BLOCK and d.regens == 0 for d in draws)
    engine = injected_engine(eng, alpha, k, E, states)
    rows, ties = injected_search(engine, nlegal, injected_inputs(E, k, nlegal))
    assert_rows(rows, draws, k, (name, alpha, k))
    for e, d in enumerate(draws):
        if d is not None and len(d.row) == 1:
            # numpy's x * (1 / x): 1.0 or the double below it, and the gamma variate consumed words all the same
            assert rows[e, 0] == d.row[0] and 1.0 - 2.0 ** -53 <= d.row[0] <= 1.0 and d.words >= 2
        if d is None:
            assert ties[e] == 0
    # device copy and host mirror: where numpy stands after the draw and the reported tie-break words; untouched if inactive
    want = [states[e] if d is None else cases.skipped(d.after, int(ties[e])) for e, d in enumerate(draws)]
    assert_streams(eng, engine, want, what=(name, alpha, k))
    engine.close()


# ---- the skip in front of the draw -----------------------------------------------------------------------------------
def sampling_words(state, n, temperature):
    """(words, numpy's state afterwards, the slot at T = inf) of select_action on numpy: one legacy double at T = 1,
    choice(n) -- a masked bounded draw -- at T = inf"""
    rs = np.random.RandomState()
    rs.set_state(state)
    slot = -1
    if np.isinf(temperature):
        slot = int(rs.randint(0, n))
    else:
        rs.random_sample()
    after = rs.get_state()
    return cases.words_between(state, after)[0], after, slot


def place_of(q, words, regens):
    end = q + words
    if regens:
        return "crosses"
    if end in (cases.BLOCK - 1, cases.BLOCK):
        return "at_623" if end == cases.BLOCK - 1 else "at_624"
    return "middle" if cases.BLOCK - cases.WINDOW < end < cases.BLOCK - 1 else ""


def skip_states(k):
    """per env (state before the host samples, temperature): nine keys for each temperature and place, the position
    found with numpy so that the sampled words end there"""
    out = []
    for t_index, temperature in enumerate((1.0, np.inf)):
        for p_index, place in enumerate(PLACES):
            for rep in range(9):
                if place == "crosses":
                    starts = [cases.BLOCK - 1, cases.BLOCK] if rep % 2 == 0 else [cases.BLOCK]
                elif place == "middle":
                    starts = [cases.BLOCK - cases.WINDOW + 4 + 9 * rep]
                else:
                    target = cases.BLOCK - 1 if place == "at_623" else cases.BLOCK
                    starts = [target - w for w in range(1, 9)]
                state = None
                for attempt in range(32):          # (a bounded draw ends at a given word only if that word is accepted)
                    key = cases.block_key(7000 + 1000 * attempt + 100 * t_index + 10 * p_index + rep)
                    for q in starts:
                        words, after, _ = sampling_words(cases.state_of(key, q), k, temperature)
                        if state is None and place_of(q, words, cases.words_between(cases.state_of(key, q), after)[1]) == place:
                            state = cases.state_of(key, q)
                    if state is not None:
                        break
                assert state is not None, (k, temperature, place, rep)
                out.append((state, temperature))
    return out


@pytest.mark.parametrize("alpha,k", SKIP_SHAPES)
def test_skip_in_front_of_the_draw(eng, alpha, k):
    chosen = skip_states(k)
    n_envs = len(chosen)
    assert n_envs == 72                                  # a full workgroup and a ragged one
    temperatures = np.array([t for _, t in chosen])
    nlegal = [k] * n_envs
    inputs = injected_inputs(n_envs, k, nlegal)
    engine = injected_engine(eng, alpha, k, n_envs, [])
    injected_search(engine, nlegal, inputs)              # a first search, from the seeded streams
    for e, (state, _) in enumerate(chosen):
        engine.set_rng_state(e, state)                   # device copy and mirror level, nothing pending
    actions, _ = engine.sample_actions(temperatures)     # the host consumes words: they are pending for the next search
    sampled = [sampling_words(state, k, t) for state, t in chosen]
    for e, (words, after, slot) in enumerate(sampled):
        mirror = engine.get_rng_state(e)
        assert mirror[2] == after[2] and np.array_equal(mirror[1], after[1]), e
        if temperatures[e] == 1.0:
            assert words == 2, e
        else:
            assert words >= 1 and actions[e] == slot, e
    rows, ties = injected_search(engine, nlegal, inputs)
    draws = [cases.draw(state, alpha, k, skip=sampled[e][0]) for e, (state, _) in enumerate(chosen)]
    # all four places, at both temperatures, from the accounting
    for temperature in (1.0, np.inf):
        places = {place_of(chosen[e][0][2], sampled[e][0], draws[e].skip_regens) for e in range(n_envs) if temperatures[e] == temperature}
        assert places == set(PLACES), (temperature, places)
    assert {d.p for d in draws} >= {cases.BLOCK - 1, cases.BLOCK} and any(d.a % 2 == 1 and d.category == "block_end" for d in draws)
    assert_rows(rows, draws, k, ("skip", alpha, k))
    assert_streams(eng, engine, [cases.skipped(d.after, int(ties[e])) for e, d in enumerate(draws)], what=("skip", alpha, k))
    engine.close()


# ---- move_inputs_kernel: device-input move batches against a twin that searches one move at a time --------------------
def game_setup(pkg, k):
    """(config, model, observations [E, ...], fused): the fused CartPole FC network for k = 2, a small fully-connected
    network searched lock-step on the board games' shapes"""
    models = importlib.import_module("muzero-hypermodel_amd.models")
    if k == 2:
        config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
        config.num_simulations = 4
        model, _ = cartpole_model_and_weights(models, config, "cuda")
        obs = np.random.RandomState(11).uniform(-0.05, 0.05, (E, 4)).astype(np.float32)
        return config, model, torch.from_numpy(obs).cuda(), True
    config = importlib.import_module("muzero-hypermodel_amd.games." + BOARD_GAMES[k]).MuZeroConfig()
    config.network, config.encoding_size, config.stacked_observations = "fullyconnected", 8, 0
    config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
    config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
    config.num_simulations = 4
    model, _ = synthetic_model(models, config, "cuda")
    obs = np.random.RandomState(11).randint(-1, 2, (E,) + tuple(config.observation_shape)).astype(np.float32)
    return config, model, torch.from_numpy(obs).cuda(), False


def make_engine(eng, config, model, fused, states, device_noise):
    engine = eng.BatchedMCTS(config, E, seeds=list(range(E)), group_width=16 if fused else 0)
    if fused:
        engine.configure_fused_fc(model)
    engine.set_device_noise(device_noise)
    for e, state in enumerate(states):
        engine.set_rng_state(e, state)
    return engine


def legal_arrays(A, nlegal):
    return np.tile(np.arange(A, dtype=np.int32), (E, 1)), np.asarray(nlegal, dtype=np.int32), np.zeros(E, np.int32)


def play_twin(twin, model, obs, nlegal_per_move, temperatures_per_move):
    """one search at a time with device noise (root_noise_kernel) and host sampling; per move the results and the words"""
    moves = []
    for nlegal, temperatures in zip(nlegal_per_move, temperatures_per_move):
        legal, nl, to_play = legal_arrays(twin.A, nlegal)
        st = twin.search(model, obs, legal, to_play, True, num_legal=nl)
        actions, _ = twin.sample_actions(np.asarray(temperatures, dtype=np.float64))
        moves.append(dict(actions=actions.copy(), visits=st["visits"].copy(), root_value_sum=st["root_value_sum"].copy(),
                          max_depth=st["max_tree_depth"].copy(), ties=st["tie_break_words"].copy(), noise=twin.noise.copy()))
    return moves


def play_batch(batch, model, obs, fused, nlegal_per_move, temperature, after_prepare=None):
    M = len(nlegal_per_move)
    legal, nl, to_play = legal_arrays(batch.A, nlegal_per_move[0])
    legal_dev, nl_dev, to_play_dev = torch.from_numpy(legal).cuda(), torch.from_numpy(nl).cuda(), torch.from_numpy(to_play).cuda()
    batch.moves_prepare_device(M, legal_dev, nl_dev, to_play_dev, temperature, True)
    if after_prepare:
        after_prepare(batch)
    for m in range(M):
        if m:
            nl_dev.copy_(torch.from_numpy(np.asarray(nlegal_per_move[m], dtype=np.int32)))    # (what environment kernels would do)
        if fused:
            batch.moves_enqueue(obs)
        else:
            batch.moves_enqueue_lockstep(model, obs)
    out = batch.moves_collect()
    rows = batch.noise_rows().cpu().numpy().copy()                  # the last move's rows, where the kernel wrote them
    return out, rows


def assert_moves_equal(out, twin_moves, searched):
    """searched[m][e]: env e was searched in move m"""
    for m, w in enumerate(twin_moves):
        live = np.asarray(searched[m])
        assert np.array_equal(out["actions"][m][live], w["actions"][live]), m
        assert (out["actions"][m][~live] == -1).all(), m
        assert np.array_equal(out["visits"][m][live], w["visits"][live]), m
        assert np.array_equal(out["root_value_sum"][m][live].view(np.uint64), w["root_value_sum"][live].view(np.uint64)), m
        assert np.array_equal(out["max_depth"][m][live], w["max_depth"][live]), m


@pytest.mark.parametrize("alpha,k", MOVE_SHAPES)
def test_three_move_device_input_batch_equals_twin_and_numpy(eng, pkg, alpha, k):
    config, model, obs, fused = game_setup(pkg, k)
    assert float(config.root_dirichlet_alpha) == alpha and len(config.action_space) == k
    states = [cases.sweep_state(e) for e in range(E)]
    M, nlegal = 3, [k] * E
    twin = make_engine(eng, config, model, fused, states, True)
    twin_moves = play_twin(twin, model, obs, [nlegal] * M, [np.ones(E)] * M)
    batch = make_engine(eng, config, model, fused, states, False)
    out, last_rows = play_batch(batch, model, obs, fused, [nlegal] * M, 1.0)
    assert np.array_equal(out["moves_done"], np.full(E, M))
    assert_moves_equal(out, twin_moves, [np.ones(E, bool)] * M)
    # numpy's accounting, per move: (nothing pending at move 0: skip 0) noise words + tie-break words + two sampling words
    state, before_last_sampling, categories = list(states), None, []
    for m in range(M):
        draws = [cases.draw(state[e], alpha, k) for e in range(E)]
        categories += [d.category for d in draws]
        assert_rows(twin_moves[m]["noise"], draws, k, ("twin", m))
        before_last_sampling = [cases.skipped(d.after, int(twin_moves[m]["ties"][e])) for e, d in enumerate(draws)]
        state = [cases.skipped(s, 2) for s in before_last_sampling]
    assert_rows(last_rows, draws, k, "the batch's last move")
    assert set(categories) >= ({"empty", "inside", "block_end", "exact_end"} if k <= 9 else {"empty", "window_out", "block_end"})
    # the batch sampled on the device: its copies stand at the end; the twin's host sampled last, its device copies lag by that
    assert_streams(eng, batch, state, what="batch")
    assert_streams(eng, twin, state, device_want=before_last_sampling, what="twin")
    batch.close()
    twin.close()


@pytest.mark.parametrize("alpha,k", MOVE_SHAPES)
def test_single_move_batch_rows_with_ragged_roots_equal_numpy(eng, pkg, alpha, k):
    config, model, obs, fused = game_setup(pkg, k)
    states = [cases.sweep_state(e) for e in range(E)]
    nlegal = [cases.ragged_n(e, k) for e in range(E)]
    draws = list(cases.ragged_sweep(alpha, k))
    counts = cases.counts(draws)
    assert counts["empty"] == 1 and counts["inside"] and counts["block_end"] and (k < 121 or counts["window_out"])
    twin = make_engine(eng, config, model, fused, states, True)
    twin_moves = play_twin(twin, model, obs, [nlegal], [np.ones(E)])
    batch = make_engine(eng, config, model, fused, states, False)
    out, rows = play_batch(batch, model, obs, fused, [nlegal], 1.0)
    searched = np.array([n > 0 for n in nlegal])
    assert np.array_equal(out["moves_done"], searched.astype(np.int32))
    assert_moves_equal(out, twin_moves, [searched])
    assert_rows(rows, draws, k, "batch")
    assert_rows(twin_moves[0]["noise"], draws, k, "twin")
    before_sampling = [states[e] if d is None else cases.skipped(d.after, int(twin_moves[0]["ties"][e])) for e, d in enumerate(draws)]
    want = [s if d is None else cases.skipped(s, 2) for s, d in zip(before_sampling, draws)]
    assert_streams(eng, batch, want, what="batch")
    assert_streams(eng, twin, want, device_want=before_sampling, what="twin")
    batch.close()
    twin.close()


# ---- the envs move_inputs_kernel must leave alone ---------------------------------------------------------------------
def late_states():
    """env e: a start position inside the last 96 words of its block, the last four positions and 624 among them; the
    two pending words (the host samples at T = 1 first) end before, at and behind the block's end"""
    tail = [cases.BLOCK - 4, cases.BLOCK - 3, cases.BLOCK - 2, cases.BLOCK - 1, cases.BLOCK]
    return [cases.state_of(cases.block_key(1000 + e), tail[(e // 4) % 5] if e % 8 < 4 else cases.BLOCK - cases.WINDOW + (e * 5) % 92) for e in range(E)]


def with_pending_words(engine, model, obs, states, k):
    """a first search without noise, the chosen states, then sample_actions at T = 1 on the host: two words pending"""
    legal, nl, to_play = legal_arrays(k, [k] * E)
    engine.search(model, obs, legal, to_play, False, num_legal=nl)
    for e, state in enumerate(states):
        engine.set_rng_state(e, state)
    engine.sample_actions(np.ones(E))


@pytest.mark.parametrize("sit_out", [False, True], ids=["inactive", "sit_out"])
def test_envs_move_inputs_kernel_leaves_alone(eng, pkg, sit_out):
    """TicTacToe's shape, two lock-step moves, two words pending per env.  Env kinds by e mod 4: 0 and 3 are searched in
    both moves, 2 has an empty legal set in both; 1 has one in both moves without sit-out, in move 0 only with sit-out.
    Without sit-out an empty legal set leaves the stream alone: the pending words stay pending, nothing is drawn, the env
    plays no move of the batch.  With moves_sit_out the kernel steps over the pending words in move 0, draws nothing, and
    counts the ply: under the temperature threshold 2 an env that sat move 0 out plays move 1 at T = 0 (no sampling words),
    as the envs that were searched in move 0 do."""
    alpha, k, M = 0.1, 9, 2
    config, model, obs, fused = game_setup(pkg, k)
    states = late_states()
    assert all(cases.BLOCK - cases.WINDOW <= s[2] <= cases.BLOCK for s in states)
    kind = np.arange(E) % 4
    empty_in_move_1 = (2,) if sit_out else (1, 2)
    nlegal = [[0 if kind[e] in (1, 2) else k for e in range(E)], [0 if kind[e] in empty_in_move_1 else k for e in range(E)]]
    searched = [np.array([n > 0 for n in row]) for row in nlegal]
    # under the threshold rule whoever is searched in move 1 has played (or sat out) one ply by then: T = 0
    temps = [np.ones(E), np.zeros(E) if sit_out else np.ones(E)]
    twin = make_engine(eng, config, model, fused, [], True)
    with_pending_words(twin, model, obs, states, k)
    twin_moves = play_twin(twin, model, obs, nlegal, temps)
    batch = make_engine(eng, config, model, fused, [], False)
    with_pending_words(batch, model, obs, states, k)

    def options(engine):
        if sit_out:
            engine.moves_sit_out(True)
            engine.moves_temperature_threshold(2, np.zeros(E, np.int32))
    out, last_rows = play_batch(batch, model, obs, fused, nlegal, 1.0, options)
    if sit_out:
        assert (out["moves_done"] == M).all()                       # a ply that was sat out is a move of the batch
    else:
        assert np.array_equal(out["moves_done"], np.where(searched[0], M, 0))
    assert_moves_equal(out, twin_moves, searched)
    # numpy's accounting per env: a device copy plus the words pending for it is where the mirror stands
    mirrors, batch_devices, twin_devices, last_draws, places = [], [], [], [], set()
    for e in range(E):
        mirror = cases.skipped(states[e], 2)                        # the host sampled at T = 1
        batch_dev, batch_lag, twin_dev, last = states[e], 2, states[e], None
        place = place_of(states[e][2], 2, cases.words_between(states[e], mirror)[1])
        for m in range(M):
            if searched[m][e]:
                d = cases.draw(batch_dev, alpha, k, skip=batch_lag)
                assert np.array_equal(d.row.view(np.uint64), cases.draw(mirror, alpha, k).row.view(np.uint64))
                twin_dev = cases.skipped(d.after, int(twin_moves[m]["ties"][e]))     # the twin's host samples
                mirror = cases.skipped(twin_dev, 2 if temps[m][e] == 1.0 else 0)
                batch_dev, batch_lag = mirror, 0                                     # the batch samples on the device
                last = d if m == M - 1 else None
            elif sit_out and batch_lag:
                batch_dev, batch_lag = cases.skipped(batch_dev, batch_lag), 0        # stepped over, nothing drawn
        if searched[0][e] or sit_out:
            places.add(place)                                       # (where move_inputs_kernel's skip ended)
        mirrors.append(mirror)
        batch_devices.append(batch_dev)
        twin_devices.append(twin_dev)
        last_draws.append(last)
    assert places == set(PLACES), places
    for e in np.flatnonzero(~searched[0] & ~searched[1]):           # never searched: untouched, or only stepped over
        want = cases.skipped(states[e], 2) if sit_out else states[e]
        assert batch_devices[e][2] == want[2] and np.array_equal(batch_devices[e][1], want[1])
    assert_rows(last_rows, last_draws, k, "the batch's last move")
    assert_streams(eng, batch, mirrors, device_want=batch_devices, what="batch")
    assert_streams(eng, twin, mirrors, device_want=twin_devices, what="twin")
    batch.close()
    twin.close()
