"""Reanalyse in batches on the device (include/mzreplay.h mzreplay_reanalyse_*, csrc/reanalyse_plan.h; ReplayBuffer.reanalyse_* and
Reanalyse.reanalyse_games): many games per pass, the plan drawn on the device, for fully-connected networks the whole pass in
one HIP launch.  The per-game path (Reanalyse.reanalyse_game, pinned by fixture G13) is the reference throughout.

  1. the plan on the device = the CPU plan (tests/test_reanalyse_plan_cpu.py's numpy restatement), stream state included;
  2. the observation batch = game_observations of the carrying games, bit for bit, also for games filed on the device;
  3. the store kernel with the fixtures' own values: G17 / G13 targets bit for bit, nothing else touched;
  4. the torch path against the per-game path and G13;
  5. the FC pass: independent of its neighbours, equal to the library's own decode of the library's own logits, within the
     float64 bounds of tests/test_gpu_fc_shapes.py, G13; fresh weights in the flat buffer are used with no further call;
  6. refused shapes and arguments;
  7. the FC pass captured in a graph and replayed;
  8. tools/train_cartpole.py --reanalyse.
Figures of test 5 are collected in measure_out/reanalyse_batch_report.json (MZ_OUT_DIR overrides the place)."""
import copy
import importlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from parity_helpers import (cartpole_model_and_weights, categorical_mean_bound, fc_reference_inference, fc_reference_model,
                            fc_rounding_bounds, history_of, load_golden, support_to_scalar64, synthetic_model,
                            value_transform_bound)
from test_gpu_replay_edges import GARBAGE, device_targets, edge_config, packed_of, synthetic_games
from test_reanalyse_plan_cpu import numpy_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

RTOL, ATOL = 3e-5, 1e-5            # test_gpu_replay.test_reanalyse_values_and_targets: this network in float32 vs G13
NAN_PATTERN = 0x7FC0BEEF           # a quiet NaN with a payload: any float write over it shows
REPORT = {}


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    yield types.SimpleNamespace(rb=importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
                                sp=importlib.import_module("muzero-hypermodel_amd.self_play"),
                                models=importlib.import_module("muzero-hypermodel_amd.models"),
                                engine=importlib.import_module("muzero-hypermodel_amd.engine"),
                                native=importlib.import_module("muzero-hypermodel_amd._native"))
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(ROOT, "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "reanalyse_batch_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


def new_store(mods, config):
    return mods.rb.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)


def cartpole_store(mods):
    fx = load_golden("g13_reanalyse_cartpole")
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    rb = new_store(mods, config)
    for g in range(len(fx["lengths"])):
        rb.save_game(history_of(mods.sp, fx, g))
    return fx, config, rb


def edge_store(mods, name, capacity=None, fill=False):
    fx = load_golden(f"g17_replay_edges_{name}")
    config = edge_config(fx, name)
    if capacity is not None:
        config.replay_buffer_size = capacity
    rb = new_store(mods, config)
    if fill:
        fill_reanalysed_rows(rb)
    if capacity is None:
        rb.save_games(packed_of(mods.sp, fx))
    else:                                                       # the ring wraps: the oldest games are dropped one by one
        for g in range(len(fx["lengths"])):
            rb.save_game(history_of(mods.sp, fx, g))
    return fx, config, rb


def fill_reanalysed_rows(rb):
    """Every float of the store's reanalysed rows becomes NAN_PATTERN (through mzreplay_set_reanalysed with whole rows; the
    games saved afterwards reset the flags and leave the rows alone)."""
    row = torch.full((rb.L,), 0.0, dtype=torch.float32, device=rb.device)
    row.view(torch.int32).fill_(NAN_PATTERN)
    for slot in range(rb.capacity):
        assert rb._lib.mzreplay_set_reanalysed(rb._h, slot, row.data_ptr(), rb.L, rb._stream()) == 0
    torch.cuda.synchronize()


def carrying(ids):
    """(draw, game id) of the draws that carry rows, in row order."""
    last = {int(g): d for d, g in enumerate(ids)}
    return [(d, int(g)) for d, g in enumerate(ids) if last[int(g)] == d]


def plan_arrays(plan):
    torch.cuda.synchronize()
    return plan.game_ids.cpu().numpy(), plan.slots.cpu().numpy(), plan.row_start.cpu().numpy()


def same_state(a, b):
    return a[2] == b[2] and np.array_equal(np.asarray(a[1], dtype=np.uint32), np.asarray(b[1], dtype=np.uint32))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stored_values(rb, ids, lengths_of):
    """{game id: float32 values [length]} and {game id: flag} read back from the store."""
    ids = sorted(set(int(g) for g in ids))
    values, has = rb.download_reanalysed(ids)
    return {g: values[i, : int(lengths_of[g])].copy() for i, g in enumerate(ids)}, dict(zip(ids, has.tolist()))


# ---- 1. the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [None, 5])
def test_plan_on_the_device_equals_the_cpu_plan(mods, capacity):
    fx, config, rb = edge_store(mods, "cartpole_long", capacity)
    G = len(fx["lengths"])
    stored = sorted(rb.buffer)
    oldest, n_stored = stored[0], len(stored)
    assert stored == list(range(G - (capacity or G), G))
    length_of_slot = np.zeros(rb.capacity, dtype=np.int32)
    for g in stored:
        length_of_slot[g % rb.capacity] = fx["lengths"][g]
    rs = np.random.RandomState(config.seed)                     # the pass's own stream: numpy.random.seed(config.seed)
    assert same_state(rb.reanalyse_state(), rs.get_state())
    sampler_before = rb.rng.get_state()
    for n_games in (1, 16, 300, 4096, 7):                       # each pass continues the stream; 4096 crosses regenerations
        got_ids, got_slots, got_start = plan_arrays(rb.reanalyse_plan(n_games))
        want_ids = oldest + np.array([int(rs.choice(n_stored)) for _ in range(n_games)], dtype=np.int64)
        slots, row_start, _, _ = numpy_plan(want_ids, oldest, rb.capacity, length_of_slot)
        assert np.array_equal(got_ids, want_ids), n_games
        assert np.array_equal(got_slots, slots) and np.array_equal(got_start, row_start), n_games
        assert same_state(rb.reanalyse_state(), rs.get_state()), n_games
    # ids handed in: nothing is drawn
    pick = np.random.RandomState(1)
    for n_games in (1, 9, 64, 4096):
        ids = oldest + pick.randint(0, n_stored, n_games)
        got_ids, got_slots, got_start = plan_arrays(rb.reanalyse_plan(n_games, ids))
        slots, row_start, _, _ = numpy_plan(ids, oldest, rb.capacity, length_of_slot)
        assert np.array_equal(got_ids, ids) and np.array_equal(got_slots, slots) and np.array_equal(got_start, row_start)
        assert same_state(rb.reanalyse_state(), rs.get_state())
    assert same_state(rb.rng.get_state(), sampler_before)       # the buffer's host stream never moved
    rb.close()


def test_plan_of_a_single_game_and_of_an_empty_store(mods):
    fx, config, rb = edge_store(mods, "cartpole_long", capacity=1)      # one stored game: choice(1) consumes no word
    before = rb.reanalyse_state()
    ids, slots, row_start = plan_arrays(rb.reanalyse_plan(5))
    last = len(fx["lengths"]) - 1
    assert ids.tolist() == [last] * 5 and slots.tolist() == [0] * 5
    assert row_start.tolist() == [0, 0, 0, 0, 0, int(fx["lengths"][last])]
    assert same_state(rb.reanalyse_state(), before)
    rb.close()
    config = edge_config(fx, "cartpole_long")
    empty = new_store(mods, config)
    before = empty.reanalyse_state()
    ids, slots, row_start = plan_arrays(empty.reanalyse_plan(8))
    assert (ids == -1).all() and (slots == -1).all() and (row_start == 0).all()
    assert same_state(empty.reanalyse_state(), before)
    re = mods.rb.Reanalyse({"weights": mods.models.MuZeroNetwork(config).get_weights()}, config)
    assert re.reanalyse_games(empty, 8) == 8 and re.num_reanalysed_games == 8      # counts, draws nothing
    assert same_state(empty.reanalyse_state(), before)
    empty.close()


# ---- 2. the observation batch -----------------------------------------------------------------------------------------
def assert_observations(rb, ids, where):
    plan = rb.reanalyse_plan(len(ids), ids)
    got = rb.reanalyse_observations(plan).cpu().numpy()
    want = np.concatenate([rb.game_observations(g).cpu().numpy() for _, g in carrying(ids)])
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), where
    return got


@pytest.mark.parametrize("name", ["g13", "tictactoe_td3", "cartpole_long"])
def test_observation_batch_is_the_games_observations_in_row_order(mods, name):
    fx, config, rb = cartpole_store(mods) if name == "g13" else edge_store(mods, name)
    G = len(fx["lengths"])
    rs = np.random.RandomState(2)
    for ids in (list(range(G)), list(range(G))[::-1], [G - 1], rs.randint(0, G, 40).tolist(), [0, 0, 0]):
        got = assert_observations(rb, ids, (name, ids))
        if name != "g13" and ids == list(range(G)):
            assert np.array_equal(got, fx["stacked"])           # the reference's own stacked observations, every position
    rb.close()


def test_observation_batch_of_games_filed_on_the_device(mods):
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    config.max_moves, config.replay_buffer_size = 12, 4096
    torch.manual_seed(0)
    weights = mods.models.MuZeroNetwork(config).get_weights()
    rb = new_store(mods, config)
    actor = mods.sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 11, 64)
    actor.file_to(rb)
    for m in (7, 16):
        actor.play_moves(m, 1.0, on_games=lambda batch: None, temperature_threshold=0)
    actor.flush(on_games=lambda batch: None)
    actor.close()
    stored = sorted(rb.buffer)
    assert len(stored) >= 64 and all(rb.buffer[g]["history"] is None for g in stored)   # they never existed on the host
    ids = np.random.RandomState(4).choice(stored, 50).tolist()
    got = assert_observations(rb, ids, "filed games")
    games = [g for _, g in carrying(ids)]
    packed = rb.download_games(games)
    want = np.concatenate([packed.observations[i, : packed.length[i]] for i in range(len(games))])
    assert np.array_equal(got.reshape(len(want), -1), want.reshape(len(want), -1))      # (stacked_observations = 0)
    # and a drawn plan over them stays inside the stored ids
    plan = rb.reanalyse_plan(200)
    drawn, _, row_start = plan_arrays(plan)
    assert set(drawn.tolist()) <= set(stored)
    assert row_start[-1] == sum(rb.buffer[g]["length"] for g in set(drawn.tolist()))
    rb.close()


# ---- 3. the store kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tictactoe_td3", "connect4_td5", "cartpole_long", "cartpole_alpha1"])
def test_store_writes_the_carrying_games_and_nothing_else(mods, name):
    fx, config, rb = edge_store(mods, name, fill=True)
    lengths, pairs, U1 = fx["lengths"], fx["pairs"], config.num_unroll_steps + 1
    G = len(lengths)
    flagged = np.flatnonzero(fx["has_reanalysed"]).tolist()
    ids = flagged + flagged[::2] + flagged[:1]                  # ONE pass, duplicates among the ids
    plan = rb.reanalyse_plan(len(ids), ids)
    values = np.concatenate([fx["reanalysed"][g, : lengths[g]] for _, g in carrying(ids)]).astype(np.float32)
    assert plan.rows() == len(values)
    rb.reanalyse_store(plan, torch.from_numpy(values).cuda())
    past_end = pairs[:, 1:2] + np.arange(U1)[None, :] > lengths[pairs[:, 0]][:, None]
    absorbing = np.where(past_end, fx["action_targets_after"], GARBAGE).astype(np.int32)
    got = device_targets(rb, [(int(g), int(p)) for g, p in pairs], absorbing)
    assert np.array_equal(got["value"], fx["value_targets_after"])
    untouched = ~np.isin(pairs[:, 0], flagged)
    assert np.array_equal(got["value"][untouched], fx["value_targets_before"][untouched]) and untouched.any()
    rows, has = rb.download_reanalysed(range(G))
    for g in range(G):
        n = int(lengths[g])
        assert bool(has[g]) == (g in flagged), g
        if g in flagged:
            assert np.array_equal(bits(rows[g, :n]), bits(fx["reanalysed"][g, :n])), g
            assert (bits(rows[g, n:]) == NAN_PATTERN).all(), g  # the floats past the game's length keep their bits
        else:
            assert (bits(rows[g]) == NAN_PATTERN).all(), g
    # save_game into a touched slot forgets the values, as today
    rb.save_game(history_of(mods.sp, fx, flagged[0]))
    assert G % rb.capacity == flagged[0] % rb.capacity
    _, has = rb.download_reanalysed([G])
    assert not has[0]
    rb.close()


def test_store_with_g13_values_gives_g13_targets(mods):
    fx, config, rb = cartpole_store(mods)
    G = len(fx["lengths"])
    ids = [5, 0, 1, 2, 5, 3, 4, 0]
    plan = rb.reanalyse_plan(len(ids), ids)
    values = np.concatenate([fx["reanalysed"][g, : fx["lengths"][g]] for _, g in carrying(ids)])
    rb.reanalyse_store(plan, torch.from_numpy(values).cuda())
    out = rb.make_targets(fx["pairs"][:, 0].astype(np.int32), fx["pairs"][:, 1].astype(np.int32),
                          fx["action_targets"].astype(np.int32))
    assert np.array_equal(out["value"].cpu().numpy(), fx["value_targets"])
    assert np.array_equal(out["reward"].cpu().numpy(), fx["reward_targets"])
    assert np.array_equal(out["policy"].cpu().numpy(), fx["policy_targets"])
    rb.close()


# ---- 4. the torch path ------------------------------------------------------------------------------------------------
def per_game_values(re, rb, games):
    return {g: re.reanalyse_game(rb, g)[1].cpu().numpy() for g in games}


def test_torch_path_cartpole_against_the_per_game_path_and_g13(mods):
    fx, config, rb = cartpole_store(mods)
    _, weights = cartpole_model_and_weights(mods.models, config, "cpu")
    re = mods.rb.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, config)
    ids = [3, 5, 0, 3, 1, 2, 4, 5]
    plan = rb.reanalyse_plan(len(ids), ids)
    values = re._pass_torch(rb, plan, max_rows=100).cpu().numpy()          # 340 rows in chunks of 100
    got, has = stored_values(rb, ids, fx["lengths"])
    at = 0
    for _, g in carrying(ids):
        n = int(fx["lengths"][g])
        assert np.array_equal(bits(got[g]), bits(values[at: at + n])) and has[g]    # what the pass computed is what is stored
        at += n
    want = per_game_values(re, rb, range(6))
    for g in range(6):
        np.testing.assert_allclose(got[g], want[g], rtol=RTOL, atol=ATOL, err_msg=f"game {g} vs reanalyse_game")
        np.testing.assert_allclose(got[g], fx["reanalysed"][g, : fx["lengths"][g]], rtol=RTOL, atol=ATOL, err_msg=f"game {g} vs G13")
    rb.close()


def test_torch_path_is_taken_for_a_residual_network(mods):
    fx, config, rb = edge_store(mods, "tictactoe_td3")
    assert config.network == "resnet"
    _, weights = synthetic_model(mods.models, config, "cpu")
    re = mods.rb.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, config, max_rows=16)
    G = len(fx["lengths"])
    ids = np.random.RandomState(6).randint(0, G, 30).tolist()
    assert re.reanalyse_games(rb, len(ids), game_ids=ids) == 30 and re.num_reanalysed_games == 30
    assert re._fc_store is None
    got, has = stored_values(rb, range(G), fx["lengths"])
    assert [g for g in range(G) if has[g]] == sorted(set(ids))
    want = per_game_values(re, rb, sorted(set(ids)))
    for g in sorted(set(ids)):
        np.testing.assert_allclose(got[g], want[g], rtol=RTOL, atol=ATOL, err_msg=f"game {g}")
    rb.close()


# ---- 5. the FC pass ---------------------------------------------------------------------------------------------------
# (width of one observation, stacked_observations, encoding_size, support_size, hidden layers of repr / value)
FC_CASES = {
    "obs5_enc5_s10": (5, 0, 5, 10, [], [16]),                   # 5 floats: not a multiple of four
    "obs28_stacked3_enc8_s127": (4, 3, 8, 127, [16], [16]),     # 4 * 7 = 28 floats; F = 255, the widest head admitted
    "obs21_stacked3_enc32_s10": (3, 3, 32, 10, [12], [32, 8]),  # 21 floats; two hidden layers in the value head
    "obs8_enc32_s127": (8, 0, 32, 127, [], [16]),
}
FC_LENGTHS = [1, 20, 7, 13, 2, 20, 5, 9]


def fc_config(width, stacked, enc, support, repr_layers, value_layers):
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    config.observation_shape, config.stacked_observations = (1, 1, width), stacked
    config.action_space, config.players = [0, 1, 2], [0]
    config.network, config.encoding_size, config.support_size = "fullyconnected", enc, support
    config.fc_representation_layers, config.fc_value_layers = list(repr_layers), list(value_layers)
    config.fc_dynamics_layers = config.fc_reward_layers = config.fc_policy_layers = [16]
    config.max_moves, config.replay_buffer_size = max(FC_LENGTHS), len(FC_LENGTHS)
    config.num_simulations = 2
    return config


def fc_setup(mods, case):
    """(config, store, Reanalyse, lengths) for a synthetic FC network on seeded games, or the CartPole checkpoint on G13."""
    if case == "cartpole_checkpoint":
        fx, config, rb = cartpole_store(mods)
        _, weights = cartpole_model_and_weights(mods.models, config, "cpu")
        lengths = fx["lengths"]
    else:
        config = fc_config(*FC_CASES[case])
        rs = np.random.RandomState(len(case))
        arrays = synthetic_games(rs, FC_LENGTHS, config.max_moves, 3, 1, config.observation_shape)
        rb = new_store(mods, config)
        rb.save_games(packed_of(mods.sp, arrays))
        _, weights = synthetic_model(mods.models, config, "cpu", seed=3)
        lengths = arrays["lengths"]
    re = mods.rb.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, config)
    return config, rb, re, lengths


def float64_values(ref, observations, support):
    """(values, bound) of the rows from the float64 network: tests/test_gpu_fc_shapes.py decode_bound -- the logit bound of
    fc_rounding_bounds through categorical_mean_bound into value_transform_bound; any float32 evaluation lies within."""
    value_logits = fc_reference_inference(ref, observations=observations)[0]
    e_value = fc_rounding_bounds(ref, observations=observations)[0]
    want = support_to_scalar64(value_logits, support)
    return want, value_transform_bound(want, categorical_mean_bound(e_value.max(axis=-1), support))


def clear_values(rb, games):
    for g in games:
        rb.set_reanalysed_values(g, np.zeros(rb.buffer[g]["length"], dtype=np.float32))


def fc_pass(rb, re, ids, lengths):
    re.reanalyse_games(rb, len(ids), game_ids=ids)
    assert re._fc_store is not None and re._fc_store[0] is rb, re._fc_refused      # the HIP pass ran, not torch
    return stored_values(rb, ids, lengths)[0]


def library_decode_of_library_logits(mods, config, model, observations, group):
    """support_to_scalar_group<group> (expand_roots_kernel) applied to the value logits mzmcts_fc_initial_inference
    returns for the rows: (float32 values, the logits)."""
    E = len(observations)
    engine = mods.engine.BatchedMCTS(config, E, group_width=group, seeds=list(range(E)))
    try:
        assert engine.group_width() == group
        engine.configure_fused_fc(model)
        engine.set_fused_options("generic")                      # one sequential chain per neuron, as the pass computes it
        v, r, p, h = engine.fc_initial_inference(observations)
        logits = v.cpu().numpy().copy()
        engine.begin_search([list(config.action_space)] * E, [0] * E, False)
        engine.expand_roots(v, r, p, h)
        predicted = engine.readout()["root_predicted_value"].copy()
    finally:
        engine.close()
    assert np.array_equal(predicted.astype(np.float32).astype(np.float64), predicted)
    return predicted.astype(np.float32), logits


@pytest.mark.parametrize("case", ["cartpole_checkpoint"] + list(FC_CASES))
def test_fc_pass(mods, case):
    config, rb, re, lengths = fc_setup(mods, case)
    G, s = len(lengths), config.support_size
    group = rb._lib.mzreplay_reanalyse_fc_group_width()
    ref = fc_reference_model(re.model)                           # float64 copy, before anything re-points the weights
    games = list(range(G))
    # (i) a game's values do not depend on its neighbours, on n_games or on where its rows fall in the grid
    whole = fc_pass(rb, re, games, lengths)
    clear_values(rb, games)
    alone = {}
    for g in games:
        alone.update(fc_pass(rb, re, [g], lengths))
    clear_values(rb, games)
    backwards = fc_pass(rb, re, games[::-1] + games[:3] + [games[-1]] * 5, lengths)
    for g in games:
        assert np.array_equal(bits(whole[g]), bits(alone[g])) and np.array_equal(bits(whole[g]), bits(backwards[g])), g
    got = np.concatenate([whole[g] for g in games]).astype(np.float64)
    assert np.isfinite(got).all()
    observations = torch.cat([rb.game_observations(g) for g in games])
    # (ii) the library's own decode of the library's own logits, bit for bit
    decoded, logits = library_decode_of_library_logits(mods, config, copy.deepcopy(re.model), observations, group)
    assert np.isfinite(logits).all()
    assert np.array_equal(bits(got), bits(decoded)), int((bits(got) != bits(decoded)).sum())
    # (iii) the network in float64 (tests/test_gpu_fc_shapes.py decode_bound)
    obs_np = observations.cpu().numpy()
    want, bound = float64_values(ref, obs_np, s)
    ratio = np.abs(got - want) / bound
    worst = int(ratio.argmax())
    print(f"\n{case}: {len(got)} rows, worst |value - float64| / bound = {ratio[worst]:.4f} "
          f"(error {abs(got[worst] - want[worst]):.3e}, bound {bound[worst]:.3e}, value {want[worst]:.4f})")
    REPORT[case] = dict(rows=len(got), group_width=int(group), worst_error_over_bound=float(ratio[worst]),
                        worst_error=float(np.abs(got - want).max()))
    assert ratio[worst] <= 1.0, (case, worst, float(got[worst]), float(want[worst]), float(bound[worst]))
    # (iv) G13's recorded values
    if case == "cartpole_checkpoint":
        fx = load_golden("g13_reanalyse_cartpole")
        for g in games:
            np.testing.assert_allclose(whole[g], fx["reanalysed"][g, : lengths[g]], rtol=RTOL, atol=ATOL, err_msg=f"game {g}")
    # new weights in the flat buffer (what Trainer.publish does: flat.load_state_dict) are used with no further call
    _, fresh = synthetic_model(mods.models, config, "cpu", seed=8)
    re.flat.load_state_dict(fresh)
    after = fc_pass(rb, re, games, lengths)
    got2 = np.concatenate([after[g] for g in games]).astype(np.float64)
    ref2 = fc_reference_model(re.model)                           # (the model's tensors alias the flat buffer)
    want2, bound2 = float64_values(ref2, obs_np, s)
    assert (np.abs(got2 - want2) <= bound2).all() and not np.array_equal(got2, got)
    REPORT[case]["worst_error_over_bound_after_publish"] = float((np.abs(got2 - want2) / bound2).max())
    rb.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,support", [(257, 10), (4, 128)])
def test_refused_shapes_take_the_torch_path(mods, width, support):
    config = fc_config(width, 0, 8, support, [], [16])
    arrays = synthetic_games(np.random.RandomState(9), FC_LENGTHS, config.max_moves, 3, 1, config.observation_shape)
    rb = new_store(mods, config)
    rb.save_games(packed_of(mods.sp, arrays))
    _, weights = synthetic_model(mods.models, config, "cpu", seed=3)
    re = mods.rb.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, config)
    flat = re.flat = importlib.import_module("muzero-hypermodel_amd.weights").FlatWeights(re.model)
    with pytest.raises(RuntimeError, match="mzreplay_reanalyse_fc_configure: layer sizes outside the supported range"):
        rb.reanalyse_fc_configure(flat)
    plan = rb.reanalyse_plan(2, [0, 1])
    with pytest.raises(RuntimeError, match="call mzreplay_reanalyse_fc_configure first"):
        rb.reanalyse_fc(plan)
    games = list(range(len(FC_LENGTHS)))
    assert re.reanalyse_games(rb, len(games), game_ids=games) == len(games)
    assert re._fc_store is None and "layer sizes outside the supported range" in re._fc_refused[1]
    got, has = stored_values(rb, games, arrays["lengths"])
    assert all(has[g] for g in games)
    # Both torch evaluations are float32 runs of this network (a batch of 77 rows may pick another GEMM than a batch of one
    # game), so each lies within the float64 bound of test 5 (iii) -- at support 128 one step of the inverse transform's
    # float32 lattice (1.2e-4 sqrt(|v| + 1), parity_helpers.value_transform_bound) is already beyond rtol 3e-5.
    want, bound = float64_values(fc_reference_model(re.model), torch.cat([rb.game_observations(g) for g in games]).cpu().numpy(),
                                 support)
    per_game = per_game_values(re, rb, games)
    for values in (got, per_game):
        flat_values = np.concatenate([values[g] for g in games]).astype(np.float64)
        assert (np.abs(flat_values - want) <= bound).all(), float((np.abs(flat_values - want) / bound).max())
    rb.close()


def test_refused_arguments(mods):
    fx, config, rb = cartpole_store(mods)
    _, weights = cartpole_model_and_weights(mods.models, config, "cpu")
    re = mods.rb.Reanalyse({"weights": weights}, config)
    for n in (0, -1, 4097):
        with pytest.raises(ValueError, match="1..4096"):
            rb.reanalyse_plan(n)
        with pytest.raises(ValueError, match="1..4096"):
            re.reanalyse_games(rb, n)
        buf = torch.zeros(8, dtype=torch.int64, device="cuda")
        assert rb._lib.mzreplay_reanalyse_plan(rb._h, n, 0, 6, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) != 0
        assert b"n_games must be 1..4096" in rb._lib.mzreplay_last_error(rb._h)
    for bad in ([6], [0, -1], [0, 1, 99]):
        with pytest.raises(RuntimeError, match="is not stored"):
            rb.reanalyse_plan(len(bad), bad)
    with pytest.raises(ValueError, match="n_games ids"):
        rb.reanalyse_plan(3, [0, 1])
    _, has = rb.download_reanalysed(range(6))
    assert not has.any()                                        # nothing was written by the refused calls
    rb.close()


# ---- 7. the FC pass in a graph ----------------------------------------------------------------------------------------
def test_fc_pass_with_drawn_ids_is_capturable(mods):
    config, rb, re, lengths = fc_setup(mods, "cartpole_checkpoint")
    games, n_games = list(range(len(lengths))), 9
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        re.reanalyse_games(rb, n_games)                         # configures the pass, allocates the plan's arrays
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        counted = re.num_reanalysed_games
        with torch.cuda.graph(graph, stream=stream):
            re.reanalyse_games(rb, n_games)
    assert re.num_reanalysed_games == counted + n_games
    torch.cuda.synchronize()
    for seed in (21, 22):
        _, fresh = synthetic_model(mods.models, config, "cpu", seed=seed)
        re.flat.load_state_dict(fresh)                          # new weights published into the flat buffer
        start = rb.reanalyse_state()
        clear_values(rb, games)
        torch.cuda.synchronize()                                # (the copies above ran on another stream)
        with torch.cuda.stream(stream):
            re.reanalyse_games(rb, n_games)
        torch.cuda.synchronize()
        eager_rows, eager_has = rb.download_reanalysed(games)
        eager_state = rb.reanalyse_state()
        eager_ids = rb._reanalyse_plans[n_games].game_ids.cpu().numpy().copy()
        assert not same_state(start, eager_state) and eager_has.any()
        clear_values(rb, games)
        rb.set_reanalyse_state(start)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        rows, has = rb.download_reanalysed(games)
        assert np.array_equal(rb._reanalyse_plans[n_games].game_ids.cpu().numpy(), eager_ids)
        assert np.array_equal(has, eager_has) and np.array_equal(bits(rows), bits(eager_rows)), seed
        assert same_state(rb.reanalyse_state(), eager_state), seed
    rb.close()


# ---- 8. the loop ------------------------------------------------------------------------------------------------------
def test_train_cartpole_with_reanalyse_is_repeatable(mods):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_cartpole.py"), "--envs", "16", "--iterations", "3", "--reanalyse", "8"]
    logs = []
    for _ in range(2):
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert proc.returncode == 0, proc.stderr[-2000:]
        rows = [json.loads(line) for line in proc.stdout.splitlines() if line.startswith("{")]
        for row in rows:
            row.pop("seconds")
        logs.append(rows)
    assert len(logs[0]) == 3 and logs[0] == logs[1]
    assert [row["num_reanalysed_games"] for row in logs[0]] == [8, 16, 24]
