"""Device self-play with config.stacked_observations = n > 0: the device frame stack (include/mzenv.h mzenv_stack_*) behind
every path of DeviceSelfPlay.  The host actor (BatchedSelfPlay, which stacks in Python through
GameHistory.get_stacked_observations) is the reference for step(); step() is the reference for the move batches, as in
tests/test_gpu_envs.py.  Stacked observations are compared bit for bit; games as the existing tests of each path compare
them."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from parity_helpers import synthetic_model
from test_gpu_envs import _assert_same_games, _games_by_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def games(name):
    return importlib.import_module(f"muzero-hypermodel_amd.games.{name}")


@pytest.fixture(scope="module")
def sp(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd.self_play")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def small_fc(config, encoding_size=8):
    config.network, config.encoding_size = "fullyconnected", encoding_size
    config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
    config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
    return config


def stacked_config(name, n, fc=False, **changes):
    config = games(name).MuZeroConfig()
    if fc:
        small_fc(config)
        config.num_simulations = min(config.num_simulations, 20)
    config.stacked_observations = n
    for key, value in changes.items():
        setattr(config, key, value)
    return config


def host_stacked(actor, n):
    return np.stack([np.asarray(gh.get_stacked_observations(-1, n), dtype=np.float32) for gh in actor.histories])


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def assert_same_histories(mine, theirs, shape, where):
    assert len(mine) == len(theirs), where
    for a, b in zip(mine, theirs):
        assert a.action_history == b.action_history and a.to_play_history == b.to_play_history, where
        assert a.reward_history == b.reward_history, where
        assert np.array_equal(np.array(a.child_visits, dtype=float), np.array(b.child_visits, dtype=float)), where
        assert a.root_values == b.root_values, where
        for oa, ob in zip(a.observation_history, b.observation_history):
            assert np.array_equal(np.asarray(oa, dtype=np.float32).reshape(shape), np.asarray(ob).reshape(shape)), where


# ---- 1. host versus device, move by move ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fc,n,use_graph", [("tictactoe", False, 2, False), ("tictactoe", False, 2, True),
                                                 ("twentyone", True, 1, True), ("twentyone", False, 1, False),
                                                 ("simple_grid", False, 8, True)])
def test_device_steps_equal_host_steps_and_stacks(sp, models_mod, name, fc, n, use_graph):
    """DeviceSelfPlay.step plays BatchedSelfPlay.step's games -- actions, rewards, child visits, root values,
    observations -- and before every step and after the last stacked_observation() equals
    histories[e].get_stacked_observations(-1, n) of the host actor for every env.  TicTacToe (its residual network) at
    n = 2, TwentyOne (fully-connected and residual) at n = 1, SimpleGrid at n = 8 with max_moves = 6: no game has more
    than 6 plies, so the stack never fills and the last three frames stay zero by the rules."""
    config = stacked_config(name, n, fc)
    if name == "simple_grid":
        assert config.max_moves == 6
    _, weights = synthetic_model(models_mod, config, "cpu")
    E, moves = 16, 14
    shape = tuple(config.observation_shape)
    host = sp.BatchedSelfPlay({"weights": weights}, games(name).Game, config, 0, E, use_graph=False)
    device = sp.DeviceSelfPlay({"weights": weights}, name, config, 0, E, use_graph=use_graph)
    assert device._stack is not None and device._stack.n == n
    done = {"host": {}, "device": {}}
    seen = []
    for move in range(moves + 1):
        want = host_stacked(host, n)
        got = device.stacked_observation()
        assert tuple(got.shape) == (E, shape[0] + n * (shape[0] + 1)) + shape[1:]
        assert same_bits(got, want), move
        seen.append(want)
        if move < moves:
            host.step(1.0, None, on_game=lambda e, gh: done["host"].setdefault(e, []).append(gh))
            device.step(1.0, None, on_game=lambda e, gh: done["device"].setdefault(e, []).append(gh))
    host.close()
    device.close()
    assert set(done["host"]) == set(done["device"]) and len(done["host"]) >= E // 2
    for e in done["host"]:
        assert_same_histories(done["device"][e], done["host"][e], shape, (name, e))
    seen = np.stack(seen)
    c = shape[0]
    assert seen[:, :, c:].any()                                       # previous frames were there to be compared
    if name == "simple_grid":
        lengths = [len(g.action_history) - 1 for gs in done["device"].values() for g in gs]
        assert max(lengths) == 6 and not seen[:, :, c + 5 * (c + 1):].any() and seen[:, :, c + 4 * (c + 1): c + 5 * (c + 1)].any()


# ---- 2. play_moves versus step() ----------------------------------------------------------------------------------------
def batches_equal_steps(sp, factory, total, sizes, temperature=1.0, threshold=None, at_least=1, want_stall=False,
                        variants=None, loop=False):
    """The games `sizes` batches (with one step() mixed in after the second) file equal the games `total` steps file; where
    every env played every move the two actors also end with the same stacked observation.  `loop` (the pre-drawn form,
    where an env may come back with fewer moves than the batch): batches of sizes[0] until every env has played `total`
    moves; the games both runs finished are compared."""
    loop = loop or want_stall
    ends = {}

    def by_step(actor, on_games):
        for _ in range(total):
            actor.step(temperature, threshold, on_games=on_games)
        ends["step"] = actor.stacked_observation().cpu().numpy()
        if variants is not None:
            variants.append(actor.engine.fused_variant())

    def by_batches(actor, on_games):
        E = actor.E
        played = np.zeros(E, np.int64)
        stalled = False
        if loop:
            while played.min() < total:
                got = actor.play_moves(sizes[0], temperature, on_games=on_games, temperature_threshold=threshold)
                stalled |= bool((got < sizes[0]).any())
                played += got
            assert stalled or not want_stall, "no env left the pre-drawn path: action = -1 was never pushed"
            if (played == total).all():
                ends["batch"] = actor.stacked_observation().cpu().numpy()
        else:
            for i, size in enumerate(sizes):
                played += actor.play_moves(size, temperature, on_games=on_games, temperature_threshold=threshold)
                if i == 1:
                    actor.step(temperature, threshold, on_games=on_games)      # the two forms mix: same stack
                    played += 1
            assert (played == total).all(), played
            ends["batch"] = actor.stacked_observation().cpu().numpy()
        actor.flush(on_games=on_games)
        if variants is not None:
            variants.append(actor.engine.fused_variant())

    want, _ = _games_by_env(sp, factory, by_step)
    got, _ = _games_by_env(sp, factory, by_batches)
    E = factory.E
    if loop:
        # the envs may have stopped at different plies: compare the games both runs finished
        compared = 0
        for e in range(E):
            for x, y in zip(want.get(e, []), got.get(e, [])):
                assert x.action_history == y.action_history and x.reward_history == y.reward_history, e
                assert np.array_equal(np.array(x.child_visits), np.array(y.child_visits)) and x.root_values == y.root_values, e
                assert all(np.array_equal(p, q) for p, q in zip(x.observation_history, y.observation_history)), e
                compared += 1
        assert compared >= at_least, compared
        if "batch" in ends:
            assert same_bits(ends["batch"], ends["step"])
    else:
        _assert_same_games(want, got, E, at_least=at_least)
        assert same_bits(ends["batch"], ends["step"])
    assert ends["step"][:, factory.C:].any()


def actor_factory(sp, name, config, weights, E, use_graph=True):
    def factory():
        actor = sp.DeviceSelfPlay({"weights": weights}, name, config, 0, E, use_graph=use_graph)
        assert actor._stack is not None
        return actor
    factory.E, factory.C = E, int(config.observation_shape[0])
    return factory


def random_weights(models_mod, config, ties=False):
    torch.manual_seed(0)       # random weights: a poor CartPole player, games end within a couple of dozen moves
    model = models_mod.MuZeroNetwork(config)
    if ties:                   # all-equal priors below the root: the searches break ties with the RNG at every level
        with torch.no_grad():
            for key, prm in model.named_parameters():
                if key.startswith("prediction_policy_network.module.2"):
                    prm.zero_()
    return model.get_weights()


@pytest.mark.parametrize("n", [1, 2])
def test_cartpole_predrawn_batches_equal_steps(sp, models_mod, n, capsys):
    """CartPole, pre-drawn form of the batch (constant legal set, fully-connected network).  The stacked observation is
    (C + n (C + 1)) H W = 9 floats at n = 1 and 14 at n = 2 (four floats of the current frame, five per previous frame).
    fused_variant(), unforced, named "narrow" for width 9 and "generic" for width 14 on an MI355X; the test prints it
    and requires only that a fused whole-move kernel ran and that both actors ran the same one."""
    config = stacked_config("cartpole", n)
    weights = random_weights(models_mod, config)
    variants = []
    factory = actor_factory(sp, "cartpole", config, weights, 32)
    batches_equal_steps(sp, factory, 40, (8,), at_least=16, variants=variants, loop=True)
    assert variants[0] == variants[1] and variants[0] in ("generic", "narrow")
    with capsys.disabled():
        print(f"\n[cartpole stacked {n}: width {4 + 5 * n} floats] fused_variant() = {variants[0]!r}")


def test_cartpole_stalled_envs_push_nothing(sp, models_mod):
    """A network whose priors tie on every level: most envs leave the pre-drawn path after a move or two of a batch, their
    actions read -1 for the rest of it and the env kernels leave them alone; the stack must do the same, or the games
    that follow differ from step()'s."""
    config = stacked_config("cartpole", 2, num_simulations=20)
    weights = random_weights(models_mod, config, ties=True)
    factory = actor_factory(sp, "cartpole", config, weights, 24)
    batches_equal_steps(sp, factory, 30, (4,), at_least=12, want_stall=True)


@pytest.mark.parametrize("n", [2, 6])
def test_tictactoe_fc_device_input_batches_equal_steps(sp, models_mod, n):
    """TicTacToe with a fully-connected network, device-input form, games ending inside the batches; n = 6 is stacked width
    243, the widest the fused kernels admit (256)."""
    config = stacked_config("tictactoe", n, fc=True, temperature_threshold=None)
    assert 27 * (n + 1) + 9 * n == (99 if n == 2 else 243)
    torch.manual_seed(0)
    weights = models_mod.MuZeroNetwork(config).get_weights()
    factory = actor_factory(sp, "tictactoe", config, weights, 32)
    batches_equal_steps(sp, factory, 24, (7, 7, 9), at_least=32)


def test_tictactoe_residual_lockstep_batches_with_threshold_equal_steps(sp, models_mod):
    config = stacked_config("tictactoe", 2, temperature_threshold=4)
    _, weights = synthetic_model(models_mod, config, "cpu")
    factory = actor_factory(sp, "tictactoe", config, weights, 32)
    batches_equal_steps(sp, factory, 18, (5, 7, 5), threshold=4, at_least=32)


@pytest.mark.parametrize("name", ["cartpole", "tictactoe"])
def test_move_limit_clears_the_stack_inside_a_batch(sp, models_mod, name):
    """config.max_moves below the game's own length: the env kernels' limit ends the games inside the batches (both forms
    of the batch), and the next game's stacked observation holds none of the old frames -- as in step(), where the
    host's len(action_history) > max_moves rule is what clears it."""
    if name == "cartpole":
        config = stacked_config("cartpole", 2, max_moves=5, num_simulations=20)
        weights = random_weights(models_mod, config)
    else:
        config = stacked_config("tictactoe", 2, fc=True, max_moves=4, temperature_threshold=None)
        torch.manual_seed(0)
        weights = models_mod.MuZeroNetwork(config).get_weights()
    factory = actor_factory(sp, name, config, weights, 24)
    if name == "cartpole":
        batches_equal_steps(sp, factory, 24, (6,), at_least=3 * 24, loop=True)
    else:
        batches_equal_steps(sp, factory, 23, (7, 6, 9), at_least=3 * 24)


# ---- 3. opponents -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opponent,mzp", [("random", 0), ("expert", 1)])
def test_opponent_plies_enter_the_stack_as_played(sp, models_mod, opponent, mzp):
    """TicTacToe at n = 2 against a scripted opponent: step() and play_moves file the host actor's games, and the stacked
    observation equals the host's after every step and after every batch -- the opponent's plies are in it with the
    action the env kernels played (the search's action of such a ply reads -1)."""
    from test_gpu_opponents import assert_same_games
    n, E, sizes = 2, 16, (1, 4, 9, 4)
    config = stacked_config("tictactoe", n)
    _, weights = synthetic_model(models_mod, config, "cpu")
    total = sum(sizes)
    want = [[] for _ in range(E)]
    stacks = []
    host = sp.BatchedSelfPlay({"weights": weights}, games("tictactoe").Game, config, 40, E, use_graph=False)
    for _ in range(total):
        stacks.append(host_stacked(host, n))
        host.step(0, None, on_game=lambda e, gh: want[e].append(gh), opponent=opponent, muzero_player=mzp)
    stacks.append(host_stacked(host, n))
    host.close()
    assert sum(len(g) for g in want) >= E
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 40, E)
    for move in range(total):
        assert same_bits(actor.stacked_observation(), stacks[move]), move
        actor.step(0, None, on_game=lambda e, gh: got[e].append(gh), opponent=opponent, muzero_player=mzp)
    assert same_bits(actor.stacked_observation(), stacks[total])
    actor.close()
    assert_same_games(got, want, f"{opponent} steps")
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 40, E)
    at = 0
    for size in sizes:
        played = actor.play_moves(size, 0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0,
                                  opponent=opponent, muzero_player=mzp)
        assert (played == size).all()
        at += size
        assert same_bits(actor.stacked_observation(), stacks[at]), at
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    actor.close()
    assert_same_games(got, want, f"{opponent} batches")


# ---- 4. pipelined groups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "batches"])
def test_pipelined_groups_equal_one_actor(sp, models_mod, form):
    """PipelinedDeviceSelfPlay (2 groups, a stack each) at n = 2 plays one actor's games, by step() and by
    play_moves(prefetch=True), and ends with the same stacked observations."""
    config = stacked_config("tictactoe", 2, temperature_threshold=5)
    _, weights = synthetic_model(models_mod, config, "cpu")
    E, size, calls = 32, 5, 3
    ends = {}

    def by_step(actor, on_games):
        for _ in range(size * calls):
            actor.step(1.0, 5, on_games=on_games)
        ends["one"] = actor.stacked_observation().cpu().numpy()

    def pipelined(actor, on_games):
        assert all(a._stack is not None for a in actor.actors) and actor.actors[0]._stack is not actor.actors[1]._stack
        if form == "step":
            for i in range(size * calls):
                actor.step(1.0, 5, on_games=on_games, prefetch=i + 1 < size * calls)
        else:
            played = np.zeros(E, np.int64)
            for i in range(calls):
                played += actor.play_moves(size, 1.0, on_games=on_games, prefetch=i + 1 < calls)
            actor.flush(on_games=on_games)
            assert (played == size * calls).all()
        ends["two"] = actor.stacked_observation().cpu().numpy()

    want, _ = _games_by_env(sp, lambda: sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, E, use_graph=False), by_step)
    got, _ = _games_by_env(sp, lambda: sp.PipelinedDeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, E, groups=2,
                                                                  use_graph=True), pipelined)
    _assert_same_games(want, got, E, at_least=E)
    assert same_bits(ends["two"], ends["one"]) and ends["one"][:, 3:].any()


# ---- 5. device filing ---------------------------------------------------------------------------------------------------
def test_cartpole_stacked_games_filed_on_the_device(sp, models_mod):
    """CartPole at n = 2: file_to a store of 8 games that wraps; the store is byte-equal to its on_games -> save_games
    twin (plain observations are what is filed), and the observations of a sampled batch -- stacked by the store -- equal
    oracle/replay_oracle.py stacked_observations of the filed games."""
    from test_gpu_replay_filer import assert_same_stores, close_all, twin_run
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    ro = importlib.import_module("replay_oracle")
    config = stacked_config("cartpole", 2, max_moves=9, td_steps=3, replay_buffer_size=8, batch_size=16, num_simulations=20)
    weights = random_weights(models_mod, config)
    a, b, aa, ab, _ = twin_run((rb_mod, sp, models_mod), "cartpole", config, weights, 16, (5, 7, 4, 6))
    assert ab._stack is not None and b.num_played_games > 2 * b.capacity
    assert assert_same_stores(a, b, "cartpole stacked", False) > 20
    ids = list(b.buffer)
    stored = b.download_games(ids)
    index_batch, batch = b.get_batch()
    observations = batch[0].cpu().numpy()
    deep = 0
    for row, (game_id, position) in enumerate(index_batch):
        i = ids.index(game_id)
        length = int(stored.length[i])
        game = types.SimpleNamespace(observations=stored.observations[i, : length + 1], actions=stored.actions[i, : length + 1])
        want = np.asarray(ro.stacked_observations(game, position, 2), dtype=np.float32)
        assert same_bits(observations[row].astype(np.float32).reshape(want.shape), want), (game_id, position)
        deep += position >= 2
    assert deep > 0                                                   # some sampled position has both previous frames
    close_all(aa, ab, a, b)


# ---- 6. n = 0 and the rest ------------------------------------------------------------------------------------------------
def test_without_stacking_the_actor_holds_no_stack(sp, models_mod):
    config = games("tictactoe").MuZeroConfig()
    assert config.stacked_observations == 0
    _, weights = synthetic_model(models_mod, config, "cpu")
    actor = sp.DeviceSelfPlay({"weights": weights}, "tictactoe", config, 0, 8, use_graph=False)
    assert actor._stack is None and actor._stacked is None and actor._stack_ring is None
    for _ in range(2):
        plain = actor.stacked_observation()
        assert tuple(plain.shape) == (8, 3, 3, 3)
        assert np.array_equal(plain.cpu().numpy(), actor.envs.observe()[0].cpu().numpy())
        actor.step(1.0, None)
    actor.play_moves(3, 1.0)
    assert actor._stack_ring is None and tuple(actor.stacked_observation().shape) == (8, 3, 3, 3)
    actor.flush()
    actor.close()


def test_evaluate_runs_stacked_games(sp, models_mod):
    """evaluate() (MuZero.test on device envs) needs no code of its own: against the expert at n = 2 it plays the games
    consecutive play_games of one worker play -- here: the same result from 1 env and from the batch form of 4 envs'
    first games is not required, only that both run and count their games."""
    config = stacked_config("tictactoe", 2)
    _, weights = synthetic_model(models_mod, config, "cpu")
    out = sp.evaluate({"weights": weights}, "tictactoe", config, 6, opponent="expert", muzero_player=1, num_envs=4, seed=3)
    assert out["games"] == 6 and 0 < out["searched_moves"] < out["env_moves"]
