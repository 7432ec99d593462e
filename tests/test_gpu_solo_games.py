"""TwentyOne and SimpleGrid as device-resident environments (include/mzenv.h ids 5 and 6; csrc/solo_rules.h): the env
kernels against fixture G23 and against the host plugins, skipped turns, the move limit, refusals, and the two games
through device self-play, move batches and device filing.  Every comparison is on integers or integer-valued floats and
is exact."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import synthetic_model
from solo_cases import GAMES, OBS_SHAPE, grid_obs, play_host, plugin, t21_obs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd.games.device")


def play_device(dev, name, seeds, actions, max_moves=0, path="advance"):
    """The device envs driven like solo_cases.play_host, returning the same arrays.  path "advance": one mzenv_advance
    per ply; "step": mzenv_step, mzenv_observe, mzenv_reset with the done mask, mzenv_observe."""
    actions = np.asarray(actions)
    E, T = actions.shape
    shape = OBS_SHAPE[name]
    envs = dev.DeviceEnvs(name, E, seeds=list(seeds))
    assert (envs.A, envs.players, envs.observation_shape) == (2, 1, shape) and envs.constant_legal_actions
    if max_moves:
        envs.set_max_moves(max_moves)
    cuda = envs.device
    acts = torch.from_numpy(np.ascontiguousarray(actions.T, dtype=np.int32)).to(cuda)
    obs_after = torch.zeros((T, E) + shape, dtype=torch.float32, device=cuda)
    obs_next = torch.zeros((T, E) + shape, dtype=torch.float32, device=cuda)
    reward = torch.zeros((T, E), dtype=torch.float32, device=cuda)
    done = torch.zeros((T, E), dtype=torch.uint8, device=cuda)
    moves = torch.zeros((T, E), dtype=torch.int32, device=cuda)
    first, legal, num_legal, to_play = envs.observe()
    first = first.clone()
    assert legal.cpu().tolist() == [[0, 1]] * E and num_legal.cpu().tolist() == [2] * E and to_play.cpu().tolist() == [0] * E
    for t in range(T):
        if path == "advance":
            envs.advance(acts[t], reward[t], done[t], obs_after[t], obs_next[t])
        else:
            envs.step(acts[t], reward=reward[t], done=done[t])
            envs.observe(obs_after[t])
            envs.reset(done[t])
            envs.observe(obs_next[t])
        moves[t] = envs.game_moves()
    assert envs.legal.cpu().tolist() == [[0, 1]] * E and envs.num_legal.cpu().tolist() == [2] * E
    assert envs.to_play.cpu().tolist() == [0] * E
    out = dict(first=first.cpu().numpy(), obs_after=obs_after.cpu().numpy(), obs_next=obs_next.cpu().numpy(),
               reward=reward.cpu().numpy(), done=done.cpu().numpy(), moves=moves.cpu().numpy())
    envs.close()
    return out


def assert_same_play(got, want, what):
    for key in ("first", "reward", "done", "obs_after", "obs_next", "moves"):
        same = got[key] == want[key]
        assert same.all(), (what, key, np.argwhere(~same)[:4].tolist())


def test_device_twentyone_replays_g23(dev, golden):
    """64 envs x 400 plies through advance: every observation after the move, observation the next search sees, reward,
    done and game_moves equals the recording of the reference's Game(e) -- the later cards prove the stream position
    after the constructor's two cards, every rejected word and every regeneration (each stream passes 1000 words)."""
    fx = dict(golden("g23_twentyone_env"))
    got = play_device(dev, "twentyone", fx["seed"], fx["action"])
    done = fx["done"].T != 0
    want = dict(first=t21_obs(fx["first_hands"]), obs_after=t21_obs(fx["hands"].transpose(1, 0, 2)),
                obs_next=t21_obs(fx["next_hands"].transpose(1, 0, 2)), reward=fx["reward"].T.astype(np.float32),
                done=done.astype(np.uint8), moves=np.where(done, 0, fx["ply"].T))
    assert done.sum() > 10000 and (fx["words"].sum(axis=1) + fx["reset_words"].sum(axis=1) > 1000).all()
    assert_same_play(got, want, "g23")


def test_device_simple_grid_replays_g23(dev, golden):
    """Env s plays sequence s of the fixture (all 2^6 six-ply walks and the illegal moves along the bottom row); an env
    whose sequence is over is left alone with action -1."""
    fx = dict(golden("g23_simple_grid_env"))
    S, T = len(fx["length"]), int(fx["length"].max())
    actions = np.full((S, T), -1, np.int32)
    actions[fx["seq"], fx["step"] - 1] = fx["action"]
    got = play_device(dev, "simple_grid", np.arange(S), actions)
    s, t = fx["seq"], fx["step"] - 1
    assert np.array_equal(got["obs_after"][t, s], grid_obs(fx["row"], fx["col"]))
    assert np.array_equal(got["reward"][t, s], fx["reward"]) and np.array_equal(got["done"][t, s], fx["done"])
    assert np.array_equal(got["moves"][t, s], np.where(fx["done"] != 0, 0, fx["step"]))
    assert_same_play(got, play_host("simple_grid", np.arange(S), actions), "g23 sequences")


@pytest.mark.parametrize("path", ["step", "advance"])
@pytest.mark.parametrize("name", GAMES)
def test_device_envs_equal_host_plugins(dev, name, path):
    """300 envs (one full 256-thread block and a partial one: envs 255 and 256 sit on the block edge) x 60 random plies,
    through step + reset(done mask) + observe and, with the same seeds, through advance."""
    E, T = 300, 60
    actions = np.random.RandomState(5).randint(0, 2, size=(E, T))
    seeds = 1000 + np.arange(E)
    want = play_host(name, seeds, actions)
    assert want["done"].sum() > E
    assert_same_play(play_device(dev, name, seeds, actions, path=path), want, (name, path))


@pytest.mark.parametrize("name", GAMES)
def test_negative_actions_leave_an_env_untouched(dev, name):
    """Every third env gets action -1 for five plies: it draws nothing and counts nothing (reward 0, done 0, the same
    observation, game_moves unchanged), and afterwards continues exactly like a host game that skipped those turns."""
    E, T = 48, 40
    actions = np.random.RandomState(6).randint(0, 2, size=(E, T))
    actions[::3, 7:12] = -1
    seeds = 50 + np.arange(E)
    want = play_host(name, seeds, actions)
    got = play_device(dev, name, seeds, actions)
    assert_same_play(got, want, name)
    skipped = (actions < 0).T
    assert (got["reward"][skipped] == 0).all() and (got["done"][skipped] == 0).all()
    assert np.array_equal(got["obs_after"][7:12, ::3], got["obs_next"][6:11, ::3])
    assert np.array_equal(got["moves"][7:12, ::3], np.repeat(got["moves"][6:7, ::3], 5, axis=0))


def test_simple_grid_ends_at_the_move_limit(dev):
    """set_max_moves(6), the config's: an env dawdling on illegal moves ends at ply 6 with reward 0 and is reset; a walk
    that reaches the goal earlier ends there with reward 10."""
    actions = np.zeros((4, 14), np.int32)
    actions[1, :] = 1
    actions[2, :] = [0, 1] * 7
    actions[3, :] = [1, 1, 1, 0, 0, 0, 0] * 2
    got = play_device(dev, "simple_grid", np.arange(4), actions, max_moves=6)
    assert_same_play(got, play_host("simple_grid", np.arange(4), actions, max_moves=6), "limit 6")
    assert got["done"][:, 0].tolist() == [0, 0, 0, 0, 0, 1] * 2 + [0, 0] and (got["reward"][:, :2] == 0).all()
    assert np.array_equal(got["obs_after"][5, 0], grid_obs(2, 0)) and np.array_equal(got["obs_next"][5, 0], grid_obs(0, 0))
    assert got["moves"][:, 1].tolist() == [1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 0, 1, 2]
    assert got["done"][:, 2].tolist() == [0, 0, 0, 1] * 3 + [0, 0] and got["reward"][3, 2] == 10
    assert got["done"][:5, 3].tolist() == [0, 0, 0, 0, 1] and got["reward"][4, 3] == 10      # (its third "right" was a no-op)


def test_twentyone_hit_ended_by_the_move_limit_is_no_stand(dev):
    """set_max_moves(1): a hit that neither busts nor reaches 21 reports done with reward 0, its terminal observation
    keeps the dealer's hand (the dealer did not play, no word was drawn for it), and the next game's cards are the
    host's, played under the same rule."""
    E, T = 64, 50
    actions = np.random.RandomState(7).randint(0, 2, size=(E, T))
    seeds = 300 + np.arange(E)
    got = play_device(dev, "twentyone", seeds, actions, max_moves=1)
    assert_same_play(got, play_host("twentyone", seeds, actions, max_moves=1), "limit 1")
    assert (got["done"] == 1).all() and (got["moves"] == 0).all()
    before = np.concatenate([got["first"][None], got["obs_next"][:-1]])            # the position each ply started from
    player = got["obs_after"][:, :, 0, 0, 0]
    limited = (actions.T == 0) & (player < 21)
    assert limited.sum() > 500
    assert np.array_equal(got["obs_after"][limited][:, 1], before[limited][:, 1]) and (got["reward"][limited] == 0).all()


@pytest.mark.parametrize("name", GAMES)
def test_refusals(dev, name):
    envs = dev.DeviceEnvs(name, 4)
    with pytest.raises(NotImplementedError, match="one-player"):
        envs.set_opponent("random", 0, engine=None)
    with pytest.raises(NotImplementedError, match="no board"):
        envs.set_boards(np.zeros((4, 9), np.int8), np.ones(4, np.int8))
    envs.set_opponent("self")
    # the C ABI says the same to a caller that does not come through DeviceEnvs
    key = torch.zeros((4, 624), dtype=torch.int32, device=envs.device)
    pos = torch.zeros(4, dtype=torch.int32, device=envs.device)
    assert envs._lib.mzenv_set_opponent(envs._h, 2, 0, key.data_ptr(), pos.data_ptr()) == -1
    assert b"one-player game has no opponent" in envs._lib.mzenv_last_error(envs._h)
    boards, players = np.zeros((4, 9), np.int8), np.ones(4, np.int8)
    assert envs._lib.mzenv_set_boards(envs._h, boards.ctypes.data, players.ctypes.data) == -1
    assert b"not a board game" in envs._lib.mzenv_last_error(envs._h)
    envs.close()


# ---- self-play ----------------------------------------------------------------------------------------------------------
def mods():
    return (importlib.import_module("muzero-hypermodel_amd.self_play"), importlib.import_module("muzero-hypermodel_amd.models"))


def solo_config(name, network=None):
    config = plugin(name).MuZeroConfig()
    if network is not None:
        config.network = network
    return config


@pytest.mark.parametrize("name,network", [("twentyone", "fullyconnected"), ("twentyone", "resnet"), ("simple_grid", None)])
def test_device_self_play_equals_host_env_self_play(dev, pkg, name, network):
    """DeviceSelfPlay.step x 12 (16 envs on the GPU) plays the games BatchedSelfPlay plays with the host plugins:
    actions, rewards, child-visit targets, root values and observations.  TwentyOne with its config switched to a
    fully-connected network and with its own residual network, SimpleGrid with its own config (games end at its
    max_moves = 6 where they dawdle)."""
    sp, models_mod = mods()
    config = solo_config(name, network)
    _, weights = synthetic_model(models_mod, config, "cpu")
    E, moves = 16, 12
    out = {}
    for kind in ("host", "device"):
        games_done = {}
        if kind == "host":
            actor = sp.BatchedSelfPlay({"weights": weights}, plugin(name).Game, config, 0, E, use_graph=False)
        else:
            actor = sp.DeviceSelfPlay({"weights": weights}, name, config, 0, E, use_graph=False)
        for _ in range(moves):
            actor.step(1.0, None, on_game=lambda e, gh: games_done.setdefault(e, []).append(gh))
        actor.close()
        out[kind] = games_done
    assert set(out["host"]) == set(out["device"]) and len(out["host"]) == E
    for e in out["host"]:
        assert len(out["host"][e]) == len(out["device"][e])
        for a, b in zip(out["host"][e], out["device"][e]):
            assert a.action_history == b.action_history and a.to_play_history == b.to_play_history
            assert a.reward_history == b.reward_history
            assert np.array_equal(np.array(a.child_visits, dtype=float), np.array(b.child_visits, dtype=float))
            assert a.root_values == b.root_values
            for oa, ob in zip(a.observation_history, b.observation_history):
                assert np.array_equal(np.asarray(oa, dtype=np.float32).reshape(OBS_SHAPE[name]), ob)
    if name == "simple_grid":
        lengths = [len(g.action_history) - 1 for gs in out["device"].values() for g in gs]
        assert max(lengths) == config.max_moves == 6


@pytest.mark.parametrize("name", GAMES)
def test_move_batches_equal_move_by_move(dev, pkg, name, capsys):
    """play_moves(6) x 3 files the games 18 step()s file, at the games' own max_moves, with fully-connected networks
    (constant legal sets: CartPole's pre-drawn batches).  For SimpleGrid's own network (9 -> 16 -> 5) the fused kernel
    the engine picks is recorded, not forced."""
    from test_gpu_envs import _assert_same_games, _games_by_env
    sp, models_mod = mods()
    config = solo_config(name, "fullyconnected")
    _, weights = synthetic_model(models_mod, config, "cpu")
    E = 16
    variants = []

    def factory():
        actor = sp.DeviceSelfPlay({"weights": weights}, name, config, 0, E)
        assert actor.engine._fc_model is actor.model and actor.envs.constant_legal_actions
        return actor

    def by_step(actor, on_games):
        for _ in range(18):
            actor.step(1.0, None, on_games=on_games)
        variants.append(actor.engine.fused_variant())

    def by_batches(actor, on_games):
        played = np.zeros(E, np.int64)
        for _ in range(3):
            played += actor.play_moves(6, 1.0, on_games=on_games)
        actor.flush(on_games=on_games)
        assert (played == 18).all()
        variants.append(actor.engine.fused_variant())
        assert actor.envs.max_moves == (6 if name == "simple_grid" else 0)       # (21 exceeds TwentyOne's own 20 plies)

    want, n_want = _games_by_env(sp, factory, by_step)
    got, n_got = _games_by_env(sp, factory, by_batches)
    assert n_want == n_got == E * 18
    _assert_same_games(want, got, E, at_least=2 * E)
    assert variants[0] == variants[1] and variants[0] in ("generic", "narrow")     # a fused whole-move kernel ran
    with capsys.disabled():
        print(f"\n[{name}] fused_variant() = {variants[0]!r}")


def test_twentyone_move_batches_filed_on_the_device(dev, pkg):
    """Games filed by file_to(replay_buffer) from TwentyOne move batches equal, byte for byte, the store that
    on_games -> save_games builds: two batches, and a store of 8 games that wraps many times."""
    from test_gpu_replay_filer import assert_same_stores, close_all, twin_run
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp, models_mod = mods()
    config = solo_config("twentyone", "fullyconnected")
    config.replay_buffer_size = 8
    _, weights = synthetic_model(models_mod, config, "cpu")
    a, b, aa, ab, _ = twin_run((rb_mod, sp, models_mod), "twentyone", config, weights, 16, (6, 7))
    assert b.num_played_games > 2 * b.capacity
    assert assert_same_stores(a, b, "twentyone", False) > 8
    close_all(aa, ab, a, b)


@pytest.mark.parametrize("name", GAMES)
def test_evaluate_plays_one_player_test_games(dev, pkg, name):
    """self_play.evaluate with the configs' opponent = None (MuZero.test of a one-player game): 40 games at temperature
    0, played as "self"; the result is the mean total reward, a multiple of 10 / 40 within the games' reward range."""
    sp, models_mod = mods()
    config = solo_config(name)
    assert config.opponent is None
    _, weights = synthetic_model(models_mod, config, "cpu")
    out = sp.evaluate({"weights": weights}, name, config, 40, num_envs=16)
    assert out["games"] == 40 and out["wins"] is None and out["searched_moves"] == out["env_moves"] > 40
    assert -10 <= out["result"] <= 10 and (out["result"] * 4) == int(out["result"] * 4)
    assert 1 <= out["mean_episode_length"] <= (20 if name == "twentyone" else 6)
