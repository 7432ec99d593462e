"""Games end at config.max_moves inside the environment kernels: the ply counters and the limit of DeviceEnvs against a
twin env that applies the rule on the host, move batches of DeviceSelfPlay / PipelinedDeviceSelfPlay under a short
max_moves against the per-move paths (step(), BatchedSelfPlay on the host plugins) in self-play and against the scripted
opponents, and the loops (continuous_self_play, evaluate) taking the batched path under a limit."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import cartpole_model_and_weights, synthetic_model
from test_gpu_parity import RESNET_TOL

pytestmark = pytest.mark.gpu

LIMITS = {"cartpole": 7, "tictactoe": 5, "connect4": 9}


def games(name):
    return importlib.import_module(f"muzero-hypermodel_amd.games.{name}")


@pytest.fixture(scope="module")
def dev(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.games.device")


@pytest.fixture(scope="module")
def sp(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.self_play")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def game_config(name, fc=False, max_moves=None):
    config = games(name).MuZeroConfig()
    if fc:
        config.network, config.encoding_size = "fullyconnected", 16
        config.fc_representation_layers, config.fc_dynamics_layers = [], [16]
        config.fc_reward_layers = config.fc_value_layers = config.fc_policy_layers = [16]
        config.num_simulations = min(config.num_simulations, 25)       # (the fused kernel keeps the trees in LDS)
    if max_moves is not None:
        config.max_moves = max_moves
    return config


# ---- the environment kernels alone ----------------------------------------------------------------------------------
class Outputs:
    """The caller's buffers of one DeviceEnvs.advance call."""

    def __init__(self, envs):
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=envs.device)
        self.actions = z(envs.E, dtype=torch.int32)
        self.reward, self.done = z(envs.E), z(envs.E, dtype=torch.uint8)
        self.obs_after, self.obs_next = z(envs.E, *envs.observation_shape), z(envs.E, *envs.observation_shape)

    def advance(self, envs, actions):
        self.actions.copy_(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)))
        envs.advance(self.actions, self.reward, self.done, self.obs_after, self.obs_next)
        torch.cuda.synchronize()
        legal, num_legal = envs.legal.cpu().numpy(), envs.num_legal.cpu().numpy()
        legal[np.arange(envs.A)[None, :] >= num_legal[:, None]] = -1      # (entries past num_legal are whatever was there)
        return {k: getattr(self, k).cpu().numpy() for k in ("reward", "done", "obs_after", "obs_next")} | {
            "legal": legal, "num_legal": num_legal, "to_play": envs.to_play.cpu().numpy()}


def pick_legal(rs, legal, num_legal):
    return np.array([legal[e, rs.randint(num_legal[e])] for e in range(len(num_legal))], dtype=np.int32)


@pytest.mark.parametrize("name", ["cartpole", "tictactoe", "connect4"])
def test_limit_off_is_the_env_without_a_limit(dev, name):
    """set_max_moves(0), a limit set and taken back before the first move, and a limit no game can reach leave every
    output of 600 advance calls what an env that never heard of limits produces."""
    E = 48
    envs = [dev.DeviceEnvs(name, E, seeds=list(range(100, 100 + E))) for _ in range(4)]
    assert all(e.max_moves == 0 for e in envs)
    envs[1].set_max_moves(0)
    envs[2].set_max_moves(3)
    envs[2].set_max_moves(0)
    envs[3].set_max_moves(10 ** 6)
    assert [e.max_moves for e in envs] == [0, 0, 0, 10 ** 6]
    outs = [Outputs(e) for e in envs]
    _, legal, num_legal, _ = (t.cpu().numpy() for t in envs[0].observe())
    rs = np.random.RandomState(4)
    ended = 0
    for call in range(600):
        actions = pick_legal(rs, legal, num_legal)
        got = [o.advance(e, actions) for o, e in zip(outs, envs)]
        for other in got[1:]:
            for k, v in got[0].items():
                assert np.array_equal(v, other[k]), (call, k)
        legal, num_legal = got[0]["legal"], got[0]["num_legal"]
        ended += int(got[0]["done"].sum())
    assert ended >= E                                          # games ended by their own rules, and restarted
    counts = [e.game_moves().cpu().numpy() for e in envs]
    assert all(np.array_equal(counts[0], c) for c in counts[1:]) and counts[0].max() <= envs[0].max_episode_steps
    with pytest.raises(RuntimeError, match="number of plies"):
        envs[0].set_max_moves(-2)
    assert envs[0].max_moves == 0
    for e in envs:
        e.close()


@pytest.mark.parametrize("name", ["cartpole", "tictactoe", "connect4"])
def test_limit_ends_games_like_a_twin_env_with_the_rule_on_the_host(dev, name):
    """E envs with a limit against E twin envs (same seeds, no limit) that are stepped, observed, reset by mask and
    observed again, the limit applied to a host-side count: advance() reports the twin's reward and position, done = the
    game's own end OR the limit, the reset observation of the twin (CartPole: the reset streams stand at the same
    position), the legal sets and player of the position to search next, and game_moves() is the host's count."""
    E, limit = 64, LIMITS[name]
    seeds = list(range(7, 7 + E))
    limited, twin = dev.DeviceEnvs(name, E, seeds=seeds), dev.DeviceEnvs(name, E, seeds=seeds)
    limited.set_max_moves(limit)
    assert twin.max_moves == 0 and limited.max_moves == limit and limited.max_episode_steps == twin.max_episode_steps
    out = Outputs(limited)
    _, legal, num_legal, _ = (t.cpu().numpy() for t in twin.observe())
    limited.observe()
    rs = np.random.RandomState(12)
    count = np.zeros(E, np.int64)
    cut = own = 0
    for call in range(120):
        assert np.array_equal(limited.game_moves().cpu().numpy(), count), call
        actions = pick_legal(rs, legal, num_legal)
        if call % 5 == 3:
            actions[call % E] = -1                              # an env left alone: nothing happens, no ply is counted
        got = out.advance(limited, actions)
        reward, done = twin.step(actions)
        reward, done = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
        after = twin.observe()[0].cpu().numpy()
        count += actions >= 0
        over = done | ((count >= limit) & (actions >= 0))
        cut += int((over & ~done).sum())
        own += int(done.sum())
        twin.reset(torch.from_numpy(over.astype(np.uint8)).to(twin.device))
        nxt, legal, num_legal, to_play = (t.cpu().numpy() for t in twin.observe())
        count[over] = 0
        assert np.array_equal(got["done"].astype(bool), over), call
        assert np.array_equal(got["reward"], reward), call        # the ply's own reward, limit or not
        assert np.array_equal(got["obs_after"], after) and np.array_equal(got["obs_next"], nxt), call
        valid = np.arange(legal.shape[1])[None, :] < num_legal[:, None]
        assert np.array_equal(got["num_legal"], num_legal) and np.array_equal(got["legal"][valid], legal[valid]), call
        assert np.array_equal(got["to_play"], to_play), call
        assert count.max() < limit                               # no game is longer than the limit
    assert cut >= E                                            # the limit did end games the rules would have played on
    if name != "cartpole":
        assert (to_play[count == 0] == 0).all()                # a restarted game is the first player's to open
    if name == "tictactoe":
        assert own > 0                                         # (a line of three is there at ply 5: both endings occur)
    limited.close()
    twin.close()


@pytest.mark.parametrize("name", ["tictactoe", "connect4"])
def test_set_boards_continues_the_game_the_position_came_from(dev, name):
    """A position with k stones handed in counts k plies: with limit k + 2 the game ends two plies later."""
    E = 4
    envs = dev.DeviceEnvs(name, E)
    cells = {"tictactoe": 9, "connect4": 42}[name]
    boards = np.zeros((E, cells), np.int8)
    boards[:, 0], boards[:, 1] = 1, -1                          # bottom row / first row: first player, second player
    boards[3] = 0                                               # env 3: the empty board
    envs.set_boards(boards, np.ones(E, np.int8))
    assert envs.game_moves().cpu().tolist() == [2, 2, 2, 0]
    envs.set_max_moves(4)
    envs.observe()
    out = Outputs(envs)
    got = out.advance(envs, [2, 2, 2, 2])
    assert not got["done"].any() and envs.game_moves().cpu().tolist() == [3, 3, 3, 1]
    got = out.advance(envs, [3, 3, -1, 3])
    assert got["done"].tolist() == [1, 1, 0, 0] and not got["reward"].any()      # no line anywhere: the limit ended them
    assert envs.game_moves().cpu().tolist() == [0, 0, 3, 2]
    assert not got["obs_next"][:2, :2].any() and (got["obs_next"][:2, 2] == 1).all()   # the reset position
    assert got["obs_after"][0, 0].sum() == 2 and got["obs_after"][0, 1].sum() == 2     # the position the ply reached
    # a masked reset zeroes the count of the masked envs only
    envs.reset(torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device=envs.device))
    assert envs.game_moves().cpu().tolist() == [0, 0, 0, 2]
    envs.close()


def test_opponent_plies_count_towards_the_limit(dev):
    """Opponent mode: MuZero second, limit 3 -- the opponent's opening, MuZero's reply and the opponent's second move
    end the game whatever MuZero does; an env on MuZero's turn with action -1 does not count."""
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    E = 8
    engine = engine_mod.BatchedMCTS(game_config("tictactoe"), E, device="cuda", seeds=list(range(E)))
    envs = dev.DeviceEnvs("tictactoe", E)
    envs.set_opponent("random", 1, engine)
    envs.set_max_moves(3)
    envs.observe()
    out = Outputs(envs)
    played = torch.zeros(E, dtype=torch.int32, device=envs.device)
    words = torch.zeros(E, dtype=torch.int32, device=envs.device)

    def advance(actions):
        out.actions.copy_(torch.from_numpy(np.asarray(actions, dtype=np.int32)))
        envs.advance(out.actions, out.reward, out.done, out.obs_after, out.obs_next, played=played, words=words)
        torch.cuda.synchronize()
        return out.done.cpu().numpy(), played.cpu().numpy()

    done, first = advance([-1] * E)                             # the opponent opens: the incoming action is ignored
    assert (first >= 0).all() and not done.any() and envs.game_moves().cpu().tolist() == [1] * E
    assert (envs.num_legal.cpu().numpy() == 8).all()            # MuZero's turn
    reply = np.array([(a + 1) % 9 for a in first], dtype=np.int32)
    reply[0] = -1                                               # env 0 is left alone
    done, got = advance(reply)
    assert not done.any() and np.array_equal(got, reply) and envs.game_moves().cpu().tolist() == [1] + [2] * (E - 1)
    done, got = advance([-1] * E)                               # env 0: still MuZero's turn, untouched; the others: ply 3
    assert done.tolist() == [0] + [1] * (E - 1) and got[0] == -1 and (got[1:] >= 0).all()
    assert envs.game_moves().cpu().tolist() == [1] + [0] * (E - 1)
    assert (envs.num_legal.cpu().numpy()[1:] == 0).all()        # restarted: the opponent opens again
    envs.close()
    engine.close()


# ---- move batches against the per-move paths ------------------------------------------------------------------------
def assert_same_games(got, want, where, limit):
    assert [len(g) for g in got] == [len(g) for g in want], where
    for e, (mine, theirs) in enumerate(zip(got, want)):
        for a, b in zip(mine, theirs):
            assert len(a.action_history) <= limit + 1, (where, e)
            assert a.action_history == b.action_history, (where, e)
            assert a.reward_history == b.reward_history and a.to_play_history == b.to_play_history, (where, e)
            assert [v is None for v in a.root_values] == [v is None for v in b.root_values], (where, e)
            assert np.array_equal(np.array(a.child_visits, dtype=float), np.array(b.child_visits, dtype=float)), (where, e)
            np.testing.assert_allclose([v for v in a.root_values if v is not None], [v for v in b.root_values if v is not None],
                                       rtol=0, atol=RESNET_TOL["value_tol"])
            assert np.array_equal(np.array(a.observation_history), np.array(b.observation_history, dtype=np.float32)), (where, e)


def cut_by_the_limit(name, gh, limit):
    """Did the limit end this game (the game's own rules would have played on)?"""
    if len(gh.action_history) != limit + 1:
        return False
    last = np.asarray(gh.observation_history[-1], dtype=np.float64)
    if name == "cartpole":
        x, theta = last.reshape(-1)[0], last.reshape(-1)[2]
        return abs(x) <= 2.4 and abs(theta) <= 12 * 2 * np.pi / 360
    full = not (last[0] + last[1] == 0).any() if name == "tictactoe" else not (last[0, 5] + last[1, 5] == 0).any()
    return gh.reward_history[-1] == 0 and not full


def count_cut(name, per_env, limit):
    return sum(cut_by_the_limit(name, gh, limit) for env_games in per_env for gh in env_games)


CARTPOLE_SIZES = [1, 16, 7, 16, 16, 7, 16, 1, 16]                # 96 plies: limits fall inside and on the edges of batches


@pytest.mark.parametrize("weights_kind,limit,temperature,threshold,lowered_later", [
    ("trained", 40, 1.0, None, True), ("trained", 40, 0.25, None, False), ("trained", 40, 1.0, 10, False),
    ("random", 12, 1.0, None, False)])
def test_cartpole_batches_under_a_limit_equal_move_by_move(sp, models_mod, weights_kind, limit, temperature, threshold,
                                                           lowered_later):
    """CartPole, fully-connected network (fused whole-move search), 256 envs: play_moves files the games step() files
    under max_moves = 40 (the reference's trained weights: nearly every game is cut) and 12 (random weights: both
    endings), in the pre-drawn form of a batch and, with a temperature threshold, its device-input form; once with
    max_moves lowered on the built actor."""
    E, total = 256, sum(CARTPOLE_SIZES)
    config = game_config("cartpole", max_moves=limit)
    if weights_kind == "trained":
        _, weights = cartpole_model_and_weights(models_mod, config, "cpu")
    else:
        torch.manual_seed(0)
        weights = models_mod.MuZeroNetwork(config).get_weights()
    want = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 3, E)
    for _ in range(total):
        actor.step(temperature, threshold, on_game=lambda e, gh: want[e].append(gh))
    actor.close()
    got = [[] for _ in range(E)]
    built_with = game_config("cartpole") if lowered_later else game_config("cartpole", max_moves=limit)
    actor = sp.DeviceSelfPlay({"weights": weights}, "cartpole", built_with, 3, E)
    assert actor.engine._fc_model is actor.model
    actor.config.max_moves = limit
    for m in CARTPOLE_SIZES:
        played = actor.play_moves(m, temperature, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=threshold or 0)
        assert (played == m).all()
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    assert actor.envs.max_moves == limit and actor.games_finished == sum(len(g) for g in got)
    actor.close()
    assert_same_games(got, want, f"cartpole {weights_kind} T={temperature} threshold={threshold}", limit)
    cut, finished = count_cut("cartpole", got, limit), sum(len(g) for g in got)
    assert finished >= E and cut >= E // 4                     # the limit did end games whose pole was still up
    if weights_kind == "random":
        assert cut < finished                                  # ... and the pole did fall in others


def test_raising_max_moves_on_a_built_actor_is_refused(sp, models_mod):
    config = game_config("cartpole", max_moves=12)
    torch.manual_seed(0)
    weights = models_mod.MuZeroNetwork(config).get_weights()
    actor = sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 0, 8)
    actor.config.max_moves = 13
    with pytest.raises(ValueError, match="history rows hold 12 moves"):
        actor.play_moves(4, 1.0)
    with pytest.raises(ValueError, match="history rows hold 12 moves"):
        actor.step(1.0, None)
    actor.close()


def host_games(sp, weights, game, config, seed, E, n_moves, temperature, opponent="self", mzp=0):
    finished = [[] for _ in range(E)]
    actor = sp.BatchedSelfPlay({"weights": weights}, games(game).Game, config, seed, E, use_graph=False)
    for _ in range(n_moves):
        actor.step(temperature, None, on_game=lambda e, gh: finished[e].append(gh), opponent=opponent, muzero_player=mzp)
    actor.close()
    return finished


BOARD_CASES = [("tictactoe", False, 32), ("tictactoe", True, 64), ("connect4", False, 4), ("connect4", True, 64)]


@pytest.mark.parametrize("game,fc,E", BOARD_CASES)
def test_board_game_batches_under_a_limit_equal_the_host_actor(sp, models_mod, game, fc, E):
    """TicTacToe cut at 5 plies and Connect4 at 9, residual (lock-step) and fully-connected (fused) networks, sampled at
    temperature 1: DeviceSelfPlay.play_moves and PipelinedDeviceSelfPlay.play_moves (2 groups) file, env by env, the games
    BatchedSelfPlay files on the host Game plugins -- whose step() applies len(action_history) > max_moves itself."""
    limit = LIMITS[game]
    config = game_config(game, fc, max_moves=limit)
    _, weights = synthetic_model(models_mod, config, "cpu")
    sizes = [1, 4, 9, 3, 5] if game == "tictactoe" else [1, 4, 9, 4, 9]
    want = host_games(sp, weights, game, config, 21, E, sum(sizes), 1.0)
    assert count_cut(game, want, limit) >= E                   # (the host actor's games: most are cut)
    assert all(len(gh.action_history) <= limit + 1 for g in want for gh in g)
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 21, E)
    for m in sizes:
        played = actor.play_moves(m, 1.0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0)
        assert (played == m).all()
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    actor.close()
    assert_same_games(got, want, f"{game} fc={fc} batches", limit)
    got = [[] for _ in range(E)]
    actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 21, E, groups=2)
    for m in sizes:
        actor.play_moves(m, 1.0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0)
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    assert all(a.envs.max_moves == limit for a in actor.actors)
    actor.close()
    assert_same_games(got, want, f"{game} fc={fc} pipelined", limit)


@pytest.mark.parametrize("game,fc,E", BOARD_CASES)
@pytest.mark.parametrize("opponent,mzp", [("expert", 1), ("random", 0)])
def test_opponent_batches_under_a_limit_equal_the_host_actor(sp, models_mod, game, fc, E, opponent, mzp):
    """Evaluation games under the same short limits (the opponent's plies count): batches of 1, 4 and 9 plies, the
    pipelined actor's batches and single steps -- which used to refuse a short max_moves -- equal the host actor's games."""
    limit = LIMITS[game]
    config = game_config(game, fc, max_moves=limit)
    _, weights = synthetic_model(models_mod, config, "cpu")
    sizes = [1, 4, 9, 4] if game == "tictactoe" else [1, 4, 9, 4, 9]
    n_moves = sum(sizes)
    want = host_games(sp, weights, game, config, 40, E, n_moves, 0, opponent, mzp)
    assert count_cut(game, want, limit) > 0                     # (the rest: somebody had a line by then)
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 40, E)
    for m in sizes:
        played = actor.play_moves(m, 0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0, opponent=opponent,
                                  muzero_player=mzp)
        assert (played == m).all()
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    actor.close()
    assert_same_games(got, want, f"{game} {opponent} batches", limit)
    got = [[] for _ in range(E)]
    actor = sp.PipelinedDeviceSelfPlay({"weights": weights}, game, config, 40, E, groups=2)
    for m in sizes:
        actor.play_moves(m, 0, on_game=lambda e, gh: got[e].append(gh), temperature_threshold=0, opponent=opponent,
                         muzero_player=mzp)
    actor.flush(on_game=lambda e, gh: got[e].append(gh))
    actor.close()
    assert_same_games(got, want, f"{game} {opponent} pipelined", limit)
    got = [[] for _ in range(E)]
    actor = sp.DeviceSelfPlay({"weights": weights}, game, config, 40, E)
    for _ in range(n_moves):
        actor.step(0, None, on_game=lambda e, gh: got[e].append(gh), opponent=opponent, muzero_player=mzp)
    actor.close()
    assert_same_games(got, want, f"{game} {opponent} steps", limit)


# ---- the loops take the fast path -----------------------------------------------------------------------------------
class Storage:
    def __init__(self, weights):
        self.info = {"training_step": 0, "terminate": False, "weights": weights, "num_played_steps": 0}

    def get_info(self, key):
        return self.info[key]

    def set_info(self, keys, values=None):
        self.info.update(keys if isinstance(keys, dict) else {keys: values})


class Replay:
    """Keeps what continuous_self_play saves; ends the loop once `stop_after` games are in."""

    def __init__(self, stop_after):
        self.games, self.stop_after = [], stop_after

    def save_game(self, game_history, shared_storage):
        self.games.append(game_history)
        if len(self.games) >= self.stop_after:
            shared_storage.info["terminate"] = True


def test_continuous_self_play_batches_under_a_limit(sp, models_mod):
    """max_moves = 40 no longer turns the batched pass off: _batchable holds, and the loop with moves_per_pass = 16
    hands the replay buffer the games the per-move loop (moves_per_pass None) hands it."""
    E, limit = 64, 40
    saved = {}
    for moves_per_pass in (None, 16):
        config = game_config("cartpole", max_moves=limit)
        config.ratio = None
        _, weights = cartpole_model_and_weights(models_mod, config, "cpu")
        actor = sp.DeviceSelfPlay({"weights": weights}, "cartpole", config, 5, E)
        assert actor._batchable(1.0, None, 16) and not actor._batchable(1.0, None, None)
        replay = Replay(3 * E)
        actor.continuous_self_play(Storage(weights), replay, False, moves_per_pass=moves_per_pass)
        assert len(replay.games) >= 3 * E
        # (a game is known by its reset observation: every env draws its own from its own stream)
        saved[moves_per_pass] = {np.asarray(gh.observation_history[0], dtype=np.float32).tobytes(): gh for gh in replay.games}
        assert len(saved[moves_per_pass]) == len(replay.games)
    common = sorted(set(saved[None]) & set(saved[16]))
    assert len(common) >= 2 * E
    assert_same_games([[saved[16][k] for k in common]], [[saved[None][k] for k in common]], "continuous_self_play", limit)
    assert count_cut("cartpole", [[saved[16][k] for k in common]], limit) >= E


SAME_KEYS = ("result", "games", "mean_episode_length", "wins", "draws", "losses", "muzero_reward", "opponent_reward")


def test_evaluate_batches_under_a_limit(sp, models_mod):
    """evaluate() with a shortened max_moves: batches of 8 moves return what the per-move path returns (CartPole: step();
    against an opponent: one-move batches, and step() against the opponent)."""
    config = game_config("cartpole", max_moves=40)
    _, weights = cartpole_model_and_weights(models_mod, config, "cpu")
    runs = [sp.evaluate({"weights": weights}, "cartpole", config, 100, num_envs=32, seed=2, moves_per_batch=b) for b in (8, None)]
    for k in SAME_KEYS:
        assert runs[0][k] == pytest.approx(runs[1][k]), k
    assert runs[0]["games"] == 100 and runs[0]["mean_episode_length"] <= 40
    assert runs[0]["mean_episode_length"] > 30                 # (the trained weights: most games reach the limit)
    config = game_config("tictactoe", max_moves=5)
    _, weights = synthetic_model(models_mod, config, "cpu")
    for opponent, mzp in (("expert", 0), ("random", 1)):
        runs = [sp.evaluate({"weights": weights}, "tictactoe", config, 60, opponent=opponent, muzero_player=mzp, num_envs=16,
                            seed=9, moves_per_batch=b) for b in (8, 1, None)]
        for other in runs[1:]:
            for k in SAME_KEYS:
                assert runs[0][k] == pytest.approx(other[k], abs=RESNET_TOL["value_tol"]), (opponent, k)
        assert runs[0]["games"] == 60 and runs[0]["wins"] + runs[0]["draws"] + runs[0]["losses"] == 60
        assert runs[0]["mean_episode_length"] <= 5
