"""Paired moves of the environment kernels (include/mzenv.h mzenv_advance_paired) against the kernels they pair up: two
twins of E envs with identical engine streams, one making ONE advance_paired call per move, the other three
advance_opponent calls (MuZero's actions, then twice all -1, which leaves an env on MuZero's turn untouched).  After
every move the twins are compared bit for bit: positions, ply counters, streams, every slot against its call."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, MOVES = 96, 40


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return (importlib.import_module("muzero-hypermodel_amd.games.device"),
            importlib.import_module("muzero-hypermodel_amd.engine"))


class Twin:
    """E envs in opponent mode on the streams of an engine of their own (seeded alike in both twins)."""

    def __init__(self, mods, game, kind, mzp, max_moves):
        dev, engine_mod = mods
        config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
        config.num_simulations = 4                                   # (the engine only lends its streams)
        seeds = [7000 + 3 * e for e in range(E)]
        self.engine = engine_mod.BatchedMCTS(config, E, device="cuda", seeds=seeds)
        self.envs = dev.DeviceEnvs(game, E, seeds=seeds)
        if max_moves:
            self.envs.set_max_moves(max_moves)
        self.envs.set_opponent(kind, mzp, self.engine)
        key, pos = self.engine.rng_streams()
        self.key = engine_mod._device_view(key, E * 624, torch.int32, self.envs.device)
        self.pos = engine_mod._device_view(pos, E, torch.int32, self.envs.device)
        self.obs_next = torch.zeros((E, *self.envs.observation_shape), dtype=torch.float32, device=self.envs.device)

    def state(self):
        """What a twin is: position (from its observation), side to move, ply counters, streams, next search's input."""
        torch.cuda.synchronize()
        envs = self.envs
        obs, legal, num_legal, to_play = (t.cpu().numpy().copy() for t in envs.observe())
        valid = np.arange(envs.A)[None, :] < np.maximum(num_legal, 0)[:, None]
        return dict(board=(obs[:, 0] - obs[:, 1]).reshape(E, -1), player=obs[:, 2].reshape(E, -1)[:, 0],
                    steps=envs.game_moves().cpu().numpy(), key=self.key.cpu().numpy(), pos=self.pos.cpu().numpy(),
                    obs=obs, legal=np.where(valid, legal, -7), num_legal=num_legal, to_play=to_play)

    def close(self):
        self.envs.close()
        self.engine.close()


def paired_call(twin, actions):
    out = twin.envs.new_paired_outputs()
    twin.envs.advance_paired(actions, out["reward"], out["done"], out["obs_after"], twin.obs_next, out["played"], out["words"])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(obs_next=twin.obs_next.cpu().numpy(), num_legal=twin.envs.num_legal.cpu().numpy(),
               legal=twin.envs.legal.cpu().numpy(), to_play=twin.envs.to_play.cpu().numpy())
    return got


def single_calls(twin, actions):
    """Three advance_opponent calls: `actions`, then twice all -1; every call's outputs, stacked like slots."""
    envs, dev = twin.envs, twin.envs.device
    calls = []
    for c in range(3):
        a = actions if c == 0 else torch.full((E,), -1, dtype=torch.int32, device=dev)
        out = dict(reward=torch.zeros(E, dtype=torch.float32, device=dev), done=torch.zeros(E, dtype=torch.uint8, device=dev),
                   obs_after=torch.zeros_like(twin.obs_next), played=torch.zeros(E, dtype=torch.int32, device=dev),
                   words=torch.zeros(E, dtype=torch.int32, device=dev))
        envs.advance(a, out["reward"], out["done"], out["obs_after"], twin.obs_next, played=out["played"], words=out["words"])
        torch.cuda.synchronize()
        calls.append({k: v.cpu().numpy() for k, v in out.items()})
    got = {k: np.stack([c[k] for c in calls]) for k in calls[0]}
    got.update(obs_next=twin.obs_next.cpu().numpy(), num_legal=envs.num_legal.cpu().numpy(), legal=envs.legal.cpu().numpy(),
               to_play=envs.to_play.cpu().numpy())
    return got


def assert_twins_equal(paired, single, where):
    a, b = paired.state(), single.state()
    for name in a:
        assert np.array_equal(a[name], b[name]), (where, name)
    assert (a["num_legal"] > 0).all(), where
    return a


def run_case(mods, game, kind, mzp, max_moves=0, moves=MOVES):
    paired, single = Twin(mods, game, kind, mzp, max_moves), Twin(mods, game, kind, mzp, max_moves)
    dev = paired.envs.device
    try:
        # the settle launch after the fresh reset: exactly the opening, in slot 1, when MuZero plays second
        none = torch.full((E,), -1, dtype=torch.int32, device=dev)
        got, want = paired_call(paired, none), single_calls(single, none)
        assert (got["played"][0] == -1).all() and (got["played"][2] == -1).all()
        assert ((got["played"][1] >= 0) == (mzp == 1)).all()
        for name in ("played", "reward", "done", "obs_after", "words"):
            # (the single-ply twin plays an opening in its FIRST call: the env is on the opponent's turn there)
            assert np.array_equal(got[name][1], want[name][0]), ("settle", name)
        state = assert_twins_equal(paired, single, "settle")
        assert (state["steps"] == mzp).all()
        rs = np.random.RandomState(11 + 2 * mzp + max_moves)
        plies, finished, openings2, held_mid_game = 0, 0, 0, 0
        for m in range(moves):
            pick = (rs.random_sample(E) * state["num_legal"]).astype(np.int64)
            actions = np.where(state["legal"][np.arange(E), pick] >= 0, state["legal"][np.arange(E), pick], 0).astype(np.int32)
            hold = rs.random_sample(E) < 0.08                       # a few envs per move get no action
            hold[rs.randint(E)] = True
            actions[hold] = -1
            held_mid_game += int((hold & (state["steps"] > 1)).sum())
            a_dev = torch.from_numpy(actions).to(dev)
            got, want = paired_call(paired, a_dev), single_calls(single, a_dev.clone())
            for name in ("played", "reward", "done", "obs_after", "words"):
                assert np.array_equal(got[name], want[name]), (m, name)
            assert np.array_equal(got["words"].view(np.uint32).sum(axis=0, dtype=np.uint64),
                                  want["words"].view(np.uint32).sum(axis=0, dtype=np.uint64)), m
            for name in ("obs_next", "num_legal", "to_play"):
                assert np.array_equal(got[name], want[name]), (m, name)
            assert (got["played"][0][hold] == -1).all() and (got["played"][1][hold] == -1).all()
            assert (got["to_play"] == mzp).all() and (got["num_legal"] > 0).all()
            state = assert_twins_equal(paired, single, m)
            assert np.array_equal(state["obs"], got["obs_next"]) and np.array_equal(state["num_legal"], got["num_legal"])
            plies += int((got["played"] >= 0).sum())
            finished += int(got["done"].sum())
            openings2 += int((got["played"][2] >= 0).sum())
        return dict(plies=plies, finished=finished, openings2=openings2, held_mid_game=held_mid_game)
    finally:
        paired.close()
        single.close()


@pytest.mark.parametrize("mzp", [0, 1])
@pytest.mark.parametrize("kind", ["expert", "random"])
@pytest.mark.parametrize("game", ["tictactoe", "connect4"])
def test_paired_launch_equals_three_single_ply_launches(mods, game, kind, mzp):
    stats = run_case(mods, game, kind, mzp)
    assert stats["finished"] > E and stats["held_mid_game"] > 0, stats           # games ended and restarted in every env
    if mzp == 1:
        assert stats["openings2"] > 0, stats                       # a reply ended a game: the next opening came in slot 2


@pytest.mark.parametrize("max_moves", [3, 2])
def test_paired_launch_under_a_move_limit_muzero_second(mods, max_moves):
    """Limit 3: opening, MuZero, reply (limit, reset), opening in slot 2.  Limit 2: opening, MuZero (limit, reset),
    opening in slot 1."""
    stats = run_case(mods, "tictactoe", "expert", 1, max_moves=max_moves)
    assert stats["finished"] > E, stats
    assert (stats["openings2"] > 0) == (max_moves == 3), stats


@pytest.mark.parametrize("mzp", [0, 1])
@pytest.mark.parametrize("serial", [False, True], ids=["wavefront", "one-thread"])
def test_paired_launch_gomoku_both_kernel_forms(mods, monkeypatch, serial, mzp):
    """Gomoku against random on the wavefront-per-env form and on the one-thread-per-env form (MZENV_GOMOKU_SERIAL, read
    at mzenv_create).  Random games do not end within 40 moves: a second run under a move limit ends them by the opponent's
    reply (limit 4 when MuZero is first; 5 when it is second, which brings the next opening into slot 2)."""
    if serial:
        monkeypatch.setenv("MZENV_GOMOKU_SERIAL", "1")
    else:
        monkeypatch.delenv("MZENV_GOMOKU_SERIAL", raising=False)
    stats = run_case(mods, "gomoku", "random", mzp)
    assert stats["plies"] > E * MOVES, stats
    stats = run_case(mods, "gomoku", "random", mzp, max_moves=5 if mzp == 1 else 4, moves=12)
    assert stats["finished"] > E, stats
    if mzp == 1:
        assert stats["openings2"] > 0, stats


def test_paired_launch_refusals(mods):
    dev, _ = mods
    twin = Twin(mods, "tictactoe", "random", 1, max_moves=1)
    none = torch.full((E,), -1, dtype=torch.int32, device=twin.envs.device)
    out = twin.envs.new_paired_outputs()
    args = (out["reward"], out["done"], out["obs_after"], twin.obs_next, out["played"], out["words"])
    with pytest.raises(RuntimeError, match="move limit of 1"):
        twin.envs.advance_paired(none, *args)
    twin.envs.set_max_moves(2)
    twin.envs.advance_paired(none, *args)                          # (the same call, admitted at a limit of 2)
    twin.envs.set_opponent("self")
    with pytest.raises(RuntimeError, match="no opponent is set"):
        twin.envs.advance_paired(none, *args)
    twin.close()
    solo = dev.DeviceEnvs("cartpole", 8)
    out = solo.new_paired_outputs()
    obs_next = torch.zeros((8, *solo.observation_shape), dtype=torch.float32, device=solo.device)
    with pytest.raises(RuntimeError, match="one-player game has no opponent"):
        solo.advance_paired(torch.zeros(8, dtype=torch.int32, device=solo.device), out["reward"], out["done"],
                            out["obs_after"], obs_next, out["played"], out["words"])
    solo.close()
