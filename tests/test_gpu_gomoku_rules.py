"""The environment kernels' Gomoku (csrc/env_kernels.hip over csrc/gomoku_rules.h) against fixture G25: one device env
per fixture row, the position handed in by set_boards, then one ply.  Every line of five completed, blocked and left
open, every walk that leaves the board, every overline and the ballot-edge boards through `step` and through `advance`;
the boards a scan without a bottom border would read into, side by side in one workgroup and across two; ragged env
counts; envs left alone between envs that finish; the random opponent's draw at the hand-over between the two 64-cell
ballots; and all of it once more in the one-thread-per-env form.  Rewards, done and legal lists are the reference's;
observation planes and the bookkeeping come from the plain model of gomoku_rules_reference.py, which the CPU suite holds
to the same fixture.  Every comparison is exact, and every output tensor carries a guard row behind the last env."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gomoku_rules_reference as model
from gomoku_rules_cases import (CELLS, COUNTS, EMPTY_SETS, ballot_boards, legal_table, model_plies, observation_planes,
                                picks, plies, rows_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FORMS = ("step", "advance")
CHUNK = 2900                      # envs per launch of the big tests: a few thousand wavefronts


@pytest.fixture(scope="module")
def dev(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module("muzero-hypermodel_amd.games.device")


@pytest.fixture(scope="module")
def eng(pkg):
    return importlib.import_module("muzero-hypermodel_amd.engine")


def masked(legal, num_legal):
    """A device legal table with the entries past each row's count set to -1."""
    return np.where(np.arange(legal.shape[1])[None, :] < num_legal[:, None], legal, -1)


def play_rows(dev, idx, form, sel=None):
    """One env per entry of `idx` (fixture row numbers; a row may occur more than once), set up by set_boards, then one
    ply through `form`; the envs where `sel` is False are handed action -1.  Checked, exactly: before the ply the
    observation, legal table, count, side to move and ply counter of every env; after it reward and done (0 and 0 for
    the envs left alone), the observation (`advance`: obs_after with the terminal boards, obs_next with the fresh ones),
    legal table, count, side to move, ply counter -- and the guard row behind the last env of every output tensor.
    Returns the number of envs compared."""
    ply = plies()
    idx = np.asarray(idx)
    E = len(idx)
    sel = np.ones(E, bool) if sel is None else np.asarray(sel, bool)
    board, player = ply["board"][idx], ply["player"][idx].astype(np.int64)
    planes_before = observation_planes(board, player)
    legal_before, n_before = legal_table(board == 0)
    stones = (board != 0).sum(axis=1).astype(np.int32)
    planes_after = np.where(sel[:, None, None, None], model_plies()[3][idx], planes_before)
    want_reward = np.where(sel, ply["reward"][idx], 0).astype(np.float32)
    want_done = sel & ply["done"][idx]
    now = dict(planes=planes_after.copy(), legal=np.where(sel[:, None], ply["legal"][idx], legal_before),
               n=np.where(sel, ply["n_legal"][idx], n_before), to_play=np.where(sel, player == 1, player == -1).astype(np.int32),
               moves=stones + sel)
    if form == "advance":                                   # a finished env is reset: the fresh position, ply count 0
        now["planes"][want_done] = 0
        now["planes"][want_done, 2] = 1
        now["legal"][want_done], now["n"][want_done] = np.arange(CELLS, dtype=np.int32), CELLS
        now["to_play"][want_done], now["moves"][want_done] = 0, 0

    envs = dev.DeviceEnvs("gomoku", E)
    # every output one row longer than the envs, the extra row a sentinel no kernel may touch
    reward = torch.full((E + 1,), -3.0, dtype=torch.float32, device="cuda")
    done = torch.full((E + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    obs = torch.full((E + 1, 3, 11, 11), -3.0, dtype=torch.float32, device="cuda")
    obs_after, obs_next = obs.clone(), obs.clone()
    envs.legal = torch.full((E + 1, CELLS), -7, dtype=torch.int32, device="cuda")
    envs.num_legal = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    envs.to_play = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    actions = torch.full((E + 1,), 60, dtype=torch.int32, device="cuda")
    actions[:E] = torch.from_numpy(np.where(sel, ply["action"][idx], -1).astype(np.int32)).cuda()

    def check_guards(where):
        assert reward[E].item() == -3.0 and done[E].item() == 0xAB, where
        for t in (obs, obs_after, obs_next):
            assert (t[E] == -3.0).all(), where
        assert (envs.legal[E] == -7).all() and envs.num_legal[E].item() == -7 and envs.to_play[E].item() == -7, where

    def check_position(got_obs, planes, legal, n, to_play, moves, where):
        wrong = np.flatnonzero((got_obs[:E].cpu().numpy() != planes).reshape(E, -1).any(axis=1))
        assert wrong.size == 0, (where, "observation", wrong[:5], idx[wrong[:5]])
        got_n = envs.num_legal[:E].cpu().numpy()
        got_legal = masked(envs.legal[:E].cpu().numpy(), got_n)
        wrong = np.flatnonzero((got_n != n) | (got_legal != legal).any(axis=1))
        assert wrong.size == 0, (where, "legal", wrong[:5], idx[wrong[:5]])
        assert np.array_equal(envs.to_play[:E].cpu().numpy(), to_play), where
        assert np.array_equal(envs.game_moves().cpu().numpy(), moves), where

    envs.set_boards(board, ply["player"][idx])
    envs.observe(obs)
    check_position(obs, planes_before, legal_before, n_before, (player == -1).astype(np.int32), stones, (form, "before"))
    if form == "step":
        envs.step(actions, reward=reward, done=done)
        envs.observe(obs)
        got_obs = obs
    else:
        envs.advance(actions, reward, done, obs_after, obs_next)
        got_obs = obs_next
        wrong = np.flatnonzero((obs_after[:E].cpu().numpy() != planes_after).reshape(E, -1).any(axis=1))
        assert wrong.size == 0, (form, "obs_after", wrong[:5], idx[wrong[:5]])           # terminal boards included
    got_reward, got_done = reward[:E].cpu().numpy(), done[:E].cpu().numpy()
    wrong = np.flatnonzero((got_reward != want_reward) | (got_done != want_done.astype(np.uint8)))
    assert wrong.size == 0, (form, "verdict", wrong[:5], idx[wrong[:5]], got_reward[wrong[:5]], got_done[wrong[:5]])
    check_position(got_obs, now["planes"], now["legal"], now["n"], now["to_play"], now["moves"], (form, "after"))
    check_guards(form)
    envs.close()
    return E


# ---- every ply --------------------------------------------------------------------------------------------------------
def every_ply(dev, form):
    """All rows of the kinds complete, blocked, open, leaving, overline and ballot in launches of CHUNK envs; in the
    `advance` form in a shuffled order, so that a line meets another wavefront of its workgroup and other neighbours."""
    idx = rows_of("complete", "blocked", "open", "leaving", "overline", "ballot")
    assert len(idx) == sum(COUNTS[k] for k in ("complete", "blocked", "open", "leaving", "overline", "ballot")) == 8570
    if form == "advance":
        idx = np.random.RandomState(25).permutation(idx)
    return sum(play_rows(dev, idx[at:at + CHUNK], form) for at in range(0, len(idx), CHUNK))


@pytest.mark.parametrize("form", FORMS)
def test_every_g25_ply_on_device_envs(dev, form):
    """2 520 completing plies, 2 520 blocked and 2 520 open fours, the 232 walks that leave the board, the 644 overlines
    and the 134 ballot-edge plies: reward, done and legal list are the reference's, the planes the model's."""
    assert every_ply(dev, form) == 8570


# ---- neighbours -------------------------------------------------------------------------------------------------------
def neighbour_layout():
    """(row numbers, sel): the 132 pairs (a walk through the bottom edge, the cells it would read from the next board)
    in envs e and e + 1 followed by an env left alone, then the same pairs in swapped order; four such sections, each
    one env longer than a multiple of four, so that every pair stands at e mod 4 = 0, 1, 2 and 3 -- both envs in one
    workgroup (adjacent LDS slices) and in two."""
    ply = plies()
    second = rows_of("neighbour")
    first = ply["pair"][second]
    spacer = int(rows_of("open")[0])
    section, sel = [], []
    for a, b in list(zip(first, second)) + list(zip(second, first)):
        section += [int(a), int(b), spacer]
        sel += [True, True, False]
    section.append(spacer)
    sel.append(False)
    assert len(section) % 4 == 1
    assert {(s * len(section)) % 4 for s in range(4)} == {0, 1, 2, 3}      # where a given pair starts, section by section
    return np.array(section * 4), np.array(sel * 4)


def neighbours(dev, form):
    idx, sel = neighbour_layout()
    assert not plies()["done"][idx].any()                     # neither board is finished on its own
    return play_rows(dev, idx, form, sel)


@pytest.mark.parametrize("form", FORMS)
def test_neighbouring_boards_do_not_lend_stones(dev, form):
    """A run that stops at the bottom edge next to the board that holds its continuation in cell numbers, in both
    orders and at every place in a workgroup: neither env finishes, neither board changes beyond its own ply."""
    assert neighbours(dev, form) == 4 * (132 * 2 * 3 + 1)


# ---- ragged grids -----------------------------------------------------------------------------------------------------
def ragged_rows(E):
    """E rows of different kinds, the last one a ply that completes a five of a line starting in the second half."""
    ply = plies()
    complete = rows_of("complete")
    last = complete[(ply["variant"][complete] == 1) & (ply["start"][complete] >= 64)][E]
    others = [rows_of(k)[3 * E + j] for j, k in enumerate(("blocked", "overline", "leaving", "ballot", "open", "complete"))]
    return np.array(others[:E - 1] + [last])


def ragged(dev, form):
    total = 0
    for E in (1, 3, 5, 7):
        idx = ragged_rows(E)
        assert len(idx) == E and plies()["done"][idx[-1]]
        total += play_rows(dev, idx, form)
    return total


@pytest.mark.parametrize("form", FORMS)
def test_ragged_grids_touch_nothing_past_the_last_env(dev, form):
    """E = 1, 3, 5, 7: the last workgroup has wavefronts without an env.  The last env completes a five, the verdicts
    are right and the guard row of every output keeps its sentinel (play_rows checks it on every call)."""
    assert ragged(dev, form) == 16


# ---- envs left alone --------------------------------------------------------------------------------------------------
def left_alone(dev, form):
    ply = plies()
    complete = rows_of("complete")
    idx = complete[ply["variant"][complete] == 1]             # four stones on the board, the ply is the fifth
    assert len(idx) == 1260
    total = 0
    for half in (0, 1):
        total += play_rows(dev, idx, form, np.arange(len(idx)) % 2 == half)
    return total


@pytest.mark.parametrize("form", FORMS)
def test_envs_handed_no_action_stay_as_they_were(dev, form):
    """Every other env gets action -1 while its neighbours complete fives (and, in `advance`, are reset): board, ply
    counter, legal list and side to move of the envs left alone read as before, their reward and done are 0."""
    assert left_alone(dev, form) == 2520


# ---- the random opponent at the ballot hand-over ----------------------------------------------------------------------
def stream_config():
    """Gomoku's config with a small network and a short search: the engine is here for its per-env streams only."""
    config = importlib.import_module("muzero-hypermodel_amd.games.gomoku").MuZeroConfig()
    config.blocks, config.channels, config.num_simulations = 1, 8, 12
    return config


def random_opponent(dev, eng):
    """The recorded draws in opponent mode, each env's stream seeded as the fixture's numpy was; the envs whose side to
    move is the second player's go through `step`, the others through `advance`.  Returns the (board, slot) pairs drawn."""
    pick = picks()
    boards, legal, n_legal = ballot_boards()
    which = pick["board"].astype(np.int64)
    E = len(which)
    seeds = pick["seed"].tolist()
    position, players = boards[which], pick["player"]
    tp = (players == -1).astype(np.int64)
    engine = eng.BatchedMCTS(stream_config(), E, device="cuda", seeds=seeds)
    envs = dev.DeviceEnvs("gomoku", E, seeds=seeds)
    played, words = np.full(E, -1), np.zeros(E, np.uint32)
    reward, done = torch.zeros(E, device="cuda"), torch.zeros(E, dtype=torch.uint8, device="cuda")
    obs_after, obs_next = torch.zeros((E, 3, 11, 11), device="cuda"), torch.zeros((E, 3, 11, 11), device="cuda")
    expect = position.copy()
    expect[np.arange(E), pick["pick"]] = players
    for mzp in (0, 1):
        sel = tp != mzp                                       # the opponent moves here
        envs.set_boards(position, players)
        envs.set_opponent("random", mzp, engine)
        _, got_legal, num_legal, to_play = envs.observe()
        num_legal = num_legal.cpu().numpy()
        assert ((num_legal == 0) == sel).all() and np.array_equal(num_legal[~sel], n_legal[which][~sel])
        assert np.array_equal(to_play.cpu().numpy(), tp)
        assert np.array_equal(masked(got_legal.cpu().numpy(), n_legal[which].astype(np.int32)), legal[which])   # the row stays filled
        handed = torch.full((E,), -1, dtype=torch.int32, device="cuda")
        if mzp == 0:
            envs.step(handed, reward=reward, done=done)
            after = envs.observe()[0].cpu().numpy()
        else:
            envs.advance(handed, reward, done, obs_after, obs_next)
            after = obs_after.cpu().numpy()
            fresh = obs_next.cpu().numpy()[sel & pick["done"]]
            assert not fresh[:, :2].any() and (fresh[:, 2] == 1).all()
        torch.cuda.synchronize()
        got, got_words = envs.played.cpu().numpy(), envs.words.cpu().numpy().view(np.uint32)
        assert (got[~sel] == -1).all() and (got_words[~sel] == 0).all()          # MuZero's turn with action -1: untouched
        played[sel], words[sel] = got[sel], got_words[sel]
        now = (after[:, 0] - after[:, 1]).reshape(E, CELLS).astype(np.int8)
        assert np.array_equal(now[~sel], position[~sel]) and np.array_equal(now[sel], expect[sel])
        assert np.array_equal(reward.cpu().numpy()[sel], pick["reward"][sel].astype(np.float32))
        assert np.array_equal(done.cpu().numpy()[sel].astype(bool), pick["done"][sel])
        assert not reward.cpu().numpy()[~sel].any() and not done.cpu().numpy()[~sel].any()
    assert set(tp.tolist()) == {0, 1}
    assert played.tolist() == pick["pick"].tolist()
    assert words.tolist() == pick["words"].tolist()
    engine.rng_consumed(words)
    for e in range(E):
        state = engine.get_rng_state(e)
        ref = model.numpy_pick(seeds[e], EMPTY_SETS[which[e]])[1]
        assert state[2] == pick["pos"][e] == ref[2] and np.array_equal(state[1], ref[1]), e
    envs.close()
    engine.close()
    return {(int(f), EMPTY_SETS[f].index(int(a))) for f, a in zip(which, played)}


def test_random_opponent_at_the_ballot_hand_over(dev, eng):
    """Boards whose empty cells are {63}, {64}, {63, 64}, {0, 120}, {62..65} and {56, 57, 120}: the opponent's move is
    numpy.random.choice(legal)'s for every recorded seed, `words` and the stream position are the fixture's, and every
    slot of every board was drawn -- the slot that crosses from the first ballot into the second included."""
    drawn = random_opponent(dev, eng)
    want = {(f, k) for f, empty in enumerate(EMPTY_SETS) if len(empty) <= 4 for k in range(len(empty))}
    assert drawn == want and len(want) == 13
    assert {(f, EMPTY_SETS[f][k]) for f, k in drawn} >= {(2, 63), (2, 64), (4, 63), (4, 64), (7, 120), (3, 0), (3, 120)}


# ---- the one-thread-per-env form --------------------------------------------------------------------------------------
def compare_all(dev, eng):
    """Everything above in one go; returns the number of envs compared."""
    total = 0
    for form in FORMS:
        total += every_ply(dev, form) + neighbours(dev, form) + ragged(dev, form) + left_alone(dev, form)
    return total + len(random_opponent(dev, eng))


def test_one_thread_per_env_form_agrees_on_every_row(dev, eng):
    """MZENV_GOMOKU_SERIAL=1 (read at mzenv_create) runs the same rules text one thread per env: a fresh process puts
    every row of this file through it and prints how many envs it compared -- as many as the wavefront form here."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import importlib, test_gpu_gomoku_rules as t\n"
            "dev = importlib.import_module('muzero-hypermodel_amd.games.device')\n"
            "eng = importlib.import_module('muzero-hypermodel_amd.engine')\n"
            "print('compared', t.compare_all(dev, eng))\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, MZENV_GOMOKU_SERIAL="1")
    proc = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "compared" in proc.stdout, proc.stdout + proc.stderr
    compared = int(proc.stdout.split("compared")[-1].split()[0])
    here = compare_all(dev, eng)
    assert compared == here == 2 * (8570 + 4 * 793 + 16 + 2520) + 13
