"""The numpy yardstick of the replay sampler (tests/replay_sampler_reference.py) and the case set of
tests/test_gpu_replay_sampler_forms.py, without a GPU:

* the yardstick gives index_batch / weight_batch of the four G12 fixtures, the fixtures' absorbing actions, and leaves
  numpy's stream where oracle/replay_oracle.get_batch leaves it;
* the restated switches of mzreplay_sample_batch flip where the case names say, and every batch of every case is on
  the side it is named for;
* every case runs under numpy.random.RandomState.choice without an exception (probabilities sum to 1, no sampled game
  without a positive priority) -- so a failure on the device is the device's;
* a copy of the yardstick with the draws spelled out word by word equals it on the named cases, and each way of
  getting the sampler wrong that the cases are there for -- one switch of that copy each -- is rejected by a named
  case: the case set means something."""
import importlib
import os
import sys

import numpy as np
import pytest

import replay_sampler_cases as rc
from parity_helpers import load_golden
from replay_sampler_reference import sample_batch
from test_oracle_replay import NAMES, cfg_of, games_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


# ---- the yardstick against the reference's recorded batches -----------------------------------------------------------
class NumpyRng:
    """oracle.replay_oracle.get_batch's generator interface over numpy's own legacy RandomState."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def choice_p(self, p):
        return int(self.rs.choice(len(p), p=p))

    def below(self, n):
        return int(self.rs.choice(n))


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_reproduces_g12(name):
    ro = importlib.import_module("replay_oracle")
    fx = load_golden(f"g12_replay_{name}")
    cfg = cfg_of(fx)
    lengths = fx["lengths"]
    U, A, per = cfg["num_unroll_steps"], len(cfg["action_space"]), cfg["PER"]
    if per:
        priorities = [fx["priorities"][g, :n] for g, n in enumerate(lengths)]
        game_priority = fx["game_priority"]
    else:
        priorities, game_priority = [np.ones(n, dtype=np.float32) for n in lengths], np.ones(len(lengths), dtype=np.float32)
    got = sample_batch(np.random.RandomState(int(fx["seed"])), game_priority, lengths, priorities, cfg["batch_size"], U, A,
                       per, int(lengths.sum()))
    assert np.array_equal(np.stack([got["game_index"], got["position"]], axis=1), fx["index_batch"])
    if per:
        assert got["weight"].dtype == np.float32
        assert np.array_equal(got["weight"].view(np.uint32), fx["weight_batch"].view(np.uint32))
    else:
        assert got["weight"] is None
    past = got["position"][:, None] + np.arange(U + 1)[None, :] > lengths[got["game_index"]][:, None]
    assert past.any() and np.array_equal(got["absorbing"][past], fx["action_batch"][past]) and not got["absorbing"][~past].any()
    # the stream: where the oracle's get_batch, over numpy's generator, stands after the same batch
    games = games_of(fx, ro)
    for g, game in enumerate(games):
        game.priorities, game.game_priority = priorities[g], game_priority[g]
    rng = NumpyRng(int(fx["seed"]))
    out = ro.get_batch(games, cfg, rng)
    assert np.array_equal(np.array(out["index"]), fx["index_batch"])
    state = rng.rs.get_state()
    assert got["state"][2] == state[2] and np.array_equal(got["state"][1], state[1])


# ---- the switches ------------------------------------------------------------------------------------------------------
def test_switch_edges():
    assert rc.lds_games(12288) and not rc.lds_games(12289)
    assert rc.lds_rows(18432) and not rc.lds_rows(18433) and not rc.lds_rows(27000)
    assert rc.lds_tails(3351, 5, 9) and not rc.lds_tails(3352, 5, 9)
    assert rc.lds_tails(4096, 4, 9) and 4096 * (8 * 4 + 4) == rc.LDS_BUDGET and not rc.lds_tails(4096, 5, 9)
    assert rc.lds_tails(4096, 121, 1)                                   # the tail is never longer than a game
    assert rc.batch_admitted(1) and rc.batch_admitted(4096) and not rc.batch_admitted(4097) and not rc.batch_admitted(0)
    # the leaf count: 64 per full piece of 8192, first past 512 at 65 033 stored games, and not monotone after that
    assert rc.leaf_count(128) == 1 and rc.leaf_count(129) == 2 and rc.leaf_count(8192) == 64 and rc.leaf_count(32768) == 256
    want = {65032: 512, 65033: 513, 65040: 512, 65536: 512, 65537: 513}
    assert {n: rc.leaf_count(n) for n in want} == want
    assert all(rc.leaf_count(n) <= 512 for n in range(1, 65033))
    assert rc.leaf_count(70001) > 512 and rc.leaf_count(140001) > 512
    assert [rc.parallel_leaves(n) for n in rc.LEAF_EDGES] == [True, False, True, True, False, False]


def test_untemper_inverts_numpys_tempering():
    rs = np.random.RandomState(1)
    words = [int(w) for w in rs.randint(0, 1 << 32, size=50, dtype=np.uint32)] + [0, 0xFFFFFFFF, 1 << 31, 1]
    key = rs.get_state()[1].copy()
    key[: len(words)] = [rc.untemper(w) for w in words]
    rs.set_state(("MT19937", key, 0, 0, 0.0))
    assert [int(rs.randint(0, 1 << 32, dtype=np.uint32)) for _ in words] == words
    doubles = [0.0, 0.25, 1 - rc.EPS, 0.5 - rc.EPS, 12345 / 2 ** 53]
    rs.set_state(("MT19937", rc.key_for_doubles(doubles), 0, 0, 0.0))
    assert [rs.random_sample() for _ in doubles] == doubles


# ---- every case under numpy ----------------------------------------------------------------------------------------------
_RUNS = {}


def run_of(name):
    if name not in _RUNS:
        run = rc.Run(rc.case_named(name))
        run.case.script(run)
        _RUNS[name] = run
    return _RUNS[name]


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_runs_under_numpy(name):
    run = run_of(name)                       # numpy raises where probabilities are NaN or do not sum to 1
    assert run.records
    for r in run.records:
        want = r["want"]
        n = len(r["inputs"][1])
        assert want["game_index"].min() >= 0 and want["game_index"].max() < n
        assert (want["position"] < r["inputs"][1][want["game_index"]]).all() and want["position"].min() >= 0
        assert want["absorbing"].max() < run.case.actions
        if r["per"]:
            assert np.isfinite(want["weight"]).all() and want["weight"].max() == 1 and want["weight"].min() > 0


def test_cases_cover_both_sides_of_every_switch():
    seen = {}
    for name in rc.CASE_NAMES:
        if name.startswith("stream"):
            continue
        for r in run_of(name).records:
            for key, side in r["forms"].items():
                if key == "lds_tails" and not r["per"]:
                    continue
                seen.setdefault(key, set()).add(side)
    assert all(seen[key] == {True, False} for key in ("lds_games", "parallel_leaves", "lds_rows", "lds_tails", "wrapped")), seen
    sizes = {r["batch"] for name in rc.CASE_NAMES for r in run_of(name).records}
    assert {1, 5, 61, 129, 3351, 3352, 4096} <= sizes
    counts = {len(r["inputs"][1]) for name in ("games G=12288", "games G=12289", "leaves n=65032..70001")
              for r in run_of(name).records}
    assert {1, 2, 12287, 12288, 12289} | set(rc.LEAF_EDGES) <= counts


def test_stream_cases_meet_the_twist_in_every_loop():
    """a start position for each way a draw can straddle the 624-word block"""
    run = run_of("stream A=3 per")
    ends = [r["want"]["state"][2] for r in run.records]
    starts = [r["before"][2] for r in run.records]
    assert starts == list(range(625))
    assert any(e < s for s, e in zip(starts, ends))                      # the block turned over inside a batch
    assert 623 in starts                                                  # between the two words of the first game double
    run = run_of("stream U=121 per")                                      # 1-ply games: 121 actions drawn per sample,
    assert all(r["want"]["absorbing"][:, 1:].size == 5 * 121 for r in run.records)   # more than one round of 64 words
    assert (run.records[0]["want"]["position"] == 0).all()


# ---- the spelled-out copy and its defects ----------------------------------------------------------------------------------
def spelled_out(rs, game_priority, lengths, priorities, batch, unroll, num_actions, per, total_samples, defect=None):
    """sample_batch with choice() taken apart: words, doubles, running sums and bisection written out."""
    def word():
        return int(rs.randint(0, 1 << 32, dtype=np.uint32))

    def double():
        first, second = word(), word()
        if defect == "words swapped":
            first, second = second, first
        return ((first >> 5) * 67108864.0 + (second >> 6)) / 9007199254740992.0

    def below(n, action=False):
        if n == 1:
            return 0
        if action and defect == "modulo":
            return word() % n
        mask = (1 << (n - 1).bit_length()) - 1
        while True:
            v = word() & mask
            if v < n:
                return v

    def quotients(p, total):
        return p.astype(np.float64) / np.float64(total) if defect == "float64 quotients" else p / total

    def table_of(p):
        cdf = np.cumsum(p.astype(np.float64))
        return cdf if defect == "no renormalisation" else cdf / cdf[-1]

    def draw(table):
        return int(np.searchsorted(table, double(), side="left" if defect == "left bisection" else "right"))

    n = len(lengths)
    U1 = unroll + 1
    if per:
        p = np.array(game_priority, dtype=np.float32)
        total = np.sum(p)
        if defect == "sequential sum" and n > 8192:
            total = np.add.accumulate(p)[-1]
        if defect == "one tree":
            total = rc.pairwise_tree(p)
        game_probs = quotients(p, total)
        table = table_of(game_probs)
        game_index = [min(draw(table), n - 1) for _ in range(batch)]
    else:
        game_index = [below(n) for _ in range(batch)]
    position = np.zeros(batch, dtype=np.int64)
    absorbing = np.zeros((batch, U1), dtype=np.int64)
    weights = []

    def draw_position(b):
        g = game_index[b]
        if not per:
            return below(int(lengths[g])), None
        row = priorities[g]
        total = np.float32(0)
        for x in row:
            total = total + x
        probs = quotients(row, total)
        pos = min(draw(table_of(probs)), len(row) - 1)
        return pos, probs[pos]

    early = None
    for b in range(batch):
        pos, prob = early if early is not None else draw_position(b)
        early = draw_position(b + 1) if defect == "early position" and b + 1 < batch else None
        position[b] = pos
        if per:
            weights.append(1 / (total_samples * game_probs[game_index[b]] * prob))
        for u in range(U1):
            if pos + u > lengths[game_index[b]]:
                absorbing[b, u] = below(num_actions, action=True)
    weight = np.array(weights, dtype="float32") / max(weights) if per else None
    return dict(game_index=np.array(game_index, dtype=np.int64), position=position, absorbing=absorbing, weight=weight,
                state=rs.get_state())


def same(a, b):
    return (np.array_equal(a["game_index"], b["game_index"]) and np.array_equal(a["position"], b["position"])
            and np.array_equal(a["absorbing"], b["absorbing"])
            and ((a["weight"] is None and b["weight"] is None)
                 or np.array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32)))
            and a["state"][2] == b["state"][2] and np.array_equal(a["state"][1], b["state"][1]))


def replay(run, record, defect=None):
    rs = np.random.RandomState(0)
    rs.set_state(record["before"])
    return spelled_out(rs, *record["inputs"][:3], record["batch"], run.case.unroll, run.case.actions, record["per"],
                       record["inputs"][3], defect=defect)


def record_of(case, label):
    run = run_of(case)
    return run, next(r for r in run.records if r["label"] == label)


DEFECTS = [  # (defect, case, batch label)
    ("sequential sum", "games G=12288", "n=12288 per"),
    ("sequential sum", "leaves n=65032..70001", "n=65033 per"),
    ("sequential sum", "games G=12289", "n=12289 per"),
    ("one tree", "games G=12288", "n=12288 per"),
    ("one tree", "games G=12289", "n=12289 per"),
    ("one tree", "leaves n=65032..70001", "n=65537 per"),
    ("left bisection", "chosen equal games", "chosen"),
    ("left bisection", "chosen zero games subnormal", "chosen"),
    ("no renormalisation", "chosen last != 1", "chosen"),
    ("float64 quotients", "positions L=27000", "batch 5 #0"),
    ("float64 quotients", "games G=12288", "wrapped per"),
    ("words swapped", "walk U=5", "batch 3352"),
    ("words swapped", "chosen equal games", "chosen"),
    ("modulo", "stream A=3 uniform", "pos 0"),
    ("modulo", "stream U=121 per", "pos 600"),
    ("early position", "stream A=2 per", "pos 17"),
    ("early position", "several batches", "#1 batch 129"),
]


@pytest.mark.parametrize("defect,case,label", DEFECTS)
def test_named_case_rejects_defect(defect, case, label):
    run, record = record_of(case, label)
    assert same(replay(run, record), record["want"]), "the spelled-out copy is not the yardstick"
    with np.errstate(invalid="ignore", divide="ignore"):      # (a zero-priority game, once a defect picks it, has no table)
        assert not same(replay(run, record, defect), record["want"]), f"{case} / {label} does not notice: {defect}"


@pytest.mark.parametrize("case", ["games G=12288", "positions L=18433", "walk U=4", "several batches", "stream A=121 per",
                                  "stream U=121 uniform", "chosen zero games", "chosen last != 1"])
def test_spelled_out_copy_is_the_yardstick(case):
    run = run_of(case)
    for record in run.records[:: max(1, len(run.records) // 25)]:
        assert same(replay(run, record), record["want"]), record["label"]
