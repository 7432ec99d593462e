"""What a finished game reports (csrc/game_outcomes.h), restated with Python's own tools: the built-in sum() over lists for
the rewards -- the reference's expressions of self_play.py:65-90, verbatim -- and numpy.mean / numpy.sum over the list of
non-zero root values.  The cases every outcome test walks (CPU: the library's host entry and the header under the
sanitizers; GPU: mzreplay_game_outcomes on a store that holds them), and five deliberate defects of the restatement, each
of which a named case tells from the rule.

`pairwise` is numpy's summation tree written out (the issue's restatement); the tests first hold it to numpy.sum itself and
only then use its `round8=False` variant as a defect."""
import math
import struct

import numpy as np

LENGTHS = (1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 500)
EDGES = (7, 8, 9, 127, 128, 129)          # counted values on either side of 8 and of 128
PLAYERS = ("one", "alternating", "twice")
REWARDS = ("integer", "fraction")
SPECIALS = ("nan", "negative_zero", "all_zero")
MAX_MOVES = 512                           # the store the GPU test fills with these games


class Case:
    def __init__(self, name, rewards, to_play, root_values):
        self.name = name
        self.rewards = np.ascontiguousarray(rewards, dtype=np.float64)          # [n + 1], rewards[0] == 0.0
        self.to_play = np.ascontiguousarray(to_play, dtype=np.int8)             # [n + 1]
        self.root_values = np.ascontiguousarray(root_values, dtype=np.float64)  # [n]
        self.n = len(self.root_values)
        assert len(self.rewards) == self.n + 1 == len(self.to_play) and self.rewards[0] == 0.0


def _to_play(kind, n):
    i = np.arange(n + 1)
    if kind == "one":
        return np.zeros(n + 1, dtype=np.int8)
    if kind == "alternating":
        return (i % 2).astype(np.int8)
    return (i % 3 == 2).astype(np.int8)   # player 0 moves twice in a row, then player 1 once


def _rewards(kind, n, rng):
    r = np.zeros(n + 1)
    r[1:] = rng.integers(-1, 2, n) if kind == "integer" else rng.integers(-9, 10, n) * 0.1 + rng.random(n) * 1e-3
    return r


def make_cases():
    cases = []
    for n in LENGTHS:
        for counted in (n,) + tuple(c for c in EDGES if c < n):
            for players in PLAYERS:
                for rewards in REWARDS:
                    name = f"n{n}-c{counted}-{players}-{rewards}"
                    rng = np.random.default_rng(abs(hash_name(name)))
                    values = rng.standard_normal(n) * (1.0 if rewards == "integer" else 0.37)
                    values[values == 0.0] = 0.5
                    values[rng.permutation(n)[: n - counted]] = 0.0
                    cases.append(Case(name, _rewards(rewards, n, rng), _to_play(players, n), values))
        for special in SPECIALS:
            name = f"n{n}-{special}"
            rng = np.random.default_rng(abs(hash_name(name)))
            values = rng.standard_normal(n) * 0.37
            if special == "nan":
                values[n // 2] = math.nan
            elif special == "negative_zero":
                values[:: 2] = -0.0           # n = 1: the only value
                values[n // 3] = -0.0
            else:
                values[:] = 0.0
            cases.append(Case(name, _rewards("fraction", n, rng), _to_play("alternating", n), values))
    return cases


def hash_name(name):
    """A seed from a case's name that does not change between interpreter runs (hash() of a str does)."""
    value = 0
    for ch in name.encode():
        value = (value * 131 + ch) % (1 << 31)
    return value


def directed_cases():
    """pairwise_last_bit: the pairwise sum and the left-to-right sum of the values differ in the last bit;
    reverse_order: non-integer rewards whose sum in descending order differs from the ascending one."""
    sixteen = [0.1] * 16                      # eight sums of two, then the tree: 1.6; one by one: 1.5999999999999999
    assert sum(sixteen) != float(np.sum(sixteen))
    assert abs(struct.unpack("<q", struct.pack("<d", sum(sixteen)))[0]
               - struct.unpack("<q", struct.pack("<d", float(np.sum(sixteen))))[0]) == 1
    rewards = [0.0, 0.1, 0.2, 0.3]
    assert sum(rewards) != sum(reversed(rewards))
    return [Case("pairwise_last_bit", np.r_[0.0, np.ones(16)], _to_play("one", 16), sixteen),
            Case("reverse_order", rewards, _to_play("alternating", 3), [0.25, -0.5, 0.125])]


def pairwise(values, round8=True, block=128):
    """numpy's pairwise sum of a list of floats, as the issue restates it."""
    c = len(values)
    if c < 8:
        res = 0.0
        for v in values:
            res = res + v
        return res
    if c <= block:
        r = list(values[:8])
        i = 8
        while i < c - c % 8:
            for j in range(8):
                r[j] = r[j] + values[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in values[i:]:
            res = res + v
        return res
    half = c // 2
    if round8:
        half -= half % 8
    return pairwise(values[:half], round8, block) + pairwise(values[half:], round8, block)


DEFECTS = ("sequential", "zeros_counted", "to_play_i", "float32", "split_unrounded")


def restate(case, defect=None):
    """dict(total_reward, reward_of_player [2], value_sum, value_count, mean_value) as Python floats / ints."""
    reward_history = [float(r) for r in case.rewards]
    to_play_history = [int(p) for p in case.to_play]
    root_values = [float(v) for v in case.root_values]
    total = sum(reward_history)
    shift = 0 if defect == "to_play_i" else 1
    # (rewards[0] is 0.0 and both sums start from 0: the reference's i = 0 term, to_play_history[-1], moves no bit)
    per_player = [float(sum(reward for i, reward in enumerate(reward_history) if to_play_history[i - shift] == player))
                  for player in (0, 1)]
    values = root_values if defect == "zeros_counted" else [value for value in root_values if value]
    count = len(values)
    if defect == "sequential":
        value_sum = float(sum(values))
    elif defect == "float32":
        value_sum = float(np.sum(np.asarray(values, dtype=np.float32), dtype=np.float32)) if count else 0.0
        total = float(np.sum(np.asarray(reward_history, dtype=np.float32), dtype=np.float32))
    elif defect == "split_unrounded":
        value_sum = float(pairwise(values, round8=False))
    else:
        value_sum = float(np.sum(values)) if count else 0.0
    if defect is None:
        mean = float(np.mean(values)) if count else math.nan
    else:
        mean = value_sum / count if count else math.nan
    return dict(total_reward=float(total), reward_of_player=per_player, value_sum=value_sum, value_count=count,
                mean_value=mean)


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def same_bits(a, b):
    """Equal as bit patterns; two NaNs are equal whatever their payloads' history (x86 and the GPU both pass the
    quieted input NaN on, the comparison does not rest on it)."""
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))


def record_matches(record, want):
    """A _native.GAME_OUTCOME_DTYPE record against restate()'s dict: every field and the mean, bit for bit."""
    count = int(record["value_count"])
    got_mean = float(record["value_sum"]) / count if count else math.nan
    return (same_bits(record["total_reward"], want["total_reward"])
            and same_bits(record["reward_of_player"][0], want["reward_of_player"][0])
            and same_bits(record["reward_of_player"][1], want["reward_of_player"][1])
            and count == want["value_count"] and same_bits(record["value_sum"], want["value_sum"])
            and same_bits(got_mean, want["mean_value"]))


def pack_cases(cases):
    """The cases as the stand-alone check program reads them: i32 count, then per case i32 n, f64[n + 1], i8[n + 1], f64[n]."""
    out = [struct.pack("<i", len(cases))]
    for case in cases:
        out += [struct.pack("<i", case.n), case.rewards.tobytes(), case.to_play.tobytes(), case.root_values.tobytes()]
    return b"".join(out)
