"""Stream states, expected rows and word accounting for the exploration noise the GPU draws (root_noise_kernel and
move_inputs_kernel, csrc/mcts_kernels.hip, through np_legacy_rng.h DeviceStream with a staged window).  numpy only: the
reference is numpy.random.RandomState itself -- set_state, skip the pending words, dirichlet([alpha] * n), get_state.

A draw from position p (after the skip) has a = min(624 - p, 96) words staged and consumes W.  Where it ends relative
to the window and to the 624-word block is its category (first match):
  empty       p = 624: nothing staged, the first word regenerates the block;
  exact_end   p + W = 624: the position stays lazily at 624, the block is not regenerated;
  inside      W <= a;
  window_out  a = 96 < W and p + W < 624: the window runs out inside the block;
  block_end   p < 624 < p + W <= 1248 (sub-cases: p = 623; odd a, where one legacy double takes its first word from the
              window and its second after the regeneration);
  two_regen   p + W > 1248.
W counts whole blocks too (a 256-action draw takes more than 624 words): the number of regenerations between two numpy
states is found by regenerating the earlier key with numpy until it equals the later one."""
import collections
import functools

import numpy as np

BLOCK = 624
WINDOW = 96                       # kNoiseWindow
E = BLOCK + 1                     # one env per start position 0..624
SHAPES = [(0.25, 2), (0.1, 9), (0.3, 7), (0.3, 121), (0.3, 256), (1.0, 3)]     # (alpha, k); the last: exponential branch
CATEGORIES = ("empty", "exact_end", "inside", "window_out", "block_end", "two_regen")

Draw = collections.namedtuple("Draw", "row p a words after regens category skip_regens")


def state_of(key, pos):
    return ("MT19937", np.asarray(key, dtype=np.uint32), int(pos), 0, 0.0)


@functools.lru_cache(maxsize=None)
def _block_key(seed):
    rs = np.random.RandomState(seed)
    rs.bytes(4)                                       # into the stream's second block
    key = rs.get_state()[1].copy()
    key.setflags(write=False)
    return key


def block_key(seed):
    return _block_key(seed)


def sweep_state(e):
    """env e of the sweep: RandomState(1000 + e)'s second block, at position e"""
    return state_of(block_key(1000 + e), e)


def regenerated(key):
    """the block numpy leaves when it draws one word at position 624"""
    rs = np.random.RandomState()
    rs.set_state(state_of(key, BLOCK))
    rs.bytes(4)
    return rs.get_state()[1]


def regenerations(key_before, key_after):
    key, count = np.asarray(key_before), 0
    while not np.array_equal(key, key_after):
        key = regenerated(key)
        count += 1
        assert count <= 4, "the later state is not reachable from the earlier one"
    return count


def words_between(before, after):
    """(words drawn between two numpy states, regenerations among them); positions are lazy (624 = block used up)"""
    regens = regenerations(before[1], after[1])
    return after[2] - before[2] + BLOCK * regens, regens


def skipped(state, words):
    """numpy's state after `words` 32-bit draws nobody looks at"""
    rs = np.random.RandomState()
    rs.set_state(state)
    if words:
        rs.bytes(4 * int(words))
    return rs.get_state()


def categorise(p, words):
    a = min(BLOCK - p, WINDOW)
    if p == BLOCK:
        return "empty"
    if p + words == BLOCK:
        return "exact_end"
    if words <= a:
        return "inside"
    if p + words < BLOCK:
        assert a == WINDOW
        return "window_out"
    return "block_end" if p + words <= 2 * BLOCK else "two_regen"


def draw(state, alpha, n, skip=0):
    """numpy's dirichlet([alpha] * n) from `state` after `skip` pending words"""
    start = skipped(state, skip)
    skip_words, skip_regens = words_between(state, start)
    assert skip_words == skip
    rs = np.random.RandomState()
    rs.set_state(start)
    row = rs.dirichlet([alpha] * n)
    after = rs.get_state()
    words, regens = words_between(start, after)
    p = start[2]
    assert words >= 2 * n and (after[3], after[4]) == (0, 0.0)        # (shape <= 1: no cached gaussian)
    return Draw(row, p, min(BLOCK - p, WINDOW), words, after, regens, categorise(p, words), skip_regens)


@functools.lru_cache(maxsize=None)
def sweep(alpha, k):
    """the 625 draws of dirichlet([alpha] * k), env e from position e"""
    return tuple(draw(sweep_state(e), alpha, k) for e in range(E))


def ragged_n(e, k):
    """legal actions of env e in the ragged launch: 1 + (e mod k), every seventh env inactive"""
    return 0 if e % 7 == 6 else 1 + e % k


@functools.lru_cache(maxsize=None)
def ragged_sweep(alpha, k):
    """the same with ragged roots; None for the inactive envs"""
    return tuple(draw(sweep_state(e), alpha, ragged_n(e, k)) if ragged_n(e, k) else None for e in range(E))


def counts(draws):
    out = collections.Counter(d.category for d in draws if d is not None)
    return {c: out.get(c, 0) for c in CATEGORIES}


def block_end_subcases(draws):
    """(number of block_end draws from p = 623, number with an odd window length)"""
    ends = [d for d in draws if d is not None and d.category == "block_end"]
    return sum(d.p == BLOCK - 1 for d in ends), sum(d.a % 2 == 1 for d in ends)


@functools.lru_cache(maxsize=None)
def exact_end_state(alpha, n, skip=0, first_seed=5000):
    """A state constructed so that skip + draw ends at 624 exactly: for a fixed key, the p = 624 - skip - W at which
    numpy's draw takes W words (the first key of first_seed, first_seed + 1, ... that has one)."""
    for seed in range(first_seed, first_seed + 64):
        key = block_key(seed)
        for words in range(2 * n, BLOCK - skip + 1, 2):
            state = state_of(key, BLOCK - skip - words)
            d = draw(state, alpha, n, skip)
            if d.words == words:
                assert d.category == "exact_end" and d.after[2] == BLOCK and d.regens == 0
                return state
    raise AssertionError("no start position whose draw ends at 624 for %r" % ((alpha, n, skip),))


def assert_coverage(shape_counts, subcases=None):
    """the categories the issue names per shape, from the classification"""
    for (alpha, k), c in shape_counts.items():
        assert c["empty"] >= 1, (alpha, k)
        if k <= 9:
            assert c["inside"] and c["block_end"], (alpha, k, c)
        if k == 121:
            assert c["window_out"] and c["block_end"], c
        if k == 256:
            assert c["two_regen"] and c["block_end"], c
    for (alpha, k), (from_623, odd_a) in (subcases or {}).items():
        if k <= 9:
            assert from_623 >= 1 and odd_a >= 1, (alpha, k, from_623, odd_a)
