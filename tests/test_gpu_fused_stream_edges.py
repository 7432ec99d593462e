"""The narrow whole-move kernel at the edges of its trees' MT19937 streams: the 624-word block of a tree ends inside the
words the kernel steps over for the host (the skip in its prologue), inside a tie-break draw of the descent, or inside
the action sampling of its epilogue, and the tree's row regenerates the block together (narrow_device.h
mt_regenerate_row).  Two batches of 48 moves through run_moves against a second engine that searches LOCK-STEP, one move
at a time, with the same seeds: its RNG code is tree_device.h's serial mt_next and the host mirrors.

E = 21: a full workgroup whose four wavefronts carry four rows each, and a ragged second one.  S = 6.  Once with
exploration noise at T = 1, once without noise at T = 0: there nothing is skipped and nothing sampled, so every row's first
draw is a tie-break at position 624 -- the four rows of a wavefront regenerate inside the descent side by side.

Where each env-move's block ends is known on the CPU: the noise words of a stream state are numpy's own dirichlet draw from
that state, a move's tie-break words are what the lock-step engine reports, sampling at T = 1 takes two.  The first three
envs start from states chosen (with numpy, at collection of the reference) so that the FIRST launch has rows of one
wavefront crossing in all three places: env 0 at position 624 (skip), env 1 where its noise row ends at 624 (tie draw), env 2
where it ends at 623 (one tie word, then sampling crosses).  The test asserts that coverage from the word accounting.

The same runs with MZMCTS_NARROW_SERIAL_TWIST=1 / MZMCTS_NARROW_NO_PREFETCH=1 / MZMCTS_NARROW_TABLE_PER_LAUNCH=1 (the
forms before the row-wide regeneration / the inputs asked for ahead of the staging / the per-engine exploration table):
one build holds both forms of each, and they are the same program."""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import cartpole_model_and_weights

pytestmark = pytest.mark.gpu

E, S, BATCH, BATCHES = 21, 6, 48, 2
MOVES = BATCH * BATCHES
SEEDS = [4100 + 7 * e for e in range(E)]
RUNS = {"noise_T1": (True, 1.0), "plain_T0": (False, 0.0)}


@pytest.fixture(scope="module")
def eng(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd.engine")


@pytest.fixture(scope="module")
def setup(pkg):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    config.num_simulations = S
    model, _ = cartpole_model_and_weights(models, config, "cuda")
    obs = torch.from_numpy(np.random.RandomState(11).uniform(-0.05, 0.05, (E, 4)).astype(np.float32)).cuda()
    return config, model, obs


def noise_words(state, alpha):
    """(words, position afterwards) of numpy's dirichlet([alpha] * 2) drawn from `state`"""
    rs = np.random.RandomState()
    rs.set_state(state)
    rs.dirichlet([alpha] * 2)
    after = rs.get_state()[2]
    before = state[2]
    return (after - before if after > before else after + 624 - before), after


def start_states(alpha):
    """env -> stream state the run starts from (the other envs start freshly seeded, at position 624)"""
    out = {}
    for env, target in ((1, 624), (2, 623)):
        rs = np.random.RandomState(SEEDS[env])
        rs.bytes(4)                                   # into the stream's second block
        key = rs.get_state()[1].copy()
        for words in range(8, 200, 2):
            state = ("MT19937", key, target - words, 0, 0.0)
            if noise_words(state, alpha) == (words, target):
                out[env] = state
                break
        assert env in out
    return out


def advance(pos, words):
    """lazy stream position (624 = block used up) after `words` draws, and whether they regenerated the block"""
    if words == 0:
        return pos, False
    end = pos + words
    return (end, False) if end <= 624 else (end - 624, True)


def make_engine(eng, config, model, states):
    engine = eng.BatchedMCTS(config, E, seeds=SEEDS, group_width=16)
    engine.configure_fused_fc(model)
    engine.set_fused_options("narrow", publish_tree=False)
    for env, state in states.items():
        engine.set_rng_state(env, state)
    return engine


def device_streams(engine):
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    key, pos = engine.rng_streams()
    torch.cuda.synchronize()
    keys = engine_mod._device_view(key, E * 624, torch.int32, engine.device).cpu().numpy().view(np.uint32).reshape(E, 624)
    return keys, engine_mod._device_view(pos, E, torch.int32, engine.device).cpu().numpy()


_reference = {}


def reference(eng, setup, run):
    """The lock-step engine's moves, its device streams after one further search, and where each env-move's block ended."""
    if run in _reference:
        return _reference[run]
    config, model, obs = setup
    add_noise, temperature = RUNS[run]
    alpha = float(config.root_dirichlet_alpha)
    states = start_states(alpha) if add_noise else {}      # (without noise every env starts at position 624)
    legal, to_play, T = [[0, 1]] * E, [0] * E, np.full(E, temperature)
    ref = make_engine(eng, config, model, states)
    moves, crossings = [], []          # crossings[m][e]: "" or the place ("skip" / "tie" / "sample") env e's block ended in move m
    for m in range(MOVES):
        before = [ref.get_rng_state(e) for e in range(E)]
        st = ref.search_lockstep_fc(obs, legal, to_play, add_noise)
        ties = st["tie_break_words"].copy()
        actions, _ = ref.sample_actions(T)
        moves.append((actions.copy(), st["visits"].copy(), st["root_value_sum"].copy(), st["max_tree_depth"].copy()))
        row = []
        for e in range(E):
            pos = before[e][2]
            place = ""
            n = noise_words(before[e], alpha)[0] if add_noise else 0
            for name, words in (("skip", n), ("tie", int(ties[e])), ("sample", 2 if temperature == 1.0 else 0)):
                pos, crossed = advance(pos, words)
                if crossed:
                    assert not place           # (a move draws far fewer than 624 words)
                    place = name
            assert pos == ref.get_rng_state(e)[2], (m, e)      # the accounting is the mirror's
            row.append(place)
        crossings.append(row)
    ref.search_lockstep_fc(obs, legal, to_play, add_noise)
    streams = device_streams(ref)
    ref.close()
    _reference[run] = (states, moves, crossings, streams)
    return _reference[run]


@pytest.mark.parametrize("run", sorted(RUNS))
def test_reference_moves_cross_in_every_place(eng, setup, run):
    """coverage, from the host-side word accounting of the lock-step engine"""
    _, _, crossings, _ = reference(eng, setup, run)
    places = {p for row in crossings for p in row if p}
    if run == "noise_T1":
        assert places == {"skip", "tie", "sample"}, places
        # one launch (no env stalls: moves_done is asserted below), two rows of one wavefront (four consecutive envs),
        # different places
        mixed = [(m, w) for m, row in enumerate(crossings) for w in range(0, E, 4)
                 if len({p for p in row[w:w + 4] if p}) >= 2]
        assert mixed, "no launch in which two rows of one wavefront regenerate in different places"
        assert (0, 0) in mixed and {crossings[0][0], crossings[0][1], crossings[0][2]} == {"skip", "tie", "sample"}
    else:
        # nothing skipped, nothing sampled: every env's first tie-break draw finds its block used up, in move 0
        assert places == {"tie"} and all(p == "tie" for p in crossings[0]), crossings[0]


@pytest.mark.parametrize("switch", [None, "MZMCTS_NARROW_SERIAL_TWIST", "MZMCTS_NARROW_NO_PREFETCH",
                                    "MZMCTS_NARROW_TABLE_PER_LAUNCH"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_fused_move_batches_equal_lockstep_across_block_ends(eng, setup, monkeypatch, run, switch):
    config, model, obs = setup
    add_noise, temperature = RUNS[run]
    states, want, _, want_streams = reference(eng, setup, run)
    legal, to_play, T = [[0, 1]] * E, [0] * E, np.full(E, temperature)
    if switch:
        monkeypatch.setenv(switch, "1")            # read once, when the engine is created
    engine = make_engine(eng, config, model, states)
    assert engine.fused_variant() == "narrow"
    for b in range(BATCHES):
        out = engine.run_moves([obs] * BATCH, legal, to_play, T, add_noise)
        assert np.array_equal(out["moves_done"], np.full(E, BATCH)), out["moves_done"]
        for m in range(BATCH):
            actions, visits, value_sum, depth = want[b * BATCH + m]
            assert np.array_equal(out["actions"][m], actions), (b, m)
            assert np.array_equal(out["visits"][m], visits), (b, m)
            assert np.array_equal(out["root_value_sum"][m].view(np.uint64), value_sum.view(np.uint64)), (b, m)
            assert np.array_equal(out["max_depth"][m], depth), (b, m)
    # one further search on each engine: the device copies of the streams have caught up with the mirrors
    engine.search_fused(obs, legal, to_play, add_noise)
    keys, pos = device_streams(engine)
    engine.close()
    assert np.array_equal(pos, want_streams[1])
    assert np.array_equal(keys, want_streams[0])
