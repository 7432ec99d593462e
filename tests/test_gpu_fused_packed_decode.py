"""The packed decode of the flagship form of the narrow whole-move kernel (narrow_device.h narrow_decode_flagship): the
five-lane tails of the value and reward support vectors and the two policy logits go through ONE exp_nonpositive chain
(lanes 0..4, 8..12 and 14..15 of one register), the two expectations through ONE inverse_value_transform_narrow (lanes 0..7
and 8..15).  The generic form of the same build keeps the unpacked functions and is the reference inside the build.

The rows reach the decode exactly, by the crafted-network method of tests/test_gpu_fused_shape_forms.py section 3: the
representation is the identity, the value, reward and policy heads end in zero weights with the row as biases.  The shape
is CartPole's (encoding 8, F = 21, two actions, one player), so the engine takes the flagship form unless told otherwise.
E = 8; one simulation (its decode is the only one whose inputs and outputs all show: the new node's priors, the reward on
the root's child, the value in the root's sum) and six (the decode's results feed further descents and backups).

Rows that tell a wrong packing from a right one: the maximum of one vector in the tail (elements 16..20) while the
other's is in the head, and the reverse; the maximum at element 15, 16 and 20; a tail more than 104 below the maximum (the
exponential's cut to 0) next to a live head, and the reverse; all 21 equal; an expectation of exactly 0 next to a non-zero
one (a swap of the transform's halves shows), and the reverse; expectations at the two ends of the support with opposite
signs; policy logits equal, more than 104 apart, the larger in either lane.

Compared three ways: the flagship form against the generic form, everything a move hands back, as integer words; against
the float64 model within categorical_mean_bound / value_transform_bound (one simulation); against the bits of the commit
before the packing, recorded with `parent_record` below on that commit's build into
tests/golden/fused_packed_decode_parent.npz.

One S = 50 search of CartPole's checkpoint rides along: real logits, and trees deeper than four levels, so that descents
take a second window and backups of several levels carry the decoded values and rewards.
"""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import (cartpole_model_and_weights, categorical_mean, categorical_mean_bound, fc_reference_inference,
                            fc_reference_model, fc_rounding_bounds, load_golden, synthetic_model, value_transform_bound)

pytestmark = pytest.mark.gpu

SWITCH = "MZMCTS_NARROW_GENERIC_SHAPE"
E, WIDTH, SUPPORT, F = 8, 8, 10, 21
SIMULATIONS = (1, 6)
DEEP_SIMULATIONS = 50


@pytest.fixture(scope="module")
def eng(pkg):
    assert torch.cuda.is_available()
    return importlib.import_module("muzero-hypermodel_amd.engine")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def words(a):
    """an array as integers: float arrays by their bit patterns"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


def cartpole_config(simulations):
    cfg = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    cfg.num_simulations = simulations
    return cfg


def crafted_config(simulations):
    cfg = cartpole_config(simulations)
    cfg.observation_shape = (1, 1, WIDTH)
    cfg.encoding_size = WIDTH
    cfg.support_size = SUPPORT
    cfg.network = "fullyconnected"
    return cfg


# ---- the rows -----------------------------------------------------------------------------------------------------------
def _f32(values):
    return np.asarray(values, np.float32)


def peak(at, height=4.0):
    """a gentle ramp with one entry raised: the maximum at element `at`"""
    v = np.linspace(-1.0, 1.0, F).astype(np.float32) * np.float32(0.5)
    v[at] = height
    return v


def lone(at):
    """every entry but one cut to 0 by the exponential: the expectation is exactly at - SUPPORT"""
    v = np.full(F, -200.0, np.float32)
    v[at] = 0.5
    return v


def dead_tail():
    v = peak(3)
    v[16:] = v.max() - np.float32(110.0) + np.linspace(0.0, 1.0, F - 16).astype(np.float32)
    return v


def dead_head():
    v = peak(18)
    v[:16] = v.max() - np.float32(110.0) + np.linspace(0.0, 1.0, 16).astype(np.float32)
    return v


def crafted_cases():
    """name -> (value logits [21], reward logits [21], policy logits [2])"""
    return {
        "value_tail+reward_head": (peak(18), peak(3), _f32([0.3, -0.2])),
        "value_head+reward_tail": (peak(3), peak(18), _f32([-0.2, 0.3])),
        "max_15+max_16": (peak(15), peak(16), _f32([0.5, 0.5])),
        "max_16+max_20": (peak(16), peak(20), _f32([1.25, -1.5])),
        "max_20+max_15": (peak(20), peak(15), _f32([-1.5, 1.25])),
        "dead_tail+dead_head": (dead_tail(), dead_head(), _f32([60.0, -60.0])),
        "dead_head+dead_tail": (dead_head(), dead_tail(), _f32([-60.0, 60.0])),
        "all_equal": (np.full(F, 0.25, np.float32), np.full(F, 0.25, np.float32), _f32([-0.75, -0.75])),
        "value_zero+reward_tail": (lone(SUPPORT), peak(17), _f32([0.0, -104.5])),
        "value_tail+reward_zero": (peak(17), lone(SUPPORT), _f32([-104.5, 0.0])),
        "value_low_end+reward_high_end": (lone(0), lone(F - 1), _f32([2.0, 1.0])),
        "value_high_end+reward_low_end": (lone(F - 1), lone(0), _f32([1.0, 2.0])),
    }


def last_linear(sd, net):
    index = max(int(k.split(".")[2]) for k in sd if k.startswith(net + ".module."))
    return f"{net}.module.{index}.weight", f"{net}.module.{index}.bias"


def crafted_model(models_mod, cfg, value, reward, policy):
    model, _ = synthetic_model(models_mod, cfg, "cpu", seed=3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    w, b = last_linear(sd, "representation_network")
    sd[w], sd[b] = torch.eye(sd[w].shape[0]), torch.zeros_like(sd[b])
    for net, row in (("prediction_value_network", value), ("dynamics_reward_network", reward),
                     ("prediction_policy_network", policy)):
        w, b = last_linear(sd, net)
        sd[w], sd[b] = torch.zeros_like(sd[w]), torch.from_numpy(row.copy())
    model.load_state_dict(sd)
    return model.to("cuda").eval()


def observations():
    obs = np.random.RandomState(41).uniform(-1.0, 1.0, (E, 1, 1, WIDTH)).astype(np.float32)
    obs[:, 0, 0, 0], obs[:, 0, 0, -1] = -1.0, 1.0
    return obs


def search_outputs(eng, monkeypatch, cfg, model, obs, add_noise, generic):
    """one whole-move search: everything it hands back, two exported trees and the hidden-state pool"""
    if generic:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    engine = eng.BatchedMCTS(cfg, E, group_width=16, seeds=[70 + 3 * e for e in range(E)])
    engine.configure_fused_fc(model)
    engine.set_fused_options("narrow", publish_tree=True)
    assert engine.fused_variant() == "narrow"
    out = {}
    st = engine.search_fused(torch.from_numpy(obs), [[0, 1]] * E, [0] * E, add_noise)
    for key, value in st.items():
        out["search " + key] = np.array(value)
    for e in (0, E - 1):
        for key, value in engine.export_tree(e).items():
            out[f"tree{e} " + key] = value
    out["hidden pool"] = engine.pool.clone().cpu().numpy()
    engine.close()
    return out


def crafted_run(eng, models_mod, monkeypatch, case, simulations, generic=False):
    value, reward, policy = crafted_cases()[case]
    cfg = crafted_config(simulations)
    model = crafted_model(models_mod, cfg, value, reward, policy)
    return search_outputs(eng, monkeypatch, cfg, model, observations(), False, generic), model, cfg


def deep_run(eng, models_mod, monkeypatch, generic=False):
    cfg = cartpole_config(DEEP_SIMULATIONS)
    model, _ = cartpole_model_and_weights(models_mod, cfg, "cuda")
    obs = np.random.RandomState(5).uniform(-0.05, 0.05, (E, 1, 1, 4)).astype(np.float32)
    return search_outputs(eng, monkeypatch, cfg, model, obs, True, generic)


def parent_record(eng, models_mod, monkeypatch):
    """what tests/golden/fused_packed_decode_parent.npz holds: "<case>/S<simulations>/<output>" of the flagship form"""
    record = {}
    for case in crafted_cases():
        for simulations in SIMULATIONS:
            out, _, _ = crafted_run(eng, models_mod, monkeypatch, case, simulations)
            for key, value in out.items():
                record[f"{case}/S{simulations}/{key}"] = value
    for key, value in deep_run(eng, models_mod, monkeypatch).items():
        record[f"cartpole/S{DEEP_SIMULATIONS}/{key}"] = value
    return record


@pytest.fixture(scope="module")
def parent_outputs():
    return load_golden("fused_packed_decode_parent")


def assert_same_words(got, want, what):
    assert got.keys() == want.keys()
    for key in got:
        assert np.array_equal(words(got[key]), words(want[key])), f"{what}: {key}"


def assert_parent_bits(out, parent_outputs, prefix):
    recorded = [k for k in parent_outputs.files if k.startswith(prefix + "/")]
    assert sorted(recorded) == sorted(f"{prefix}/{key}" for key in out)
    for key, value in out.items():
        assert np.array_equal(words(value), words(parent_outputs[f"{prefix}/{key}"])), f"parent's bits: {key}"


def assert_within(name, got, want, bound):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        excess = np.abs(got - want) - bound
    assert np.isfinite(got).all() and (excess <= 0).all(), \
        f"{name}: off by {np.abs(got - want).max():.3g} where {np.asarray(bound).flat[np.argmax(excess)]:.3g} is allowed"


def scalar_of(logits):
    x = categorical_mean(logits, SUPPORT)
    z = (np.sqrt(1.0 + 4.0 * 0.001 * (np.abs(x) + 1.0 + 0.001)) - 1.0) / (2.0 * 0.001)
    return np.sign(x) * (z * z - 1.0)


def decode_bound(logits, logit_bound):
    value = scalar_of(logits)
    return value, value_transform_bound(value, categorical_mean_bound(logit_bound.max(axis=-1), SUPPORT))


@pytest.mark.parametrize("simulations", SIMULATIONS)
@pytest.mark.parametrize("case", list(crafted_cases()))
def test_packed_decode_on_crafted_rows(eng, models_mod, monkeypatch, parent_outputs, case, simulations):
    out, model, cfg = crafted_run(eng, models_mod, monkeypatch, case, simulations)
    generic, _, _ = crafted_run(eng, models_mod, monkeypatch, case, simulations, generic=True)
    assert (out["search visits"].sum(axis=1) == simulations).all()
    assert_same_words(out, generic, "flagship form against generic form")
    if simulations == 1:
        # float64: the rows arrive, and the one decode of the simulation shows whole
        value_row, reward_row, policy_row = crafted_cases()[case]
        ref = fc_reference_model(model)
        obs = observations()
        _, _, _, state64 = fc_reference_inference(ref, observations=obs)
        _, _, _, e_state = fc_rounding_bounds(ref, observations=obs)
        action = out["search visits"].argmax(axis=1).astype(np.int64)
        v, r, p, _ = fc_reference_inference(ref, hidden=state64, action=action)
        e_v, e_r, _, _ = fc_rounding_bounds(ref, hidden=state64, action=action, hidden_error=e_state)
        assert np.array_equal(v, np.tile(value_row, (E, 1))) and np.array_equal(r, np.tile(reward_row, (E, 1)))
        assert np.array_equal(p, np.tile(policy_row, (E, 1)))
        child_value, child_bound = decode_bound(v, e_v)
        reward, reward_bound = decode_bound(r, e_r)
        assert_within("root value sum", out["search root_value_sum"], reward + cfg.discount * child_value,
                      reward_bound + cfg.discount * child_bound + 1e-12)
        prior = np.exp(p - p.max(axis=1, keepdims=True))
        prior /= prior.sum(axis=1, keepdims=True)
        for e in (0, E - 1):
            # the node the simulation expanded, and the reward on the root's child it hangs under
            np.testing.assert_allclose(out[f"tree{e} prior"][1], prior[e], rtol=0, atol=1e-6)
            assert_within(f"reward of tree {e}", out[f"tree{e} reward"][0, action[e]], reward[e], reward_bound[e])
    assert_parent_bits(out, parent_outputs, f"{case}/S{simulations}")


def test_deep_trees_take_a_second_window(eng, models_mod, monkeypatch, parent_outputs):
    out = deep_run(eng, models_mod, monkeypatch)
    generic = deep_run(eng, models_mod, monkeypatch, generic=True)
    recorded_depth = parent_outputs[f"cartpole/S{DEEP_SIMULATIONS}/search max_tree_depth"]
    assert (recorded_depth > 4).any(), recorded_depth       # a descent past four levels loads a second window
    assert (out["search visits"].sum(axis=1) == DEEP_SIMULATIONS).all()
    assert_same_words(out, generic, "flagship form against generic form")
    assert_parent_bits(out, parent_outputs, f"cartpole/S{DEEP_SIMULATIONS}")
