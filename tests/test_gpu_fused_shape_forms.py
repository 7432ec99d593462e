"""The two forms of the narrow whole-move kernel (fused_narrow.hip: FlagshipShape, CartPole's network with every shape value a
compile-time constant, and GenericShape, the values read at run time) and the one-instruction min / max lane steps both use.

1. The flagship form against the generic form, bit for bit: CartPole's checkpoint, E = 20 (one full workgroup of 16 trees
   and a partial wavefront), S = 6 and S = 50, with and without exploration noise; a batch of three queued moves, then a
   single search.  One engine is created normally, one under MZMCTS_NARROW_GENERIC_SHAPE=1 (read when the engine is created).
   Everything a move hands back is compared as integers or float words; the word counts of the tie-breaks are the single
   search's `tie_break_words`, and those of the device's action sampling show in the stream positions (host mirror and
   device copy), which are compared as well.
2. Shapes one step away from the flagship's must take the generic form, with the flagship form compiled into the same
   library: F <= 16 (support 5), a 16-lane state (enc 14: enc + A <= 16 is the narrow kernel's admission limit, so enc 16
   itself goes to the generic whole-move kernel of mcts_kernels.hip -- that case runs too), and the two-player masked-root
   two-action shape of tests/test_gpu_fused.py.  E = 8, S = 8, against the lock-step search, bit for bit: a near-miss shape
   sent to the constant-shape form would compute with the wrong widths.
3. The min / max steps (narrow_device.h row_min_max_step and friends) on the operands that tell implementations apart:
   rows of equal values, the extreme in the first and in the last lane, zeros of both signs side by side, denormals next to
   each other and next to zero, support vectors whose maximum is element 0, element 15 or in the upper half (>= 16).  The
   rows reach the kernels exactly: the representation is the identity (raw state = observation row), the last dynamics
   Linear has zero weights and the row as biases, the value and reward heads end in zero weights and the support vector as
   biases.  (A neuron ends in a + b of its two accumulators, and b starts from +0.0, so a -0.0 in a row reaches the
   min / max steps as +0.0: no arithmetic result there is -0.0.  The rows with both zeros stay in as inputs that would show
   a network kernel treating the two differently; the fixture pins what arrives.)
   Through the lock-step narrow inference entries (fc_inference_narrow_kernel) and one simulation of the whole-move kernel
   (narrow_support_pair / narrow_softmax run only there), against the float64 model within the bounds of
   tests/test_gpu_fc_shapes.py, and bit for bit against tests/golden/fused_shape_forms_parent.npz: the outputs of the commit
   before the steps were written by hand (compiler-generated v_mov_dpp + canonicalise + v_min / v_max), recorded with
   `crafted_outputs` below on that commit's build.
"""
import importlib

import numpy as np
import pytest
import torch

from parity_helpers import (cartpole_model_and_weights, categorical_mean, categorical_mean_bound, fc_reference_inference,
                            fc_reference_model, fc_rounding_bounds, load_golden, synthetic_model, value_transform_bound)

pytestmark = pytest.mark.gpu

SWITCH = "MZMCTS_NARROW_GENERIC_SHAPE"


@pytest.fixture(scope="module")
def eng(pkg):
    assert torch.cuda.is_available()
    return importlib.import_module("muzero-hypermodel_amd.engine")


@pytest.fixture(scope="module")
def models_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def cartpole_config(simulations):
    cfg = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    cfg.num_simulations = simulations
    return cfg


def device_streams(engine):
    engine_mod = importlib.import_module("muzero-hypermodel_amd.engine")
    E = engine.E
    key, pos = engine.rng_streams()
    torch.cuda.synchronize()
    keys = engine_mod._device_view(key, E * 624, torch.int32, engine.device).cpu().numpy().view(np.uint32).reshape(E, 624)
    return keys.copy(), engine_mod._device_view(pos, E, torch.int32, engine.device).cpu().numpy().copy()


def words(a):
    """an array as integers: float arrays by their bit patterns"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


# ---- 1. flagship form == generic form -------------------------------------------------------------------------------
FORM_E, FORM_MOVES = 20, 3


def moves_of_form(eng, models_mod, monkeypatch, simulations, add_noise, generic):
    config = cartpole_config(simulations)
    model, _ = cartpole_model_and_weights(models_mod, config, "cuda")
    obs = torch.from_numpy(np.random.RandomState(5).uniform(-0.05, 0.05, (FORM_E, 4)).astype(np.float32)).cuda()
    legal, to_play, T = [[0, 1]] * FORM_E, [0] * FORM_E, np.full(FORM_E, 1.0)
    if generic:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    engine = eng.BatchedMCTS(config, FORM_E, seeds=[900 + 13 * e for e in range(FORM_E)], group_width=16)
    engine.configure_fused_fc(model)
    engine.set_fused_options("narrow", publish_tree=True)
    assert engine.fused_variant() == "narrow"
    got = {}
    out = engine.run_moves([obs] * FORM_MOVES, legal, to_play, T, add_noise)
    assert np.array_equal(out["moves_done"], np.full(FORM_E, FORM_MOVES)), out["moves_done"]
    for key in ("actions", "visits", "root_value_sum", "root_predicted", "max_depth"):
        got["batch " + key] = np.array(out[key])
    got["batch mirror position"] = np.array([engine.get_rng_state(e)[2] for e in range(FORM_E)])
    st = engine.search_fused(obs, legal, to_play, add_noise)
    for key, value in st.items():
        got["search " + key] = np.array(value)
    actions, slots = engine.sample_actions(1.0)
    got["search actions"], got["search slots"] = actions.copy(), slots.copy()
    got["search noise"] = engine.noise.copy()
    for key, value in engine.export_tree(FORM_E - 1).items():
        got["tree " + key] = value
    got["hidden pool"] = engine.pool.clone().cpu().numpy()
    got["mirror position"] = np.array([engine.get_rng_state(e)[2] for e in range(FORM_E)])
    # one further search: the device copies of the streams catch up with the mirrors (sampled words included)
    engine.search_fused(obs, legal, to_play, add_noise)
    got["stream keys"], got["mt_pos"] = device_streams(engine)
    engine.close()
    return got


@pytest.mark.parametrize("add_noise", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("simulations", [6, 50])
def test_flagship_form_equals_generic_form(eng, models_mod, monkeypatch, simulations, add_noise):
    flagship = moves_of_form(eng, models_mod, monkeypatch, simulations, add_noise, generic=False)
    generic = moves_of_form(eng, models_mod, monkeypatch, simulations, add_noise, generic=True)
    assert flagship.keys() == generic.keys()
    assert (flagship["batch visits"].sum(axis=2) == simulations).all()
    assert (flagship["search tie_break_words"] > 0).any() or add_noise      # (without noise every first descent ties)
    for key in flagship:
        assert np.array_equal(words(flagship[key]), words(generic[key])), key


# ---- 2. near-miss shapes take the generic form -----------------------------------------------------------------------
def near_miss_config(name):
    cfg = cartpole_config(8)
    if name == "support_5":          # F = 11 <= 16: one register of support logits
        cfg.support_size = 5
    elif name == "enc_14":           # the 16-lane rescale; enc + A = 16
        cfg.encoding_size = 14
    elif name == "enc_16":           # beyond the narrow kernel: the generic whole-move kernel
        cfg.encoding_size = 16
    elif name == "pair_2p":          # two actions, two players, masked roots (tests/test_gpu_fused.py narrow_pair_2p)
        cfg.players = list(range(2))
    cfg.network = "fullyconnected"
    return cfg


@pytest.mark.parametrize("name", ["support_5", "enc_14", "enc_16", "pair_2p"])
def test_near_miss_shapes_run_the_generic_form(eng, models_mod, name):
    cfg = near_miss_config(name)
    model, _ = synthetic_model(models_mod, cfg, "cuda", seed=3)
    E, A = 8, 2
    rs = np.random.RandomState(17)
    obs = rs.uniform(-0.05, 0.05, (E, 1, 1, 4)).astype(np.float32)
    legal, to_play = [], []
    for e in range(E):
        n = A if len(cfg.players) == 1 else int(rs.randint(1, A + 1))
        legal.append(sorted(rs.choice(A, size=n, replace=False).tolist()))
        to_play.append(int(rs.randint(0, len(cfg.players))))
    if name == "pair_2p":
        assert any(len(row) == 1 for row in legal) and any(len(row) == 2 for row in legal)
    seeds = [int(s) for s in rs.randint(0, 2**31 - 1, E)]
    runs = []
    for fused in (False, True):
        engine = eng.BatchedMCTS(cfg, E, seeds=seeds, group_width=16)
        engine.configure_fused_fc(model)
        assert engine.fused_variant() == ("generic" if name == "enc_16" else "narrow")
        run = engine.search_fused if fused else engine.search_lockstep_fc
        st = {k: np.array(v) for k, v in run(torch.from_numpy(obs), legal, to_play, True).items()}
        actions, _ = engine.sample_actions(1.0)
        runs.append((st, actions.copy(), engine.export_tree(E - 1), engine.noise.copy()))
        engine.close()
    a, b = runs
    assert (b[0]["visits"].sum(axis=1) == 8).all()
    for key in a[0]:
        assert np.array_equal(words(a[0][key]), words(b[0][key])), key
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    for key in a[2]:
        assert np.array_equal(words(a[2][key]), words(b[2][key])), f"tree {key}"


# ---- 3. the min / max steps on crafted rows ---------------------------------------------------------------------------
D1, D2 = np.float32(3e-40), np.float32(7e-41)      # denormals
CRAFTED_SHAPES = {
    "row8": dict(width=8, support=10),      # CartPole's widths: the 8-lane rescale (steps 1, 2, 4), F = 21
    "row14": dict(width=14, support=15),    # the 16-lane rescale (steps 1, 2, 4, 8), F = 31
}


def crafted_rows(width):
    """state rows: name -> float32 [width]"""
    ramp = np.linspace(0.25, 0.75, width).astype(np.float32)
    rows = {"equal": np.full(width, 0.375, np.float32)}
    rows["max_first"] = ramp.copy(); rows["max_first"][0] = 3.0
    rows["min_first"] = ramp.copy(); rows["min_first"][0] = -3.0
    rows["max_last"] = ramp.copy(); rows["max_last"][-1] = 3.0
    rows["min_last"] = ramp.copy(); rows["min_last"][-1] = -3.0
    rows["zeros_both_signs"] = np.array([0.0, -0.0] * (width // 2), np.float32)
    rows["signed_zeros_and_one"] = np.array([-0.0, 0.0] * (width // 2), np.float32); rows["signed_zeros_and_one"][-1] = 1.0
    rows["denormal_next_to_zero"] = np.zeros(width, np.float32); rows["denormal_next_to_zero"][1] = D1
    rows["denormals"] = np.full(width, D1, np.float32); rows["denormals"][width // 2] = D2
    rows["negative_denormal"] = np.zeros(width, np.float32); rows["negative_denormal"][2] = -D1
    return rows


def crafted_supports(F):
    """support logit vectors: name -> float32 [F]"""
    base = np.linspace(-1.0, 1.0, F).astype(np.float32) * np.float32(0.5)
    out = {"equal": np.full(F, 0.25, np.float32)}
    out["max_at_0"] = base.copy(); out["max_at_0"][0] = 4.0
    out["max_at_15"] = base.copy(); out["max_at_15"][15] = 4.0
    out["max_upper_half"] = base.copy(); out["max_upper_half"][F - 2] = 4.0
    out["max_at_16_and_zeros"] = np.array([0.0, -0.0] * F, np.float32)[:F]; out["max_at_16_and_zeros"][16] = D1
    return out


def crafted_config(s):
    cfg = cartpole_config(1)
    cfg.observation_shape = (1, 1, s["width"])
    cfg.encoding_size = s["width"]
    cfg.support_size = s["support"]
    cfg.network = "fullyconnected"
    return cfg


def last_linear(sd, net):
    index = max(int(k.split(".")[2]) for k in sd if k.startswith(net + ".module."))
    return f"{net}.module.{index}.weight", f"{net}.module.{index}.bias"


def crafted_model(models_mod, cfg, state_row, support_vector):
    model, _ = synthetic_model(models_mod, cfg, "cpu", seed=3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    w, b = last_linear(sd, "representation_network")
    sd[w], sd[b] = torch.eye(sd[w].shape[0]), torch.zeros_like(sd[b])
    w, b = last_linear(sd, "dynamics_encoded_state_network")
    sd[w], sd[b] = torch.zeros_like(sd[w]), torch.from_numpy(state_row.copy())
    for net in ("dynamics_reward_network", "prediction_value_network"):
        w, b = last_linear(sd, net)
        vector = support_vector if net.startswith("prediction") else support_vector[::-1]
        sd[w], sd[b] = torch.zeros_like(sd[w]), torch.from_numpy(vector.copy())
    model.load_state_dict(sd)
    return model.to("cuda").eval()


def crafted_cases():
    """(shape name, case name, state row for the dynamics biases, support vector) -- one engine each"""
    cases = []
    for shape_name, s in CRAFTED_SHAPES.items():
        rows, supports = crafted_rows(s["width"]), crafted_supports(2 * s["support"] + 1)
        row_names, support_names = list(rows), list(supports)
        for i in range(max(len(row_names), len(support_names))):
            r, v = row_names[i % len(row_names)], support_names[i % len(support_names)]
            cases.append((shape_name, f"{r}+{v}", rows[r], supports[v]))
    return cases


def crafted_inputs(s):
    rows = crafted_rows(s["width"])
    obs = np.stack(list(rows.values())).reshape(len(rows), 1, 1, s["width"])
    hidden = np.random.RandomState(29).uniform(0.0, 1.0, (len(rows), s["width"])).astype(np.float32)
    hidden[:, 0], hidden[:, -1] = 0.0, 1.0
    return obs, hidden


def crafted_run(eng, models_mod, shape_name, state_row, support_vector):
    """One crafted network through the narrow inference entries and a one-simulation whole-move search; returns the
    outputs (name -> array), the float64 model and the inputs."""
    s = CRAFTED_SHAPES[shape_name]
    cfg = crafted_config(s)
    model = crafted_model(models_mod, cfg, state_row, support_vector)
    ref = fc_reference_model(model)
    obs, hidden = crafted_inputs(s)
    E = len(obs)
    engine = eng.BatchedMCTS(cfg, E, group_width=16, seeds=list(range(E)))
    engine.configure_fused_fc(model)
    engine.set_fused_options("narrow")
    assert engine.fused_variant() == "narrow"
    out = {}
    for name, t in zip(("value", "reward", "policy", "hidden"), engine.fc_initial_inference(torch.from_numpy(obs).cuda())):
        out["initial " + name] = t.detach().cpu().numpy().copy()
    for a in range(2):
        action = np.full(E, a, np.int64)
        got = engine.fc_recurrent_inference(torch.from_numpy(hidden).cuda(), torch.from_numpy(action).cuda())
        for name, t in zip(("value", "reward", "policy", "hidden"), got):
            out[f"recurrent{a} " + name] = t.detach().cpu().numpy().copy()
    st = engine.search_fused(torch.from_numpy(obs), [[0, 1]] * E, [0] * E, False)
    for key in ("visits", "child_prior", "root_predicted_value", "root_value_sum", "min_max"):
        out["search " + key] = np.array(st[key])
    out["search hidden pool"] = engine.pool.clone().cpu().numpy()
    engine.close()
    return out, ref, cfg, obs, hidden


def crafted_outputs(eng, models_mod):
    """every crafted case's outputs under "<shape>/<case>/<output>": what the parent's fixture records"""
    record = {}
    for shape_name, case, state_row, support_vector in crafted_cases():
        out, _, _, _, _ = crafted_run(eng, models_mod, shape_name, state_row, support_vector)
        for key, value in out.items():
            record[f"{shape_name}/{case}/{key}"] = value
    return record


def assert_within(name, got, want, bound):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        excess = np.abs(got - want) - bound
    assert np.isfinite(got).all() and (excess <= 0).all(), \
        f"{name}: off by {np.abs(got - want).max():.3g} where {np.asarray(bound).flat[np.argmax(excess)]:.3g} is allowed"


def scalar_of(logits, support):
    x = categorical_mean(logits, support)
    z = (np.sqrt(1.0 + 4.0 * 0.001 * (np.abs(x) + 1.0 + 0.001)) - 1.0) / (2.0 * 0.001)
    return np.sign(x) * (z * z - 1.0)


def decode_bound(logits, logit_bound, support):
    value = scalar_of(logits, support)
    return value, value_transform_bound(value, categorical_mean_bound(logit_bound.max(axis=-1), support))


@pytest.fixture(scope="module")
def parent_outputs():
    return load_golden("fused_shape_forms_parent")


@pytest.mark.parametrize("shape_name,case,state_row,support_vector", crafted_cases(),
                         ids=[f"{c[0]}-{c[1]}" for c in crafted_cases()])
def test_min_max_steps_on_crafted_rows(eng, models_mod, parent_outputs, shape_name, case, state_row, support_vector):
    out, ref, cfg, obs, hidden = crafted_run(eng, models_mod, shape_name, state_row, support_vector)
    support, E = cfg.support_size, len(obs)
    # the crafted rows arrive: a rescaled row spans [0, 1] exactly where the row has a span of at least 1e-5
    raw = obs.reshape(E, -1)
    spans = raw.max(axis=1) - raw.min(axis=1)
    state = out["initial hidden"]
    assert (state.min(axis=1) == 0.0).all() and (state.max(axis=1)[spans >= 1e-5] == 1.0).all()
    # float64, within the bounds of tests/test_gpu_fc_shapes.py
    want = fc_reference_inference(ref, observations=obs)
    bounds = fc_rounding_bounds(ref, observations=obs)
    for name, i in (("value", 0), ("policy", 2), ("hidden", 3)):
        assert_within(f"initial {name}", out["initial " + name], want[i], bounds[i])
    for a in range(2):
        action = np.full(E, a, np.int64)
        want_r = fc_reference_inference(ref, hidden=hidden, action=action)
        bounds_r = fc_rounding_bounds(ref, hidden=hidden, action=action)
        for name, w, b in zip(("value", "reward", "policy", "hidden"), want_r, bounds_r):
            assert_within(f"recurrent {name} (action {a})", out[f"recurrent{a} " + name], w, b)
    # the whole-move kernel's decode (narrow_support_pair, narrow_softmax) after one simulation, as in
    # test_gpu_fc_shapes.py::test_whole_move_kernel_decodes_like_float64
    value, _, policy, state64 = want
    e_value, _, _, e_state = bounds
    prior = np.exp(policy - policy.max(axis=1, keepdims=True))
    prior /= prior.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(out["search child_prior"], prior, rtol=0, atol=1e-6)
    root_value, root_bound = decode_bound(value, e_value, support)
    assert_within("root value", out["search root_predicted_value"], root_value, root_bound)
    assert (out["search visits"].sum(axis=1) == 1).all()
    action = out["search visits"].argmax(axis=1).astype(np.int64)
    v, r, _, _ = fc_reference_inference(ref, hidden=state64, action=action)
    e_v, e_r, _, _ = fc_rounding_bounds(ref, hidden=state64, action=action, hidden_error=e_state)
    child_value, child_bound = decode_bound(v, e_v, support)
    reward, reward_bound = decode_bound(r, e_r, support)
    assert_within("root value sum", out["search root_value_sum"], reward + cfg.discount * child_value,
                  reward_bound + cfg.discount * child_bound + 1e-12)
    # the parent's bits
    for key, value in out.items():
        recorded = parent_outputs[f"{shape_name}/{case}/{key}"]
        assert np.array_equal(words(value), words(recorded)), key
