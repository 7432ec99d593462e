"""Shared helpers of the parity tests (and of __graft_entry__.smoke / bench.py's checker legs).

"Injected mode": per-simulation network outputs (value, reward, priors) come from a fixture or a
seeded generator instead of a network, so the tree arithmetic of the HIP engine can be compared
BIT-EXACTLY with the oracle / the reference's recorded traces.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for _p in (ROOT, GOLDEN, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def fixture_config(fx, base_config=None, H=0):
    """A MuZeroConfig-like attribute bag carrying the search constants of a trace fixture."""
    cfg = base_config if base_config is not None else types.SimpleNamespace()
    cfg.action_space = list(range(int(fx["cfg_A"])))
    cfg.players = list(range(int(fx["cfg_players"])))
    cfg.num_simulations = int(fx["cfg_S"])
    d = float(fx["cfg_discount"])
    cfg.discount = int(d) if d == int(d) else d
    cfg.pb_c_base = float(fx["cfg_pb_c_base"])
    cfg.pb_c_init = float(fx["cfg_pb_c_init"])
    cfg.root_dirichlet_alpha = float(fx["cfg_alpha"])
    cfg.root_exploration_fraction = float(fx["cfg_frac"])
    cfg.support_size = int(fx["cfg_support"])
    if base_config is None:
        cfg.seed = 0
        cfg.network = "fullyconnected"
        cfg.encoding_size = max(H, 4)
        cfg.observation_shape = (1, 1, 4)
        cfg.downsample = False
    return cfg


def make_search_config(A, S, players, discount, alpha=0.25, frac=0.25, support=10, pb_c_base=19652,
                       pb_c_init=1.25, H=4):
    return types.SimpleNamespace(
        action_space=list(range(A)), players=list(range(players)), num_simulations=S,
        discount=discount, pb_c_base=pb_c_base, pb_c_init=pb_c_init, root_dirichlet_alpha=alpha,
        root_exploration_fraction=frac, support_size=support, seed=0, network="fullyconnected",
        encoding_size=H, observation_shape=(1, 1, 4), downsample=False)


# ---- injected streams --------------------------------------------------------------------------
def streams_from_fixture(fx, idx):
    """dict of per-tree inputs for `idx` traces of a golden trace file."""
    idx = list(idx)
    return dict(
        seeds=[int(fx["seed"][i]) for i in idx],
        legal=[fx["legal"][i][: int(fx["n_legal"][i])].tolist() for i in idx],
        to_play=[int(fx["to_play"][i]) for i in idx],
        root_reward=np.array([fx["root_reward"][i] for i in idx], dtype=np.float64),
        root_priors=np.stack([fx["root_priors"][i] for i in idx]).astype(np.float64),
        value=np.stack([fx["sim_value"][i] for i in idx]).astype(np.float64),      # [T,S]
        reward=np.stack([fx["sim_reward"][i] for i in idx]).astype(np.float64),    # [T,S]
        priors=np.stack([fx["sim_priors"][i] for i in idx]).astype(np.float64),    # [T,S,A]
    )


def random_streams(T, A, S, seed, n_players=1, ties=False, min_legal=1):
    """Seeded synthetic injected streams for configurations no golden trace covers.  Values and
    rewards are fp32-representable like the reference's `.item()` results."""
    rs = np.random.RandomState(seed)
    legal = []
    for _ in range(T):
        n = int(rs.randint(min_legal, A + 1))
        legal.append(sorted(rs.choice(A, size=n, replace=False).tolist()))

    def f32(x):
        return np.asarray(x, dtype=np.float32).astype(np.float64)

    def priors(shape):
        p = rs.dirichlet([0.6] * A, size=shape).astype(np.float32)
        if ties:
            p = np.round(p * 4) / 4 + np.float32(0.125)      # many exactly-equal priors
            p = (p / p.sum(axis=-1, keepdims=True)).astype(np.float32)
        return p.astype(np.float64)

    root_priors = np.zeros((T, A))
    for t in range(T):
        n = len(legal[t])
        p = rs.dirichlet([0.8] * n).astype(np.float32)
        root_priors[t, :n] = p
    scale = 3.0 if n_players == 2 else 30.0
    return dict(
        seeds=[int(s) for s in rs.randint(0, 2**31 - 1, size=T)],
        legal=legal,
        to_play=[int(p) for p in rs.randint(0, n_players, size=T)],
        root_reward=np.zeros(T),
        root_priors=root_priors,
        value=f32(scale * rs.standard_normal((T, S))),
        reward=f32(rs.standard_normal((T, S)) * (rs.random_sample((T, S)) < 0.5)),
        priors=priors((T, S)),
    )


def run_injected_on_oracle(oracle, cfg_or_fx, streams=None, idx=None, temperature=1.0):
    """Replay injected streams through the C oracle, one tree at a time."""
    if streams is None:
        fx = cfg_or_fx
        streams = streams_from_fixture(fx, idx)
        ocfg = oracle.config_from_fixture(fx)
    else:
        ocfg = oracle.config_from_muzero(cfg_or_fx)
    T, A, S = len(streams["seeds"]), ocfg.A, ocfg.S
    out = _result_arrays(T, A, S)
    temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (T,))
    for t in range(T):
        rng = oracle.Rng(streams["seeds"][t])
        tree = oracle.Tree(ocfg)
        n = len(streams["legal"][t])
        noise = tree.reset(rng, streams["legal"][t], streams["to_play"][t], float(streams["root_reward"][t]),
                           root_priors=streams["root_priors"][t][:n], add_noise=True)
        tree.simulate(rng, value=streams["value"][t], reward=streams["reward"][t], priors=streams["priors"][t])
        st = tree.root_stats()
        out["noise"][t, :n] = noise[:n]
        out["visits"][t, :n] = st["visits"]
        out["child_value_sum"][t, :n] = st["child_value_sum"]
        out["child_prior"][t, :n] = st["child_prior"]
        out["child_reward"][t, :n] = st["child_reward"]
        out["root_value_sum"][t] = st["root_value_sum"]
        out["root_visits"][t] = st["root_visit"]
        out["max_tree_depth"][t] = st["max_tree_depth"]
        out["min_max"][t] = (st["mms_min"], st["mms_max"])
        out["sim_depth"][t] = tree.sim_depth
        out["sim_actions"][t] = tree.sim_actions[:, :S]
        out["sim_ties"][t] = tree.sim_ties[:, :S]
        words_before = rng.words
        cv, rv = tree.search_statistics()
        out["child_visits_target"][t] = cv
        out["root_value_target"][t] = rv
        slot = oracle.select_action(rng, st["visits"], float(temps[t]))
        out["action"][t] = streams["legal"][t][slot]
        out["rng_words_run"][t] = words_before
        out["rng_words_total"][t] = rng.words
    return out


def _result_arrays(T, A, S):
    return dict(
        noise=np.zeros((T, A)), visits=np.zeros((T, A), np.int32), child_value_sum=np.zeros((T, A)),
        child_prior=np.zeros((T, A)), child_reward=np.zeros((T, A)), root_value_sum=np.zeros(T),
        root_visits=np.zeros(T, np.int32), max_tree_depth=np.zeros(T, np.int32), min_max=np.zeros((T, 2)),
        sim_depth=np.zeros((T, S), np.int32), sim_actions=np.full((T, S, S), -1, np.int32),
        sim_ties=np.zeros((T, S, S), np.int32), child_visits_target=np.zeros((T, A)),
        root_value_target=np.zeros(T), action=np.zeros(T, np.int32), rng_words_run=np.zeros(T, np.int64),
        rng_words_total=np.zeros(T, np.int64))


def run_injected_on_engine(engine_mod, config, fx_or_streams, idx=None, device="cuda", temperature=1.0,
                           record_paths=True, repeat=1, engine=None, group_width=0, fused_step=False, select_queue=0,
                           device_noise=False):
    """Drive the HIP engine through the C ABI with injected streams.

    `repeat` tiles the T trees `repeat` times (env e replays stream e % T), which exercises batching:
    every copy must come out identical.  Returns arrays for the first T envs plus `all_equal`."""
    import torch
    if idx is not None:
        streams = streams_from_fixture(fx_or_streams, idx)
        config = fixture_config(fx_or_streams, config)
    else:
        streams = fx_or_streams
    T = len(streams["seeds"])
    E = T * repeat
    A, S = len(config.action_space), config.num_simulations
    own = engine is None
    if own:
        engine = engine_mod.BatchedMCTS(config, E, device=device, seeds=streams["seeds"] * repeat, group_width=group_width)
    else:
        engine.seed(streams["seeds"] * repeat)
    if record_paths:
        engine.set_debug_ties(True)
    if device_noise:
        engine.set_device_noise(True)            # the GPU draws the Dirichlet rows (they reach the host at readout)
    if select_queue:
        engine.set_select_queue(select_queue)   # trees per wavefront of `select` (0 = one descent per lane group)

    def tile(a):
        return np.concatenate([a] * repeat, axis=0)

    engine.begin_search(streams["legal"] * repeat, streams["to_play"] * repeat, True)
    noise = engine.noise.copy()
    engine.expand_roots_injected(tile(streams["root_reward"]), tile(streams["root_priors"]))
    out = _result_arrays(E, A, S)
    value, reward, priors = tile(streams["value"]), tile(streams["reward"]), tile(streams["priors"])
    for s in range(S):
        if s == 0 or not fused_step:
            engine.select(gather=False)
        if record_paths:
            depth, actions, ties = engine.last_paths(with_ties=True)
            out["sim_depth"][:, s] = depth
            out["sim_actions"][:, s, :] = actions
            out["sim_ties"][:, s, :] = ties
        if fused_step and s + 1 < S:     # expand_backup(s) + select(s + 1) in one launch
            engine.expand_backup_select_injected(value[:, s], reward[:, s], priors[:, s, :])
        else:
            engine.expand_backup_injected(value[:, s], reward[:, s], priors[:, s, :])
    st = engine.readout()
    out["noise"][:] = engine.noise if device_noise else noise
    for key in ("visits", "child_value_sum", "child_prior", "child_reward", "root_value_sum", "root_visits",
                "max_tree_depth", "min_max"):
        out[key][:] = st[key]
    out["tie_break_words"] = st["tie_break_words"].copy()
    out["depth_sum"] = st["depth_sum"].copy()
    cv, rv = engine.search_statistics()
    out["child_visits_target"][:] = cv
    out["root_value_target"][:] = rv
    actions, _ = engine.sample_actions(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (T,)).tolist() * repeat)
    out["action"][:] = actions
    torch.cuda.synchronize()
    all_equal = True
    if repeat > 1:
        for key, arr in out.items():
            base = arr[:T]
            for r in range(1, repeat):
                if not np.array_equal(base, arr[r * T:(r + 1) * T]):
                    all_equal = False
    result = {k: v[:T] for k, v in out.items()}
    result["all_equal"] = all_equal
    if own:
        engine.close()
    return result


# ---- models ---------------------------------------------------------------------------------------
def cartpole_model_and_weights(models_mod, config, device="cpu"):
    """The reference's trained CartPole network (weights fixture) on `device`."""
    import torch
    w = load_golden("cartpole_weights")
    weights = {k: torch.from_numpy(w[k]) for k in w.files}
    model = models_mod.MuZeroNetwork(config)
    model.set_weights(weights)
    model.to(device)
    model.eval()
    return model, weights


def synthetic_model(models_mod, config, device="cpu", seed=0):
    """Network with the deterministic synthetic weights of tests/golden/synth.py."""
    import torch
    from synth import synthetic_state_dict
    model = models_mod.MuZeroNetwork(config)
    sd = synthetic_state_dict(model.state_dict(), seed)
    weights = {k: torch.from_numpy(v) for k, v in sd.items()}
    model.set_weights(weights)
    model.to(device)
    model.eval()
    return model, weights


# ---- a fully-connected network in float64, and what float32 kernels may differ from it by ---------------------------
def fc_reference_model(model, dtype=None):
    """A copy of a models.MuZeroFullyConnectedNetwork on the CPU in `dtype` (float64 unless told otherwise): the module's
    own forward, nothing else, is the reference the FC kernels are compared with."""
    import copy
    import torch
    ref = copy.deepcopy(model).cpu().to(dtype if dtype is not None else torch.float64)
    ref._zero_reward_cache = None
    ref.eval()
    return ref


def fc_reference_inference(ref, observations=None, hidden=None, action=None):
    """(value logits, reward logits, policy logits, hidden state) as numpy arrays from `ref` (fc_reference_model):
    initial_inference(observations) or recurrent_inference(hidden, action)."""
    import torch
    dtype = next(ref.parameters()).dtype
    with torch.no_grad():
        if observations is not None:
            out = ref.initial_inference(torch.as_tensor(np.asarray(observations)).to(dtype))
        else:
            act = torch.as_tensor(np.asarray(action)).long().reshape(-1, 1)
            out = ref.recurrent_inference(torch.as_tensor(np.asarray(hidden)).to(dtype), act)
    return tuple(t.to(dtype).numpy().copy() for t in out)      # (the constant reward row of initial_inference is float32)


F32_UNIT = 2.0 ** -24        # unit roundoff of float32


def _mlp_rounding_bound(seq, x, e):
    """Forward `seq` (Linear / ELU stack of a float64 model) on x and carry a bound e on the distance between a float32
    evaluation's activations and these.  A neuron is a sum of m products and a bias in some order (the narrow kernel: two
    FMA chains and one addition; the generic one: FMA chains per lane and a butterfly): every term passes through at most
    m + 1 roundings, so its error is at most gamma(m + 2) (|W| |x| + |b|) on top of |W| e, and nothing when no product is
    non-zero (adding exact zeros to the bias rounds nothing).  ELU is 1-Lipschitz; its exponential and the subtraction of 1
    stay within 2^-23 of the exact value on the negative side."""
    import torch
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    for i, lin in enumerate(linears):
        w, b = lin.weight, lin.bias
        y = x @ w.T + b
        magnitude = (x.abs() + e) @ w.abs().T + b.abs()
        products = (x != 0).to(x.dtype) @ (w != 0).to(x.dtype).T
        k = products + 2.0
        rounding = torch.where(products > 0, k * F32_UNIT / (1.0 - k * F32_UNIT) * magnitude, torch.zeros_like(magnitude))
        e = e @ w.abs().T + rounding
        if i + 1 < len(linears):
            x = torch.nn.functional.elu(y)
            e = e + 2.0 ** -23
        else:
            x = y
    return x, e


def _rescale_rounding_bound(raw, e):
    """models._unit_rescale with the bound carried along: minimum and maximum move by at most max(e); the span takes one
    rounding, the 1e-5 constant is float32's and its addition rounds once more; the quotient (raw - min) / span then
    differs by (e_numerator + quotient * e_span) / (span - e_span) and one rounding.  An input error grows by 1 / span."""
    import torch
    low, high = raw.amin(dim=1, keepdim=True), raw.amax(dim=1, keepdim=True)
    worst = e.amax(dim=1, keepdim=True)
    span = high - low
    undecided = ((span - 1e-5).abs() <= 2.0 * worst + 2.0 * F32_UNIT * 1e-5)
    assert not bool(undecided.any()), "a span within rounding of the 1e-5 threshold: the two evaluations may take different branches"
    span = torch.where(span < 1e-5, span + 1e-5, span)
    e_span = 2.0 * worst + 4.0 * F32_UNIT * span
    numerator = raw - low
    e_numerator = e + worst + F32_UNIT * numerator
    quotient = numerator / span
    return quotient, (e_numerator + quotient * e_span) / (span - e_span) + F32_UNIT * quotient


def fc_rounding_bounds(ref, observations=None, hidden=None, action=None, hidden_error=None):
    """Per-element bounds on |float32 kernel - float64 reference| for (value logits, reward logits, policy logits, hidden
    state) of one inference of `ref` (a float64 fc_reference_model), from the arithmetic alone: inputs and weights are
    float32 numbers, so the first layer starts without error (`hidden_error`: a bound on the hidden input's own distance,
    for chained inferences); see _mlp_rounding_bound / _rescale_rounding_bound.  The reward bound of an initial inference
    is zero (the logits are constants)."""
    import torch
    with torch.no_grad():
        if observations is not None:
            x = torch.as_tensor(np.asarray(observations)).double().reshape(len(observations), -1)
            raw, e = _mlp_rounding_bound(ref.representation_network.module, x, torch.zeros_like(x))
            e_reward = None
        else:
            h = torch.as_tensor(np.asarray(hidden)).double()
            act = torch.as_tensor(np.asarray(action)).long().reshape(-1, 1)
            one_hot = (act == torch.arange(ref.action_space_size)).double()
            x = torch.cat((h, one_hot), dim=1)
            e_in = torch.zeros_like(x)
            if hidden_error is not None:
                e_in[:, :h.shape[1]] = torch.as_tensor(np.asarray(hidden_error)).double()
            raw, e = _mlp_rounding_bound(ref.dynamics_encoded_state_network.module, x, e_in)
            _, e_reward = _mlp_rounding_bound(ref.dynamics_reward_network.module, raw, e)
        state, e_state = _rescale_rounding_bound(raw, e)
        _, e_policy = _mlp_rounding_bound(ref.prediction_policy_network.module, state, e_state)
        _, e_value = _mlp_rounding_bound(ref.prediction_value_network.module, state, e_state)
        if e_reward is None:
            e_reward = torch.zeros_like(e_value)
    return tuple(t.numpy() for t in (e_value, e_reward, e_policy, e_state))


# ---- the value transform seen as an error amplifier (reference models.py:641-662) ----------------------
def categorical_mean(logits, support_size):
    """x = sum(softmax(logits) * [-s .. s]) in float64 (the quantity the inverse transform is applied to)."""
    logits = np.asarray(logits, dtype=np.float64)
    p = np.exp(logits - logits.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    return (p * np.arange(-support_size, support_size + 1, dtype=np.float64)).sum(axis=-1)


def categorical_mean_bound(logit_deviation, support_size):
    """|x' - x| for logits that differ by at most `logit_deviation` per entry: the soft-max moves by
    ||p' - p||_1 <= 2 * ||l' - l||_inf (to first order; 1 % margin for the rest) and |x' - x| <= s * ||p' - p||_1."""
    return 2.02 * support_size * logit_deviation


def value_transform_bound(value, delta_x, eps=0.001):
    """Bound on |support_to_scalar(l') - support_to_scalar(l)| for decoded value `value` (either of the two) when the
    categorical means differ by at most delta_x, both decodes evaluated in float32 in the reference's operation order:

        v = sign(x) * (z**2 - 1),   z = (sqrt(1 + 4 eps (|x| + 1 + eps)) - 1) / (2 eps)       (models.py:655-660)

    * analytic part: dv/dx = 2 z / u with u = 1 + 2 eps z (= 2 at x = 0, growing like 2 sqrt(|v| + 1)): kappa * delta_x;
    * granularity of the float32 evaluation, by forward error analysis of the seven operations (half an ulp each; the
      soft-max and the weighted sum that produce x are charged 8 ulps).  What dominates: w = 1 + 4 eps (...) lies in
      [1, 2) for |x| < 249, where float32 numbers are 2**-23 apart, and so does u = sqrt(w); u - 1 is exact, so
      z = (u - 1) / (2 eps) lives on a lattice of spacing 2**-23 / (2 eps) = 6.0e-5 and v = z**2 - 1 moves in steps of
      2 z * 6.0e-5 = 1.2e-4 * sqrt(|v| + 1).  The reference's own output cannot resolve anything finer
      (tests/test_value_bound.py shows fixture G1 sitting on that lattice); each of the two evaluations carries this error.
    Returns kappa(|x| + delta_x) * delta_x + 2 * (rounding error of one evaluation)."""
    f32 = np.float32

    def ulp(a):
        return np.spacing(np.asarray(a, dtype=np.float64).astype(f32)).astype(np.float64)

    value = np.abs(np.asarray(value, dtype=np.float64))
    delta_x = np.asarray(delta_x, dtype=np.float64)
    z = np.sqrt(value + 1.0) + delta_x                     # (z grows by at most dz/dx * delta_x <= delta_x)
    x = z - 1.0 + eps * (z * z - 1.0)                      # the forward transform h(v), models.py:665-671
    u = 1.0 + 2.0 * eps * z
    kappa = 2.0 * z / u
    e_x = 8.0 * ulp(np.maximum(x, 1.0))
    t = x + 1.0 + eps
    e_t = e_x + ulp(t)                                     # two additions
    e_m = 4.0 * eps * e_t + 0.5 * ulp(4.0 * eps * t)
    e_w = e_m + 0.5 * ulp(u * u)
    e_u = e_w / (2.0 * u) + 0.5 * ulp(u)
    e_z = e_u / (2.0 * eps) + 0.5 * ulp(z)                 # (u - 1 is exact)
    e_s = 2.0 * z * e_z + 0.5 * ulp(z * z)
    e_v = e_s + 0.5 * ulp(np.maximum(z * z - 1.0, 1e-30))
    return 1.01 * kappa * delta_x + 2.0 * e_v


def inverse_value_transform64(x, eps=0.001):
    """models.py:655-660 in float64: sign(x) * (z**2 - 1), z = (sqrt(1 + 4 eps (|x| + 1 + eps)) - 1) / (2 eps)."""
    x = np.asarray(x, dtype=np.float64)
    z = (np.sqrt(1.0 + 4.0 * eps * (np.abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    return np.sign(x) * (z * z - 1.0)


def support_to_scalar64(logits, support_size):
    """models.py:641-662 on float32 logits, every operation in float64: the yardstick of the decode tests."""
    return inverse_value_transform64(categorical_mean(logits, support_size))


def _gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * F32_UNIT / (1.0 - k * F32_UNIT)


def _softmax_terms(logits):
    """float64 soft-max of the rows of `logits` with what its float32 evaluation is charged per entry BEFORE any
    summation: d_i = fl(l_i - max) carries one rounding, i.e. |d_i| u on the exponent and so a relative |d_i| u on
    exp(d_i); expf itself is good to one ulp = 2 u.  Returns (p, |d| with the -inf entries at 0, c = sum p (|d| + 2)):
    c u is the relative error those two leave on the normaliser sum exp(d_k), whatever order it is added in."""
    logits = np.asarray(logits, dtype=np.float64)
    d = logits - logits.max(axis=-1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(axis=-1, keepdims=True)
    absd = np.where(np.isfinite(d), np.abs(d), 0.0)
    absd = np.where(p > 0, absd, 0.0)                      # (exp underflows in float64 too: the entry is exactly 0 in both)
    return p, absd, (p * (absd + 2.0)).sum(axis=-1, keepdims=True)


def categorical_mean_rounding(logits, support_size, group=1):
    """delta_x: bound on |x_f32 - x| for x = sum_i (i - s) softmax(l)_i evaluated in float32 by a lane group of `group`
    lanes (tree_device.h support_to_scalar_pair; group = 1 is any sequential or vectorised sum of F terms: the C oracle,
    torch), against the float64 value of the same float32 logits.  The usual gamma_n argument, per entry i:

        exp(fl(l_i - max))              |d_i| + 2            (see _softmax_terms; the maximum itself is exact)
        the normaliser Z                c + n                the entries' own errors, and a sum in which every term
                                                             passes through at most n = ceil(F / G) + log2(G) additions
                                                             (a lane's chain, then the butterfly)
        1 / Z, e_i * (1 / Z), (i - s) * p_i     3            one rounding each; (i - s) is an exact float
        the weighted sum                n                    the same chain and butterfly

    so x_f32 = sum_i (i - s) p_i (1 + theta_i) with |theta_i| <= gamma(2 n + 5 + |d_i| + c) and
    delta_x = sum_i |i - s| p_i gamma(...): small when the mass sits near the centre, up to s * gamma for a peaked row.
    Entries whose exponential leaves float32's normal range (p_i < 2**-126) are charged absolutely.  1 % for the second
    order.  A single non-zero probability, at the maximum, costs nothing at all: every operation on it is exact."""
    p, absd, c = _softmax_terms(logits)
    F = p.shape[-1]
    n = -(-F // group) + int(np.log2(group))
    weight = np.abs(np.arange(-support_size, support_size + 1, dtype=np.float64))
    lone = (p > 0).sum(axis=-1) == 1                       # exp(0) = 1, Z = 1, 1 / Z = 1, (i - s) * 1, + 0: all exact
    bound = 1.01 * (weight * p * _gamma(2 * n + 5 + absd + c)).sum(axis=-1) + weight.sum() * 2.0 ** -126
    return np.where(lone, 0.0, bound)


def softmax_rounding_bound(logits, group=1, chunks=1):
    """Per-entry bound on |softmax_f32(l) - softmax(l)| (tree_device.h group_softmax: `chunks` entries per lane, then a
    butterfly over `group` lanes; group = 1, chunks = n is a sequential sum of n terms: the C oracle, torch): relative
    gamma(|d_i| + 2 + c + (chunks - 1 + log2(group)) + 2) by the argument of categorical_mean_rounding (own exponential,
    the normaliser's entries and its sum, the reciprocal and the product), plus 2**-126 where float32 leaves its normal
    range.  A row with a single non-zero entry is exact."""
    p, absd, c = _softmax_terms(logits)
    k = absd + 2.0 + c + (chunks - 1 + int(np.log2(group))) + 2.0
    lone = ((p > 0).sum(axis=-1, keepdims=True) == 1)
    return np.where(lone, 0.0, 1.01 * p * _gamma(k) + 2.0 ** -126)


def softmax64(logits):
    return _softmax_terms(logits)[0]


TOWER_CHAIN_BAR = 4e-7       # |fp32 k-ordered chain - float64| / sum |a b|: the bar tests/test_gpu_board_conv.py holds a
                             # single layer of both tower forms to (test_random_data_within_one_fp32_chain_of_fp64,
                             # test_split_tower_single_layer_against_fp64)


def tower_layer_rounding_bound(magnitude, conv, scale, shift, skip=None, split_store=False):
    """Per-element bound on |tower layer in float32 - the same layer in float64 on the same float32 input| for
    csrc/board_conv.hip's layer  v = conv * scale + shift; v += skip; relu(v)  (the epilogue's operation order, separate
    multiply and add: the library is built without contraction):

        the accumulation     TOWER_CHAIN_BAR * sum |a b| (`magnitude`), carried through the multiply: * |scale|
        conv * scale         one rounding, half an ulp of the product:        u (|conv scale| + e)
        + shift              one rounding of the sum:                         u (|conv scale + shift| + e)
        + skip               one more where the layer has one (the skip planes are the run's own float32 values)
        ReLU                 1-Lipschitz, exact

    with u = 2^-24 and e the error carried so far (second order, kept so that the bound is one).  `split_store`: the split
    form keeps the result as two fp16 halves of 8 v (h0 to 11 bits, the remainder to 11 more: a relative 2^-22; a
    remainder in fp16's subnormal range is held to 2^-25, that is 2^-28 of v) -- what its export shows carries that too.
    conv, magnitude: float64 [b, cout, h, w]; scale, shift: [cout]; skip: as conv, or None."""
    cout = conv.shape[1]
    scale = np.asarray(scale, dtype=np.float64).reshape(1, cout, 1, 1)
    shift = np.asarray(shift, dtype=np.float64).reshape(1, cout, 1, 1)
    e = TOWER_CHAIN_BAR * np.asarray(magnitude, dtype=np.float64) * np.abs(scale)
    t = conv * scale
    e = e + F32_UNIT * (np.abs(t) + e)
    t = t + shift
    e = e + F32_UNIT * (np.abs(t) + e)
    if skip is not None:
        t = t + skip
        e = e + F32_UNIT * (np.abs(t) + e)
    if split_store:
        e = e + 2.0 ** -22 * (np.abs(t) + e) + 2.0 ** -28
    return e


def dot_layer_rounding_bound(x, e, w, b):
    """_mlp_rounding_bound's layer in numpy, for one affine layer y = x w^T + b of the conv heads (csrc/net_kernels.hip,
    board_heads_cols_kernel) and of the down-sampler's two convolutions seen as rows of patches: x [n, K] float64 with a
    bound e [n, K] on the float32 evaluation's distance from it, w [m, K], b [m].  Returns (y, e_out).

    Every term of a K-term dot product plus bias passes through at most K + 1 roundings in each of the kernels' forms:
      * the matrix cores' k-ordered chain of fused multiply-adds (conv_head_mfma_kernel, the cols heads, the down-sampler):
        the first term is rounded K times by the chain and once by the bias; k-steps padded with zeros round nothing;
      * Linear-1's four `kParts` chains and their three additions: a term of a chain of n terms sees n roundings there, at
        most m - 1 additions of the m <= 4 chains that hold anything (a chain of exact zeros adds exactly) and the bias;
        each of the other m - 1 chains holds a term or more, so n + m - 1 <= K;
      * conv_head_kernel (no contraction): the product rounds once, is added to 0 exactly, then n - 1 additions of its
        `split` partial sum, at most m - 1 additions of the partial sums in order and the bias: n + m <= K + 1 again.
    So the layer's error is at most gamma(K + 2) (|w| (|x| + e) + |b|) on top of |w| e, with K counted per output as the
    products that are not zero (adding an exact zero rounds nothing), and nothing at all where no product is non-zero."""
    x, e, w, b = (np.asarray(a, dtype=np.float64) for a in (x, e, w, b))
    y = x @ w.T + b
    magnitude = (np.abs(x) + e) @ np.abs(w).T + np.abs(b)
    products = (x != 0).astype(np.float64) @ (w != 0).astype(np.float64).T
    rounding = np.where(products > 0, _gamma(products + 2.0) * magnitude, 0.0)
    return y, e @ np.abs(w).T + rounding


def head_rounding_bound(x, conv_w, conv_b, w1, b1, w2, b2):
    """Per-logit bound on |float32 head - float64 head| for float32 boards x [B, C, P] and float32 parameters:
    dot_layer_rounding_bound for the 1x1 convolution (rows = (sample, position) pairs, K = C), Linear-1 (K = R P) and
    Linear-2 (K = Hd); ELU is 1-Lipschitz and its exponential and `- 1` stay within 2^-23 of the exact value on the
    negative side (charged on every unit, as _mlp_rounding_bound does; tests/test_gpu_device_numerics.py's
    MZMCTS_NUMERICS_EXP sweep holds expf to that).  Returns e [B, O]."""
    x = np.asarray(x, dtype=np.float64)
    batch, channels, plane = x.shape
    rows = x.transpose(0, 2, 1).reshape(batch * plane, channels)
    y, e = dot_layer_rounding_bound(rows, np.zeros_like(rows), conv_w, conv_b)
    reduced = y.shape[1]
    flat = y.reshape(batch, plane, reduced).transpose(0, 2, 1).reshape(batch, reduced * plane)
    e = e.reshape(batch, plane, reduced).transpose(0, 2, 1).reshape(batch, reduced * plane)
    pre, e = dot_layer_rounding_bound(flat, e, w1, b1)
    hidden = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0.0)))
    _, e = dot_layer_rounding_bound(hidden, e + 2.0 ** -23, w2, b2)
    return e


def window_mean_rounding_bound(values, e):
    """The adaptive average of the down-sampler: `values` [..., n] are a window's n float64 numbers, e the bounds they
    carry.  The float32 kernel adds them one by one (the first to an exact 0: n - 1 roundings) and divides once: the
    mean of e, and gamma(n) of the mean of (|v| + e)."""
    n = values.shape[-1]
    return e.mean(axis=-1) + _gamma(n) * (np.abs(values) + e).mean(axis=-1)


# ---- replay store ------------------------------------------------------------------------------
def history_of(sp, fx, g):
    """Game g of a replay fixture (G12 layout: arrays padded past `lengths[g]`) as a GameHistory with the field types
    play_game leaves behind."""
    n = int(fx["lengths"][g])
    gh = sp.GameHistory()
    gh.observation_history = [o for o in fx["observations"][g, : n + 1]]
    gh.action_history = [int(a) for a in fx["actions"][g, : n + 1]]
    gh.reward_history = [float(r) for r in fx["rewards"][g, : n + 1]]
    gh.to_play_history = [int(t) for t in fx["to_play"][g, : n + 1]]
    gh.child_visits = [[float(v) for v in row] for row in fx["child_visits"][g, :n]]
    gh.root_values = [float(v) for v in fx["root_values"][g, :n]]
    return gh
