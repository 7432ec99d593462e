"""One training step of a MuZeroFullyConnectedNetwork in float64 numpy, written without autograd: the yardstick of the
HIP training step (csrc/fc_train.hip, csrc/fc_backward.h).

`unroll64` restates the forward (Trainer._unroll on models.MuZeroFullyConnectedNetwork), the loss (unroll_loss_reference.
unroll_loss64, whose two-hot targets are the float32 ones the loss kernel forms), the backward rule and the weight
gradients of loss.mean().  It also returns, per position (sample b, step k), what the kernels keep: every layer's input,
the raw and the normalised state, the rescale's min index, max index and scale, and the gradient of every layer's
pre-activation -- in the record layout of `record_layout`, which tests/fc_backward_check.cpp reads.

Beside every gradient it carries the sum of the absolute values of the terms it is made of (the same walk on |weights|,
|slopes|, |gradients|) and the length of the longest chain of float32 operations that leads to it: a float32 evaluation
that rounds every operation once differs from the exact value by at most gamma(n) * sum|terms|, n the chain length.

DEFECTS are deliberate mistakes; tests/test_fc_train_reference.py shows that each of them is seen.
"""
import types

import numpy as np

from unroll_loss_reference import unroll_loss64

U = 2.0 ** -24

MLPS = ("representation_network", "dynamics_encoded_state_network", "dynamics_reward_network",
        "prediction_policy_network", "prediction_value_network")

DEFECTS = ("half_dropped", "half_on_dynamics_share_only", "reward_reads_normalised", "min_scale_constant",
           "small_scale_branch_ignored", "elu_slope_without_exponential", "mean_factor_missing", "one_hot_off_by_one",
           "step_0_reward_counted")


def shape(obs, enc, hidden, A, support, cases, stacked=0, frame=None):
    hidden = [list(h) for h in (hidden * 5 if len(hidden) == 1 else hidden)]
    return dict(obs=obs, enc=enc, hidden=hidden, A=A, support=support, cases=cases, stacked=stacked, frame=frame or obs)


# obs, enc, hidden widths of representation / dynamics / reward / policy / value, A, support; the (B, K1) cases
SHAPES = {
    "S1": shape(4, 8, [[16]], 2, 10, [(1, 1), (5, 3), (33, 11)]),
    "S2": shape(9, 5, [[15], [17], [33], [16], [1]], 3, 1, [(17, 2)]),
    "S3": shape(4, 1, [[]], 2, 10, [(4, 3)]),
    "S4": shape(256, 32, [[8, 24, 16]], 121, 127, [(3, 2)]),
    "S5": shape(9, 5, [[16]], 2, 10, [(16, 7)]),
    "S6": shape(27, 32, [[16]], 2, 10, [(16, 6)]),
    "S1stacked": shape(19, 8, [[16]], 2, 10, [(5, 3)], stacked=3, frame=4),
}
# model seeds for which every row of every case keeps its two smallest and its two largest state entries 1e-4 apart and
# its scale away from 1e-5 (test_fc_train_reference.py asserts it)
SEEDS = {"S1": 1, "S2": 1, "S3": 1, "S4": 1, "S5": 1, "S6": 1, "S1stacked": 1}
LAST_LAYER_GAIN = 4.0


def config_for(sh):
    """What models.MuZeroNetwork reads of a MuZeroConfig."""
    return types.SimpleNamespace(
        network="fullyconnected", observation_shape=(sh["frame"], 1, 1), stacked_observations=sh["stacked"],
        action_space=list(range(sh["A"])), encoding_size=sh["enc"], fc_representation_layers=sh["hidden"][0],
        fc_dynamics_layers=sh["hidden"][1], fc_reward_layers=sh["hidden"][2], fc_policy_layers=sh["hidden"][3],
        fc_value_layers=sh["hidden"][4], support_size=sh["support"])


def make_model(models, sh, seed):
    """models.MuZeroNetwork at a fixed seed, the last layer of every MLP scaled up: ELU sees both signs, states spread out."""
    import torch
    torch.manual_seed(seed)
    model = models.MuZeroNetwork(config_for(sh))
    with torch.no_grad():
        for name in MLPS:
            linears = [m for m in getattr(model, name).module if isinstance(m, torch.nn.Linear)]
            linears[-1].weight.mul_(LAST_LAYER_GAIN)
    return model


def layers_of(state, mlp):
    """[(weight, bias)] of one MLP out of a state dict (numpy), in layer order."""
    out, index = [], 0
    while f"{mlp}.module.{index}.weight" in state:
        out.append((np.asarray(state[f"{mlp}.module.{index}.weight"]), np.asarray(state[f"{mlp}.module.{index}.bias"])))
        index += 2
    return out


def parameter_names(state):
    return [k for k in state if k.split(".")[0] in MLPS]


def make_batch(sh, B, K1, seed, weights="none", scales="random", bad_actions=False):
    """The seven batch entries as numpy arrays (float32; actions int64 [B, K1])."""
    rng = np.random.RandomState(1000 + seed)
    A = sh["A"]
    policies = rng.rand(B, K1, A).astype(np.float32) + 0.05
    policies /= policies.sum(axis=2, keepdims=True)
    batch = {
        "observations": rng.randn(B, sh["obs"]).astype(np.float32),
        "actions": rng.randint(0, A, size=(B, K1)).astype(np.int64),
        "values": (rng.randn(B, K1) * 10).astype(np.float32),
        "rewards": rng.randn(B, K1).astype(np.float32),
        "policies": policies.astype(np.float32),
        "weights": None if weights == "none" else (rng.rand(B) + 0.5).astype(np.float32),
        "gradient_scales": (rng.randint(1, K1 + 1, size=(B, K1)).astype(np.float32) if scales == "random"
                            else np.ones((B, K1), dtype=np.float32)),
    }
    if bad_actions:
        batch["actions"][::2, 1:] = -1
        batch["actions"][1::3, 1:] = A
    return batch


# ---- the record of a position ------------------------------------------------------------------------------------------
def record_layout(sh):
    """Offsets (floats) of a position's record: x | raw | norm | reward | value | policy | every hidden layer | stats.
    Returns (offsets dict, per MLP per layer (x_off, y_off), record floats)."""
    F = 2 * sh["support"] + 1
    off, at = {}, 0
    for name, size in (("x", max(sh["obs"], sh["enc"] + sh["A"])), ("raw", sh["enc"]), ("norm", sh["enc"]), ("reward", F),
                       ("value", F), ("policy", sh["A"])):
        off[name] = at
        at += size
    first = {0: "x", 1: "x", 2: "raw", 3: "norm", 4: "norm"}
    last = {0: "raw", 1: "raw", 2: "reward", 3: "policy", 4: "value"}
    places = []
    for m in range(5):
        widths = sh["hidden"][m]
        hidden = []
        for width in widths:
            hidden.append(at)
            at += width
        n = len(widths) + 1
        places.append([(off[first[m]] if l == 0 else hidden[l - 1], off[last[m]] if l == n - 1 else hidden[l])
                       for l in range(n)])
    off["stats"] = at
    return off, places, at + 3


def elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def _mlp_forward(layers, x):
    inputs = []
    for l, (W, b) in enumerate(layers):
        inputs.append(x)
        z = x @ W.T + b
        x = elu(z) if l < len(layers) - 1 else z
    return inputs, x


class _Tracked:
    """A gradient with the sum of |terms| it is made of and the float32 chain length behind it."""

    def __init__(self, value, mag=None, n=0):
        self.v, self.m, self.n = value, (np.abs(value) if mag is None else mag), n


def _mlp_backward(layers, inputs, delta, grads, mags, chains, deltas, defect, want_input=True):
    """delta: _Tracked [B, out of the last layer].  Adds the layers' weight gradients into grads / mags (lists of [dW, db]),
    stores each layer's delta in deltas[l], returns the gradient of the MLP's input."""
    for l in range(len(layers) - 1, -1, -1):
        W = layers[l][0]
        x = inputs[l]
        deltas[l] = delta
        grads[l][0] += delta.v.T @ x
        grads[l][1] += delta.v.sum(axis=0)
        mags[l][0] += delta.m.T @ np.abs(x)
        mags[l][1] += delta.m.sum(axis=0)
        chains[l] = max(chains[l], delta.n + 2)
        if l == 0 and not want_input:
            return None
        g = _Tracked(delta.v @ W, delta.m @ np.abs(W), delta.n + W.shape[0] + 1)
        if l == 0:
            return g
        y = x                                         # the ELU output of layer l - 1
        if defect == "elu_slope_without_exponential":
            slope, slope_mag = np.ones_like(y), np.ones_like(y)
        else:
            slope, slope_mag = np.where(y > 0, 1.0, y + 1.0), np.where(y > 0, 1.0, np.abs(y) + 1.0)
        delta = _Tracked(g.v * slope, g.m * slope_mag, g.n + 3)
    return None


def unroll64(state, batch, sh, value_loss_weight=0.25, per_alpha=0.5, defect=None):
    """state: the network's state dict (anything numpy.asarray takes); batch: make_batch's dict.  Everything in float64."""
    assert defect is None or defect in DEFECTS, defect
    nets = [[(np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)) for W, b in layers_of(state, name)]
            for name in MLPS]
    repr_, dyn, reward, policy, value = nets
    obs = np.asarray(batch["observations"], dtype=np.float64).reshape(len(batch["observations"]), -1)
    actions = np.asarray(batch["actions"]).reshape(obs.shape[0], -1)
    B, K1 = actions.shape
    A, enc, F = sh["A"], sh["enc"], 2 * sh["support"] + 1
    off, places, R = record_layout(sh)
    act = np.zeros((B, K1, R))
    del_ = np.zeros((B, K1, R))
    del_mag, del_chain = np.zeros((B, K1, R)), np.zeros((B, K1, R))

    def rescale(raw):
        imin, imax = raw.argmin(axis=1), raw.argmax(axis=1)            # (the first index that attains it)
        mn, mx = raw.min(axis=1, keepdims=True), raw.max(axis=1, keepdims=True)
        span = mx - mn
        scale = span if defect == "small_scale_branch_ignored" else np.where(span < 1e-5, span + 1e-5, span)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (raw - mn) / scale, imin, imax, scale

    saved = []
    logits = {"value": np.zeros((K1, B, F)), "reward": np.zeros((K1, B, F)), "policy": np.zeros((K1, B, A))}
    hidden = None
    for k in range(K1):
        if k == 0:
            x = obs
            pre_inputs, raw = _mlp_forward(repr_, x)
        else:
            shift = 1 if defect == "one_hot_off_by_one" else 0
            one_hot = (actions[:, k][:, None] + shift == np.arange(A)[None, :]).astype(np.float64)
            x = np.concatenate([hidden, one_hot], axis=1)
            pre_inputs, raw = _mlp_forward(dyn, x)
        norm, imin, imax, scale = rescale(raw)
        reward_in = norm if defect == "reward_reads_normalised" else raw
        head_inputs = {}
        if k > 0 or defect == "step_0_reward_counted":
            head_inputs["reward"], logits["reward"][k] = _mlp_forward(reward, reward_in)
        head_inputs["policy"], logits["policy"][k] = _mlp_forward(policy, norm)
        head_inputs["value"], logits["value"][k] = _mlp_forward(value, norm)
        saved.append(dict(pre=pre_inputs, raw=raw, norm=norm, imin=imin, imax=imax, scale=scale, heads=head_inputs))
        hidden = norm
        # the record
        act[:, k, off["x"]:off["x"] + x.shape[1]] = x
        act[:, k, off["raw"]:off["raw"] + enc] = raw
        act[:, k, off["norm"]:off["norm"] + enc] = norm
        act[:, k, off["stats"]:off["stats"] + 3] = np.stack([imin, imax, scale[:, 0]], axis=1)
        for m, inputs in ((0 if k == 0 else 1, pre_inputs), (2, head_inputs.get("reward")), (3, head_inputs["policy"]),
                          (4, head_inputs["value"])):
            if inputs is None:
                continue
            for l in range(1, len(inputs)):
                x_off = places[m][l][0]
                act[:, k, x_off:x_off + inputs[l].shape[1]] = inputs[l]

    case = {"value": logits["value"], "reward": logits["reward"], "policy": logits["policy"],
            "target_value": np.asarray(batch["values"], dtype=np.float32),
            "target_reward": np.asarray(batch["rewards"], dtype=np.float32),
            "target_policy": np.asarray(batch["policies"], dtype=np.float32),
            "gradient_scale": np.asarray(batch["gradient_scales"], dtype=np.float32),
            "weight": None if batch["weights"] is None else np.asarray(batch["weights"], dtype=np.float32),
            "support": sh["support"], "value_loss_weight": value_loss_weight, "per_alpha": per_alpha}
    loss = unroll_loss64(case, mutation="step_0_reward_counted" if defect == "step_0_reward_counted" else None)

    inv_b = 1.0 if defect == "mean_factor_missing" else 1.0 / B
    grads = [[[np.zeros_like(W), np.zeros_like(b)] for W, b in net] for net in nets]
    mags = [[[np.zeros_like(W), np.zeros_like(b)] for W, b in net] for net in nets]
    chains = [[0] * len(net) for net in nets]
    g_hidden = None
    for k in range(K1 - 1, -1, -1):
        s = saved[k]
        deltas = {m: [None] * len(nets[m]) for m in range(5)}

        def head(m, name):
            top = _Tracked(loss["grad_" + name][k] * inv_b, n=3)
            return _mlp_backward(nets[m], s["heads"][name], top, grads[m], mags[m], chains[m], deltas[m], defect)

        g_p, g_v = head(3, "policy"), head(4, "value")
        g_r = head(2, "reward") if "reward" in s["heads"] else None
        total = _Tracked(g_p.v + g_v.v, g_p.m + g_v.m, max(g_p.n, g_v.n) + 1)
        if defect == "reward_reads_normalised" and g_r is not None:
            total = _Tracked(total.v + g_r.v, total.m + g_r.m, max(total.n, g_r.n) + 1)
        if g_hidden is not None:
            share = 0.5 if defect == "half_on_dynamics_share_only" else 1.0
            total = _Tracked(total.v + share * g_hidden.v, total.m + share * g_hidden.m, max(total.n, g_hidden.n) + 1)
        if k > 0 and defect not in ("half_dropped", "half_on_dynamics_share_only"):
            total = _Tracked(0.5 * total.v, 0.5 * total.m, total.n)
        # the rescale
        scale, norm = s["scale"], s["norm"]
        with np.errstate(divide="ignore", invalid="ignore"):
            g_raw, m_raw = total.v / scale, total.m / scale
            if defect != "min_scale_constant":
                s1, s2 = total.v.sum(axis=1), (total.v * norm).sum(axis=1)
                m1, m2 = total.m.sum(axis=1), (total.m * np.abs(norm)).sum(axis=1)
                d_scale, d_min = -s2 / scale[:, 0], -s1 / scale[:, 0]
                rows = np.arange(B)
                same = s["imin"] == s["imax"]
                g_raw[rows, s["imax"]] += np.where(same, 0.0, d_scale)
                g_raw[rows, s["imin"]] += np.where(same, d_min, d_min - d_scale)
                m_raw[rows, s["imax"]] += np.where(same, 0.0, m2 / scale[:, 0])
                m_raw[rows, s["imin"]] += np.where(same, m1 / scale[:, 0], (m1 + m2) / scale[:, 0])
        n_raw = total.n + enc + 8
        if g_r is not None and defect != "reward_reads_normalised":
            g_raw, m_raw, n_raw = g_raw + g_r.v, m_raw + g_r.m, max(n_raw, g_r.n) + 1
        top = _Tracked(g_raw, m_raw, n_raw)
        m_pre = 0 if k == 0 else 1
        g_in = _mlp_backward(nets[m_pre], s["pre"], top, grads[m_pre], mags[m_pre], chains[m_pre], deltas[m_pre], defect,
                             want_input=k > 0)
        g_hidden = _Tracked(g_in.v[:, :enc], g_in.m[:, :enc], g_in.n) if k > 0 else None
        for m in range(5):
            for l, d in enumerate(deltas[m]):
                if d is not None:
                    y_off = places[m][l][1]
                    del_[:, k, y_off:y_off + d.v.shape[1]] = d.v
                    del_mag[:, k, y_off:y_off + d.v.shape[1]] = d.m
                    del_chain[:, k, y_off:y_off + d.v.shape[1]] = d.n

    names = {}
    for m, mlp in enumerate(MLPS):
        for l in range(len(nets[m])):
            for t, kind in enumerate(("weight", "bias")):
                names[f"{mlp}.module.{2 * l}.{kind}"] = (grads[m][l][t], mags[m][l][t], chains[m][l])
    return {"logits": logits, "loss": loss, "act": act, "del": del_, "del_mag": del_mag, "del_chain": del_chain,
            "grads": {k: v[0] for k, v in names.items()}, "grad_mags": {k: v[1] for k, v in names.items()},
            "grad_chains": {k: v[2] for k, v in names.items()},
            "states": np.stack([s["raw"] for s in saved], axis=1), "scales": np.stack([s["scale"][:, 0] for s in saved], axis=1)}


def state_spread_ok(out, enc):
    """The conditions on the inputs: in every row the two smallest and the two largest raw state entries at least 1e-4
    apart, the scale not within 1e-6 of 1e-5.  Returns (ok, worst gap, closest scale distance)."""
    states = np.sort(out["states"], axis=2)
    gaps = np.inf if enc < 2 else min(float((states[..., 1] - states[..., 0]).min()), float((states[..., -1] - states[..., -2]).min()))
    distance = float(np.abs(out["scales"] - 1e-5).min())
    return gaps >= 1e-4 and distance > 1e-6, gaps, distance


def flat_offsets(sh):
    """(w_off, b_off) per MLP per layer in the flat buffer: every Linear's weight then bias, in state_dict order."""
    F = 2 * sh["support"] + 1
    ins = [sh["obs"], sh["enc"] + sh["A"], sh["enc"], sh["enc"], sh["enc"]]
    outs = [sh["enc"], sh["enc"], F, sh["A"], F]
    at, table, widths_of = 0, [], []
    for m in range(5):
        widths = [ins[m], *sh["hidden"][m], outs[m]]
        rows = []
        for fan_in, fan_out in zip(widths[:-1], widths[1:]):
            rows.append((at, at + fan_in * fan_out))
            at += fan_in * fan_out + fan_out
        table.append(rows)
        widths_of.append(widths)
    return table, widths_of, at


def flatten(state, dtype=np.float32):
    """The flat buffer of a state dict (or of a dict of gradients keyed alike)."""
    parts = []
    for mlp in MLPS:
        index = 0
        while f"{mlp}.module.{index}.weight" in state:
            parts += [np.asarray(state[f"{mlp}.module.{index}.weight"]).reshape(-1), np.asarray(state[f"{mlp}.module.{index}.bias"]).reshape(-1)]
            index += 2
    return np.concatenate(parts).astype(dtype)
