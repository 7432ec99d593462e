"""The training-loss kernel (csrc/trainer_kernels.hip unroll_loss_kernel, C entry mztrain_unroll_loss) against float64.

The C entry is driven through ctypes on raw device buffers, one launch per case of tests/unroll_loss_cases.py: EVERY element
of sample_loss, head_sums, priorities and the three gradient tensors is held to unroll_loss64 (tests/unroll_loss_reference.py)
within its own bound, derived from the kernel's operation order; non-finite expectations are met by the same non-finite
class.  What needs no tolerance is asserted bit for bit: the two-hot targets the kernel really uses (through the gradient
rows of a probe launch, against the numpy float32 restatement two_hot32), the ignored reward row of step 0, the exact
cases, per_alpha = 0, permuted batches, the guard bands round every output.  Then the autograd wrapper under a non-uniform
upstream gradient and from non-contiguous views, and one whole training step of two networks against the same model in
float64.  The worst error / bound ratio per shape and output family is printed (-s shows it) and collected, with the
charged logf / powf figures, in measure_out/unroll_loss_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

from unroll_loss_cases import SHAPES, STAND_IN, describe, make_case, probe_case, shape_id
from unroll_loss_reference import (F32_UNIT, LOGF_ULPS, OUTPUTS, POWF_ULPS, compare, torch_reference,
                                   two_hot_rows, unroll_loss64, unroll_loss_bounds)

pytestmark = pytest.mark.gpu

GUARD = 256                   # floats of NaN before and after every output buffer
REPORT = {"logf_ulps_charged": LOGF_ULPS, "powf_ulps_charged": POWF_ULPS, "shapes": {}, "training_step": {}}


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "unroll_loss_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def launch(native, case):
    """One mztrain_unroll_loss launch on raw buffers; outputs as numpy float32 arrays keyed like the struct.  Every output
    lies between two NaN-filled guard bands, which must come back untouched."""
    B, K1, s, A = case["B"], case["K1"], case["support"], case["A"]
    F = 2 * s + 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(case[k], dtype=np.float32)).cuda()
           for k in ("value", "reward", "policy", "target_value", "target_reward", "target_policy", "gradient_scale")}
    weight = None if case["weight"] is None else torch.from_numpy(np.ascontiguousarray(case["weight"], dtype=np.float32)).cuda()
    assert dev["value"].shape == (K1, B, F) and dev["reward"].shape == (K1, B, F) and dev["policy"].shape == (K1, B, A)
    assert dev["target_value"].shape == (B, K1) and dev["target_policy"].shape == (B, K1, A)
    assert dev["gradient_scale"].shape == (B, K1) and (weight is None or weight.shape == (B,))
    shapes = {"sample_loss": (B,), "head_sums": (3, B), "priorities": (B, K1), "grad_value": (K1, B, F),
              "grad_reward": (K1, B, F), "grad_policy": (K1, B, A)}
    buffers = {k: torch.full((int(np.prod(shape)) + 2 * GUARD,), float("nan"), device="cuda") for k, shape in shapes.items()}
    args = native.MzTrainLossArgs(
        value_logits=dev["value"].data_ptr(), reward_logits=dev["reward"].data_ptr(), policy_logits=dev["policy"].data_ptr(),
        target_value=dev["target_value"].data_ptr(), target_reward=dev["target_reward"].data_ptr(),
        target_policy=dev["target_policy"].data_ptr(), gradient_scale=dev["gradient_scale"].data_ptr(),
        weight=weight.data_ptr() if weight is not None else None, batch=B, steps=K1, support_size=s, actions=A,
        value_loss_weight=float(case["value_loss_weight"]), per_alpha=float(case["per_alpha"]),
        **{k: buf.data_ptr() + 4 * GUARD for k, buf in buffers.items()})
    torch.cuda.synchronize()
    rc = native.load().mztrain_unroll_loss(ctypes.byref(args), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    for k, buf in buffers.items():
        host = buf.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all(), f"{k}: a guard band was written"
        out[k] = host[GUARD:-GUARD].reshape(shapes[k]).copy()
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


CASES = list(enumerate(SHAPES))


@pytest.mark.parametrize("index,shape", CASES, ids=[shape_id(*s) for s in SHAPES])
def test_every_output_element_vs_float64(native, index, shape):
    case = make_case(*shape, index=index)
    B, K1 = case["B"], case["K1"]
    got = launch(native, case)
    ref = unroll_loss64(case)
    report = compare(got, ref, unroll_loss_bounds(case, ref, group=64))
    print(f"\n{case['id']} (weights {case['weight_mode']}, vw {case['value_loss_weight']}, alpha {case['per_alpha']}): "
          "worst error / bound " + ", ".join(f"{k} {v[0]:.3f}" for k, v in report.items()))
    REPORT["shapes"][case["id"]] = {k: v[0] for k, v in report.items()}
    for key, (ratio, where, passed) in report.items():
        assert passed, (key, ratio, where, describe(case, key, where), float(got[key][where]), float(ref[key][where]))
    # the documented domain: -inf value entries outside the two target entries leave their sample finite
    assert np.isfinite(got["head_sums"][0, 0]) and np.isfinite(got["grad_value"][K1 - 1, 0]).all()
    assert (got["grad_value"][K1 - 1, 0][np.isneginf(case["value"][K1 - 1, 0])] == 0).all()
    # step 0's reward row (NaN or log(one_hot)) is never read: zeros, bit for bit, and no reward term for K1 = 1
    assert same_bits(got["grad_reward"][0], np.zeros_like(got["grad_reward"][0]))
    if K1 == 1:
        assert same_bits(got["head_sums"][1], np.zeros(B, dtype=np.float32))
    if case["per_alpha"] == 0.0:
        assert same_bits(got["priorities"], np.ones((B, K1), dtype=np.float32))
    # the non-finite samples: NaN (zero targets on -inf logits) and +inf (a target on one), each inside its sample
    special = case["special"]
    if "nan" in special:
        assert np.isnan(got["sample_loss"][special["nan"]]) and np.isnan(got["head_sums"][2, special["nan"]])
    if "inf" in special:
        loss, weight = got["sample_loss"][special["inf"]], (1.0 if case["weight"] is None else case["weight"][special["inf"]])
        assert np.isposinf(got["head_sums"][2, special["inf"]]) and (np.isposinf(loss) if weight > 0 else np.isnan(loss))
    if special:
        twin = launch(native, make_case(*shape, index=index, nan_sample=False))
        others = np.setdiff1d(np.arange(B), list(special.values()))
        for key in OUTPUTS:
            axis = {"sample_loss": 0, "head_sums": 1, "priorities": 0}.get(key, 1)
            assert same_bits(np.take(got[key], others, axis=axis), np.take(twin[key], others, axis=axis)), \
                f"{key}: a non-finite sample changes another sample's bits"
        assert np.isfinite(twin["sample_loss"][list(special.values())]).all()


@pytest.mark.parametrize("s", sorted({s for _, _, s, _ in SHAPES}))
def test_the_two_hot_targets_are_the_float32_restatement_bit_for_bit(native, s):
    """Probe logits (0 at an entry j away from the target's two entries, -200 elsewhere: every other soft-max entry is
    exactly 0 in float32), no weight, value_loss_weight 1, gradient scale 1: the gradient row is -target at every i != j.
    -grad_value[k][b] and -grad_reward[1][b] equal two_hot32's rows bit for bit over all scalar cases -- no tolerance; a
    difference names an operation of two_hot that does not round as IEEE float32 does."""
    case, j = probe_case(s, seed=s)
    got = launch(native, case)
    rows = two_hot_rows(case["target_value"][:, 0], s)
    away = np.arange(2 * s + 1)[None, :] != j[:, None]
    kinds = case["kinds"]["target_value"]
    for what, grad in (("value, step 0", got["grad_value"][0]), ("value, step 1", got["grad_value"][1]),
                       ("reward, step 1", got["grad_reward"][1])):
        target = -grad + np.float32(0.0)                                      # (-0.0 + 0.0 = +0.0: zeros compare as bits)
        wrong = ((target.view(np.uint32) != rows.view(np.uint32)) & away).any(axis=1)
        assert not wrong.any(), (what, [(kinds[i], float(case["target_value"][i, 0])) for i in np.nonzero(wrong)[0][:8]])
    assert same_bits(got["grad_reward"][0], np.zeros_like(got["grad_reward"][0]))
    assert np.isfinite(got["sample_loss"]).all() and (got["sample_loss"] <= 2 * 200.0 * 1.5 + 2.0).all()
    print(f"\ns={s}: {len(rows)} scalar targets x 3 rows, two-hot targets bit-identical to two_hot32")


@pytest.mark.parametrize("s,A", [(1, 1), (10, 4), (64, 65), (300, 129)])
def test_a_lone_finite_logit_under_a_one_hot_target_costs_nothing(native, s, A):
    """Every operation is exact (x - max = 0, expf(0) = 1, S = 1, logf(1) = 0, a weight of 1): loss 0, gradient rows 0.
    The other entries hold the finite stand-in (expf gives exactly 0); a true -inf under a zero weight would be NaN."""
    F = 2 * s + 1
    lone = np.full((1, 3, F), STAND_IN, dtype=np.float32)
    lone[0, :, F - 1] = (2.5, -7.0, 3e38)
    policy = np.full((1, 3, A), STAND_IN, dtype=np.float32)
    policy[0, :, A - 1] = (-7.0, 0.0, 1e30)
    one_hot = np.zeros((3, 1, A), dtype=np.float32)
    one_hot[:, 0, A - 1] = 1.0
    case = dict(B=3, K1=1, support=s, A=A, value=lone, reward=lone.copy(), policy=policy,
                target_value=np.full((3, 1), 3e38, dtype=np.float32), target_reward=np.full((3, 1), 3e38, dtype=np.float32),
                target_policy=one_hot, gradient_scale=np.ones((3, 1), dtype=np.float32), weight=None,
                value_loss_weight=0.25, per_alpha=0.5)
    got = launch(native, case)
    for key in ("sample_loss", "head_sums", "grad_value", "grad_reward", "grad_policy"):
        assert (got[key] == 0).all(), (key, got[key])
    ref = unroll_loss64(case)
    assert all(passed for _, _, passed in compare(got, ref, unroll_loss_bounds(case, ref)).values())


@pytest.mark.parametrize("index,shape", [c for c in CASES if c[1][0] in (7, 128)], ids=lambda v: shape_id(*v) if isinstance(v, tuple) else None)
def test_permuting_the_samples_permutes_every_output(native, index, shape):
    case = make_case(*shape, index=index)
    perm = np.random.RandomState(index).permutation(case["B"])
    moved = dict(case)
    for key in ("value", "reward", "policy"):
        moved[key] = case[key][:, perm]
    for key in ("target_value", "target_reward", "target_policy", "gradient_scale"):
        moved[key] = case[key][perm]
    moved["weight"] = None if case["weight"] is None else case["weight"][perm]
    a, b = launch(native, case), launch(native, moved)
    for key in OUTPUTS:
        axis = {"sample_loss": 0, "head_sums": 1, "priorities": 0}.get(key, 1)
        assert same_bits(np.take(a[key], perm, axis=axis), b[key]), key


# ---- through the autograd wrapper -------------------------------------------------------------------------------------
def _wrapper_inputs(case, contiguous=True):
    """Tensors for trainer._UnrollLoss.apply; not contiguous: every logit stack and batch entry is a strided view (a
    transposed stack, every other column of a wider tensor)."""
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def strided(t):
        if contiguous:
            return t
        wide = torch.stack([t, torch.full_like(t, float("nan"))], dim=-1).reshape(t.shape[:-1] + (2 * t.shape[-1],))
        view = wide[..., ::2]
        assert not view.is_contiguous() or view.numel() <= 1
        return view

    def stack(a):                                        # [K1, B, n]
        t = dev(a)
        if contiguous:
            return t.requires_grad_()
        return strided(t.transpose(0, 1).contiguous().transpose(0, 1)).detach().requires_grad_()

    logits = [stack(case[k]) for k in ("value", "reward", "policy")]
    b = {"values": strided(dev(case["target_value"])), "rewards": strided(dev(case["target_reward"])),
         "policies": strided(dev(case["target_policy"])), "gradient_scales": strided(dev(case["gradient_scale"])),
         "weights": None if case["weight"] is None else strided(dev(case["weight"]))}
    return logits, b


@pytest.mark.parametrize("index", [SHAPES.index((11, 11, 10, 63)), SHAPES.index((7, 6, 32, 64)), SHAPES.index((128, 6, 10, 121))],
                         ids=lambda i: shape_id(*SHAPES[i]))
def test_wrapper_under_a_nonuniform_upstream_gradient(native, mods, index):
    """(sample_loss * c).sum().backward() with a different seeded c per sample, on a shape with B == K1 and on shapes with
    B != K1: the gradient that reaches the logits is c[b] times the float64 one, within c[b] times its bound plus the one
    rounding of backward's product.  (mean() hands every sample the same 1 / B: a wrong broadcast passes it.)  And the
    same call on non-contiguous views of every input gives bit-identical outputs."""
    trainer_mod, _ = mods
    case = make_case(*SHAPES[index], index=index)
    B = case["B"]
    c = (np.random.RandomState(index).random_sample(B) * 3.0 + 0.25).astype(np.float32)
    ref = unroll_loss64(case)
    bounds = unroll_loss_bounds(case, ref, group=64)
    results = []
    for contiguous in (True, False):
        logits, b = _wrapper_inputs(case, contiguous)
        sample_loss, head_sums, priorities = trainer_mod._UnrollLoss.apply(*logits, b, case["support"], case["value_loss_weight"],
                                                                          case["per_alpha"])
        (sample_loss * torch.from_numpy(c).cuda()).sum().backward()
        results.append({"sample_loss": sample_loss, "head_sums": head_sums, "priorities": priorities,
                        **{"grad_" + k: t.grad for k, t in zip(("value", "reward", "policy"), logits)}})
        results[-1] = {k: v.detach().cpu().numpy() for k, v in results[-1].items()}
    got, strided = results
    for key in OUTPUTS:
        assert same_bits(got[key], strided[key]), f"{key}: non-contiguous inputs change the bits"
    c64 = c.astype(np.float64)
    want, allowed = dict(ref), dict(bounds)
    for key in ("grad_value", "grad_reward", "grad_policy"):
        want[key] = ref[key] * c64[None, :, None]
        with np.errstate(invalid="ignore"):
            allowed[key] = c64[None, :, None] * bounds[key] + F32_UNIT * (np.abs(want[key]) + c64[None, :, None] * bounds[key])
    report = compare(got, want, allowed)
    print(f"\n{case['id']}: wrapper, non-uniform upstream gradient, worst error / bound " +
          ", ".join(f"{k} {v[0]:.3f}" for k, v in report.items()))
    REPORT["shapes"][case["id"] + " (wrapper, upstream c[b])"] = {k: v[0] for k, v in report.items()}
    for key, (ratio, where, passed) in report.items():
        assert passed, (key, ratio, where, describe(case, key, where))


# ---- one whole training step ------------------------------------------------------------------------------------------
def _scalar_to_support64(x, support_size):
    """models.scalar_to_support evaluated in the dtype of x (the function itself scatters into a float32 tensor)."""
    x = torch.sign(x) * (torch.sqrt(torch.abs(x) + 1) - 1) + 0.001 * x
    x = torch.clamp(x, -support_size, support_size)
    low = x.floor()
    frac = x - low
    out = torch.zeros(x.shape[0], x.shape[1], 2 * support_size + 1, dtype=x.dtype)
    out.scatter_(2, (low + support_size).long().unsqueeze(-1), (1 - frac).unsqueeze(-1))
    upper = low + support_size + 1
    overflow = 2 * support_size < upper
    frac = frac.masked_fill(overflow, 0.0)
    upper = upper.masked_fill(overflow, 0.0)
    out.scatter_(2, upper.long().unsqueeze(-1), frac.unsqueeze(-1))
    return out


@pytest.mark.parametrize("game", ["cartpole", "tictactoe"])
def test_parameter_gradients_of_one_training_step_vs_float64(native, mods, game):
    """One batch through Trainer.update_weights on a fully connected (CartPole) and a residual (TicTacToe) network, with
    native_loss = True (the HIP launch) and False (the torch expression in float32 on the GPU); the parameter gradients of
    both against the same model in float64 on the CPU with the torch expression.  Both float32 paths share the network's
    forward and backward, so the loss launch may reorder sums but has no room for more: per parameter tensor the native
    path's largest error is at most 4 times the float32 library path's own (with a floor of 4 u max|g64|, u = 2^-24, so
    that a tensor the library path happens to get almost exactly does not decide the test).  The factor is a margin over
    the library path's measured error, not the kernel's; the ratios go into the report."""
    trainer_mod, models = mods
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    torch.manual_seed(3)
    model = models.MuZeroNetwork(config)
    ckpt = {"weights": copy.deepcopy(model.get_weights()), "training_step": 0, "optimizer_state": None}
    B, K1, A = 32, config.num_unroll_steps + 1, len(config.action_space)
    g = torch.Generator().manual_seed(17)
    batch = (torch.rand((B,) + tuple(config.observation_shape), generator=g), torch.randint(0, A, (B, K1), generator=g),
             torch.randn(B, K1, generator=g) * 10, torch.randn(B, K1, generator=g),
             torch.softmax(torch.randn(B, K1, A, generator=g), dim=2), torch.rand(B, generator=g) + 0.5,
             torch.randint(1, K1 + 1, (B, K1), generator=g).float())
    gradients = {}
    for native_loss in (True, False):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda")
        trainer.native_loss = native_loss
        trainer.update_weights(tuple(t.cuda() for t in batch))
        gradients[native_loss] = {k: p.grad.detach().double().cpu() for k, p in trainer.model.named_parameters() if p.grad is not None}
    model64 = models.MuZeroNetwork(config)
    model64.set_weights(copy.deepcopy(ckpt["weights"]))
    model64 = model64.double()
    model64._zero_reward_cache = None
    model64.refresh_inference_constants()
    model64.train()
    observations, actions, values, rewards, policies, weights, scales = batch
    steps = trainer_mod.Trainer._unroll(types.SimpleNamespace(model=model64), observations.double(), actions.long().unsqueeze(-1))
    b64 = {"values": values.double(), "rewards": rewards.double(), "policies": policies.double(),
           "gradient_scales": scales.double(), "weights": weights.double() if config.PER else None}
    helpers = types.SimpleNamespace(scalar_to_support=_scalar_to_support64, support_to_scalar=models.support_to_scalar)
    loss, _, _ = torch_reference(trainer_mod, helpers, [s[0] for s in steps], [s[1] for s in steps], [s[2] for s in steps],
                                 b64, config.support_size, config.value_loss_weight, config.PER_alpha)
    loss.mean().backward()
    exact = {k: p.grad.detach() for k, p in model64.named_parameters() if p.grad is not None}
    assert set(exact) == set(gradients[True]) == set(gradients[False]) and len(exact) >= 8
    ratios = {}
    for name, g64 in exact.items():
        scale = float(g64.abs().max())
        native_error = float((gradients[True][name] - g64).abs().max())
        library_error = float((gradients[False][name] - g64).abs().max())
        allowed = 4.0 * max(library_error, 4.0 * F32_UNIT * scale)
        ratios[name] = native_error / allowed if allowed > 0 else (0.0 if native_error == 0 else float("inf"))
        REPORT["training_step"].setdefault(game, {})[name] = {"native": native_error, "library": library_error,
                                                              "max_abs_gradient": scale, "ratio": ratios[name]}
    worst = max(ratios, key=ratios.get)
    print(f"\n{game}: {len(ratios)} parameter tensors, worst native error / allowed {ratios[worst]:.3f} ({worst})")
    assert ratios[worst] <= 1.0, (worst, REPORT["training_step"][game][worst])
