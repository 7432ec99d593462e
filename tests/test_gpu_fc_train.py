"""The training step of fully-connected networks as HIP launches (include/mztrain.h mztrain_fc_*, csrc/fc_train.hip,
csrc/fc_backward.h; Trainer(fc_step=True)) on the MI355X.

Forward: the logits of all K1 positions are the bits of the search's own lock-step inference.  Gradients, losses, head sums
and priorities: against the float64 yardstick (tests/fc_train_reference.py) by the project's rule for a training step,
native error <= 4 max(library error, 4 * 2^-24 max|x64|), the library being today's Trainer (torch forward and backward in
float32 on the GPU) on the same batch in the same test; every ratio goes into measure_out/fc_train_report.json.  Exact
properties: same bits from run to run, every gradient entry written, guard bands, exact zeros for K1 = 1.  Then whole
steps through Trainer(fc_step=True)."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import fc_train_reference as ref
from unroll_loss_reference import torch_reference, two_hot_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 256
VALUE_LOSS_WEIGHT, PER_ALPHA = 0.25, 0.5
REPORT = {"gradients": {}, "outputs": {}, "whole_steps": {}}
CASES = [(name, B, K1) for name, sh in ref.SHAPES.items() for B, K1 in sh["cases"]]
FURTHER = {"per-weights": dict(weights="per"), "no-weights": dict(weights="none"), "scales-1": dict(scales="ones"),
           "actions-outside": dict(bad_actions=True)}


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fc_train_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def full_config(sh):
    """A whole MuZeroConfig (CartPole's) carrying the shape's network."""
    cfg = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    small = ref.config_for(sh)
    for key, value in vars(small).items():
        setattr(cfg, key, value)
    cfg.value_loss_weight, cfg.PER_alpha = VALUE_LOSS_WEIGHT, PER_ALPHA
    return cfg


def fc_desc(native, sh):
    desc = native.MzFcDesc()
    desc.observation_floats, desc.encoding_size = sh["obs"], sh["enc"]
    for i, widths in enumerate(sh["hidden"]):
        desc.n_hidden[i] = len(widths)
        for k, width in enumerate(widths):
            desc.hidden[i][k] = width
    return desc


def guarded(n, dtype=torch.float32, fill=float("nan")):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_untouched(buf):
    host = buf.cpu().numpy()
    return np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all()


class _DeviceBytes:
    """`count` bytes of device memory at a raw pointer, as the array interface torch reads."""

    def __init__(self, pointer, count):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "|u1", "data": (pointer, False), "version": 2}


def device_bytes(pointer, count):
    """`count` bytes of device memory at a raw pointer (the handle's workspace is not a torch tensor): copied by torch."""
    torch.cuda.synchronize()
    return torch.as_tensor(_DeviceBytes(pointer, count), device="cuda").cpu().numpy().copy()


class Step:
    """One handle on guarded weight / gradient buffers."""

    def __init__(self, native, sh, state, max_batch, max_steps):
        self.native, self.lib, self.sh = native, native.load(), sh
        flat = ref.flatten(state)
        self.n = flat.size
        self.w_buf, self.weights = guarded(self.n)
        self.weights.copy_(torch.from_numpy(flat))
        self.g_buf, self.grads = guarded(self.n)
        self.max = (max_batch, max_steps)
        self.handle = ctypes.c_void_p()
        rc = self.lib.mztrain_fc_create(ctypes.byref(fc_desc(native, sh)), sh["A"], sh["support"], self.weights.data_ptr(), self.n,
                                        self.grads.data_ptr(), max_batch, max_steps, torch.cuda.current_device(),
                                        ctypes.byref(self.handle))
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))

    def close(self):
        torch.cuda.synchronize()
        self.lib.mztrain_fc_destroy(self.handle)

    def run(self, batch, expect=0):
        B, K1 = batch["actions"].shape
        F, A = 2 * self.sh["support"] + 1, self.sh["A"]
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items() if v is not None}
        outs = {"sample_loss": guarded(B), "head_sums": guarded(3 * B), "priorities": guarded(B * K1)}
        args = self.native.MzTrainFcArgs(
            observations=dev["observations"].data_ptr(), actions=dev["actions"].data_ptr(),
            target_value=dev["values"].data_ptr(), target_reward=dev["rewards"].data_ptr(),
            target_policy=dev["policies"].data_ptr(), gradient_scale=dev["gradient_scales"].data_ptr(),
            weight=dev["weights"].data_ptr() if "weights" in dev else None, batch=B, steps=K1,
            value_loss_weight=VALUE_LOSS_WEIGHT, per_alpha=PER_ALPHA,
            **{k: v[1].data_ptr() for k, v in outs.items()})
        torch.cuda.synchronize()
        rc = self.lib.mztrain_fc_step(self.handle, ctypes.byref(args), torch.cuda.current_stream().cuda_stream)
        if expect != 0:
            return rc
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))
        torch.cuda.synchronize()
        for name, (buf, _) in outs.items():
            assert guards_untouched(buf), f"{name}: a guard band was written"
        assert guards_untouched(self.g_buf), "the gradient buffer's guard band was written"
        assert guards_untouched(self.w_buf), "the weight buffer's guard band was written"
        pointers = [ctypes.c_void_p() for _ in range(3)]
        assert self.lib.mztrain_fc_logits(self.handle, *(ctypes.byref(p) for p in pointers)) == 0
        sizes = (K1 * B * F, K1 * B * F, K1 * B * A)
        logits = [device_bytes(p.value, 4 * n).view(np.float32).reshape(K1, B, -1) for p, n in zip(pointers, sizes)]
        return {"grads": self.grads.cpu().numpy().copy(), "sample_loss": outs["sample_loss"][1].cpu().numpy(),
                "head_sums": outs["head_sums"][1].cpu().numpy().reshape(3, B),
                "priorities": outs["priorities"][1].cpu().numpy().reshape(B, K1), "value": logits[0], "reward": logits[1],
                "policy": logits[2], "pointers": [p.value for p in pointers]}


def build(mods, name, B, K1, **how):
    sh = ref.SHAPES[name]
    model = ref.make_model(mods[1], sh, ref.SEEDS[name])
    state = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    return sh, model, state, ref.make_batch(sh, B, K1, seed=B * 100 + K1, **how)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                          np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def split(sh, flat):
    """A flat gradient buffer as {parameter name: array}."""
    table, widths, _ = ref.flat_offsets(sh)
    out = {}
    for m, mlp in enumerate(ref.MLPS):
        for l, (w_off, b_off) in enumerate(table[m]):
            fan_in, fan_out = widths[m][l], widths[m][l + 1]
            out[f"{mlp}.module.{2 * l}.weight"] = flat[w_off:w_off + fan_in * fan_out].reshape(fan_out, fan_in)
            out[f"{mlp}.module.{2 * l}.bias"] = flat[b_off:b_off + fan_out]
    return out


def batch_tensors(batch, device="cuda"):
    return {"observations": torch.from_numpy(batch["observations"]).to(device),
            "actions": torch.from_numpy(batch["actions"]).to(device).unsqueeze(-1),
            "values": torch.from_numpy(batch["values"]).to(device), "rewards": torch.from_numpy(batch["rewards"]).to(device),
            "policies": torch.from_numpy(batch["policies"]).to(device),
            "weights": None if batch["weights"] is None else torch.from_numpy(batch["weights"]).to(device),
            "gradient_scales": torch.from_numpy(batch["gradient_scales"]).to(device)}


def library_step(mods, sh, model, batch):
    """Today's Trainer on the same batch: torch forward and backward in float32 on the GPU, the loss launch in between."""
    trainer_mod, _ = mods
    ckpt = {"weights": copy.deepcopy(model.state_dict()), "training_step": 0, "optimizer_state": None}
    trainer = trainer_mod.Trainer(ckpt, full_config(sh), device="cuda")
    sample_loss, head_sums, priorities = trainer._loss_native(batch_tensors(batch))
    sample_loss.mean().backward()
    grads = {k: (p.grad.detach().double().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape)))
             for k, p in trainer.model.named_parameters()}
    return {"grads": grads, "sample_loss": sample_loss.detach().double().cpu().numpy(),
            "head_sums": head_sums.double().cpu().numpy(), "priorities": priorities.double().cpu().numpy()}


def ratio(native_value, library_value, exact):
    """native error / (4 max(library error, 4 u max|exact|)); 0 / 0 = 0."""
    scale = float(np.abs(exact).max())
    native_error = float(np.abs(np.asarray(native_value, dtype=np.float64) - exact).max())
    library_error = float(np.abs(np.asarray(library_value, dtype=np.float64) - exact).max())
    allowed = 4.0 * max(library_error, 4.0 * U * scale)
    value = native_error / allowed if allowed > 0 else (0.0 if native_error == 0 else float("inf"))
    return value, {"native": native_error, "library": library_error, "max_abs": scale, "ratio": value}


def check_against_float64(mods, native, name, B, K1, label, **how):
    sh, model, state, batch = build(mods, name, B, K1, **how)
    exact = ref.unroll64(state, batch, sh, VALUE_LOSS_WEIGHT, PER_ALPHA)
    step = Step(native, sh, state, B, K1)
    got = step.run(batch)
    step.close()
    library = library_step(mods, sh, model, batch)
    assert np.isfinite(got["grads"]).all(), "an entry of the gradient buffer was left at its NaN"
    mine = split(sh, got["grads"])
    worst = {}
    for key, g64 in exact["grads"].items():
        worst[key], entry = ratio(mine[key], library["grads"][key], g64)
        REPORT["gradients"].setdefault(label, {})[key] = entry
        if K1 == 1 and key.startswith(("dynamics_encoded_state_network", "dynamics_reward_network")):
            assert same_bits(mine[key], np.zeros_like(mine[key])), key
    for key in ("sample_loss", "head_sums", "priorities"):
        worst[key], entry = ratio(got[key], library[key], exact["loss"][key])
        REPORT["outputs"].setdefault(label, {})[key] = entry
    top = max(worst, key=worst.get)
    print(f"\n{label}: worst native error / allowed {worst[top]:.3f} ({top})")
    assert worst[top] <= 1.0, (top, worst[top])
    return got, exact


@pytest.mark.parametrize("name,B,K1", CASES, ids=[f"{n}-B{b}-K{k}" for n, b, k in CASES])
def test_gradients_and_losses_vs_float64(mods, native, name, B, K1):
    how = dict(weights="per") if (B + K1) % 2 else {}
    check_against_float64(mods, native, name, B, K1, f"{name}-B{B}-K{K1}", **how)


@pytest.mark.parametrize("label", list(FURTHER))
def test_further_cases_vs_float64(mods, native, label):
    got, exact = check_against_float64(mods, native, "S1", 5, 3, "S1-" + label, **FURTHER[label])


@pytest.mark.parametrize("name,B,K1", CASES, ids=[f"{n}-B{b}-K{k}" for n, b, k in CASES])
def test_forward_logits_are_the_search_inference_bit_for_bit(mods, native, name, B, K1):
    eng = importlib.import_module("muzero-hypermodel_amd.engine")
    sh, model, state, batch = build(mods, name, B, K1)
    step = Step(native, sh, state, B, K1)
    got = step.run(batch)
    step.close()
    cfg = full_config(sh)
    cfg.num_simulations = 2
    # (121 actions need the engine's own choice of lanes per tree; a neuron's sum does not depend on it)
    engine = eng.BatchedMCTS(cfg, B, group_width=16 if sh["A"] <= 16 else 0, seeds=list(range(B)))
    engine.configure_fused_fc(model.to("cuda").eval())
    # fc_initial<G> / fc_recurrent<G>, the generic kernels' device functions (the narrow kernels keep a row's activations
    # in registers and add a neuron's products in rotation order: other roundings, CartPole's shape would take them)
    engine.set_fused_options(variant="generic")
    obs = torch.from_numpy(batch["observations"]).cuda()
    v, r, p, hidden = engine.fc_initial_inference(obs)
    for k in range(K1):
        if k > 0:
            v, r, p, hidden = engine.fc_recurrent_inference(hidden, torch.from_numpy(batch["actions"][:, k]).cuda())
            assert same_bits(got["reward"][k], r.cpu().numpy()), k
        assert same_bits(got["value"][k], v.cpu().numpy()), k
        assert same_bits(got["policy"][k], p.cpu().numpy()), k
        hidden = hidden.clone()
    engine.close()


def test_a_sample_has_the_same_bits_in_a_batch_of_1_and_of_33(mods, native):
    sh, model, state, batch = build(mods, "S1", 33, 11, weights="per")
    step = Step(native, sh, state, 33, 11)
    whole = step.run(batch)
    for b in (0, 16, 32):
        single = {k: (None if v is None else v[b:b + 1].copy()) for k, v in batch.items()}
        alone = step.run(single)
        for key in ("value", "policy"):
            assert same_bits(alone[key][:, 0], whole[key][:, b]), (key, b)
        assert same_bits(alone["reward"][1:, 0], whole["reward"][1:, b]), b
        assert same_bits(alone["priorities"][0], whole["priorities"][b]) and same_bits(alone["sample_loss"][0], whole["sample_loss"][b])
    step.close()


def test_exact_properties(mods, native):
    """Two calls give the same bits; a gradient buffer pre-filled with NaN (and with other numbers) comes back the same,
    fully written; the workspace's own guard bands and the gaps behind the logits stay as create left them; a batch
    above the created maxima is refused."""
    sh, model, state, batch = build(mods, "S1", 33, 11, weights="per")
    step = Step(native, sh, state, 33, 11)
    first = step.run(batch)
    step.grads.fill_(12345.0)
    second = step.run(batch)
    for key in ("grads", "sample_loss", "head_sums", "priorities", "value", "policy"):
        assert same_bits(first[key], second[key]), key
    assert np.isfinite(second["grads"]).all() and not (second["grads"] == 12345.0).any()
    # the workspace: [256 B guard][value logits][reward logits][policy logits]...[256 B guard], segments on 256 B
    # boundaries, everything 0xff after create
    total = step.lib.mztrain_fc_workspace_bytes(step.handle)
    raw = device_bytes(first["pointers"][0] - 256, total)
    assert (raw[:256] == 0xff).all() and (raw[-256:] == 0xff).all(), "a guard band of the workspace was written"
    F, A, P = 21, 2, 33 * 11
    at = 256
    for pointer, floats in zip(first["pointers"], (P * F, P * F, P * A)):
        assert pointer - first["pointers"][0] == at - 256
        end = at + 4 * floats
        padded = (end + 255) // 256 * 256
        assert (raw[end:padded] == 0xff).all(), "the gap behind a logits array was written"
        at = padded
    over = ref.make_batch(sh, 34, 11, seed=1)
    assert step.run(over, expect=-1) == native.ERR_INVALID
    assert b"above the maxima" in step.lib.mzmcts_last_error(None)
    over = ref.make_batch(sh, 4, 12, seed=1)
    assert step.run(over, expect=-1) == native.ERR_INVALID
    step.close()


# ---- whole steps through the Trainer -------------------------------------------------------------------------------------
def cartpole_setup(mods, seed=1, **over):
    trainer_mod, models = mods
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    for key, value in over.items():
        setattr(config, key, value)
    torch.manual_seed(seed)
    model = models.MuZeroNetwork(config)
    return config, {"weights": model.get_weights(), "training_step": 0, "optimizer_state": None}


def cuda_batches(config, B, count, seed):
    K1, A = config.num_unroll_steps + 1, len(config.action_space)
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.rand((B,) + tuple(config.observation_shape), generator=g, device="cuda"),
             torch.randint(0, A, (B, K1), generator=g, device="cuda"),
             torch.randn(B, K1, generator=g, device="cuda") * 10, torch.randn(B, K1, generator=g, device="cuda"),
             torch.softmax(torch.randn(B, K1, A, generator=g, device="cuda"), dim=2),
             torch.rand(B, generator=g, device="cuda") + 0.5,
             torch.randint(1, K1 + 1, (B, K1), generator=g, device="cuda").float()) for _ in range(count)]


def test_fc_step_refuses_what_it_does_not_cover(mods):
    trainer_mod, models = mods
    config, ckpt = cartpole_setup(mods)
    with pytest.raises(NotImplementedError, match="must be on the GPU"):
        trainer_mod.Trainer(ckpt, config, device="cpu", fc_step=True)
    resnet = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    with pytest.raises(NotImplementedError, match="fully-connected"):
        trainer_mod.Trainer({"weights": models.MuZeroNetwork(resnet).get_weights(), "training_step": 0,
                             "optimizer_state": None}, resnet, device="cuda", fc_step=True)
    wide, wide_ckpt = cartpole_setup(mods, fc_dynamics_layers=[256, 256, 256], fc_value_layers=[256, 256, 256],
                                     fc_reward_layers=[256, 256, 256])
    with pytest.raises(NotImplementedError, match="160 KB of LDS"):
        trainer_mod.Trainer(wide_ckpt, wide, device="cuda", fc_step=True)


def test_sgd_update_is_linear_in_the_gradient_and_three_steps_vs_float64(mods, native):
    trainer_mod, models = mods
    config, ckpt = cartpole_setup(mods, optimizer="SGD", momentum=0.0, PER=True, batch_size=32)
    batches = cuda_batches(config, 32, 3, seed=7)
    runs = {}
    for fc_step in (True, False):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", fc_step=fc_step)
        before = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
        for index, bt in enumerate(batches):
            trainer.update_lr()
            trainer.update_weights(bt)
            if fc_step and index == 0:        # w1 = w0 - lr (g + wd w0): one rounding per operation
                lr, wd = trainer.optimizer.param_groups[0]["lr"], config.weight_decay
                for key, p in trainer.model.named_parameters():
                    w0, g = before[key].double(), p.grad.double()
                    expected = w0 - lr * (g + wd * w0)
                    slack = 4 * U * (w0.abs() + lr * (g.abs() + wd * w0.abs()))
                    assert bool(((p.detach().double() - expected).abs() <= slack).all()), key
        runs[fc_step] = {k: (v.detach().double().cpu() - before[k].double().cpu()) for k, v in trainer.model.state_dict().items()}
    # the same three steps in float64 on the CPU
    model64 = models.MuZeroNetwork(config)
    model64.load_state_dict(copy.deepcopy(ckpt["weights"]))
    model64 = model64.double()
    model64._zero_reward_cache = None
    start = {k: v.detach().clone() for k, v in model64.state_dict().items()}
    optimizer = torch.optim.SGD(model64.parameters(), lr=config.lr_init, momentum=0.0, weight_decay=config.weight_decay)

    def rows(x, support):
        return torch.from_numpy(two_hot_rows(x.detach().to(torch.float32).numpy(), support)).double()

    helpers = types.SimpleNamespace(scalar_to_support=rows, support_to_scalar=models.support_to_scalar)
    for index, bt in enumerate(batches):
        for group in optimizer.param_groups:
            group["lr"] = config.lr_init * config.lr_decay_rate ** (index / config.lr_decay_steps)
        obs, act, val, rew, pol, weight, scale = (t.cpu() for t in bt)
        steps = trainer_mod.Trainer._unroll(types.SimpleNamespace(model=model64), obs.double(), act.long().unsqueeze(-1))
        b64 = {"values": val.double(), "rewards": rew.double(), "policies": pol.double(), "gradient_scales": scale.double(),
               "weights": weight.double()}
        loss, _, _ = torch_reference(trainer_mod, helpers, [s[0] for s in steps], [s[1] for s in steps], [s[2] for s in steps],
                                     b64, config.support_size, config.value_loss_weight, config.PER_alpha)
        optimizer.zero_grad()
        loss.mean().backward()
        optimizer.step()
    worst = {}
    for key, now in model64.state_dict().items():
        exact = (now.detach() - start[key]).numpy()
        worst[key], REPORT["whole_steps"].setdefault("sgd_three_steps", {})[key] = ratio(runs[True][key].numpy(),
                                                                                       runs[False][key].numpy(), exact)
    top = max(worst, key=worst.get)
    print(f"\nthree SGD steps: worst native error / allowed {worst[top]:.3f} ({top})")
    assert worst[top] <= 1.0, (top, worst[top])


def test_graphed_fc_step_equals_eager_fc_step(mods):
    """Adam, four steps under a decaying learning rate: 1e-5, the figure of test_graphed_step_equals_eager_step.  Then a
    replayed graph sees weights published into the flat buffer in between."""
    trainer_mod, models = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32)
    batches = cuda_batches(config, 32, 5, seed=5)
    runs = []
    for graph in (False, True):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, fc_step=True)
        out = []
        for bt in batches[:4]:
            trainer.update_lr()
            out.append(trainer.update_weights(bt))
        runs.append((out, {k: v.clone() for k, v in trainer.model.state_dict().items()}, trainer))
    (eager, w_eager, t_eager), (graphed, w_graphed, t_graphed) = runs
    worst_w = max(float((w_eager[k] - w_graphed[k]).abs().max()) for k in w_eager)
    worst_p = max(float(np.abs(a[0] - b[0]).max()) for a, b in zip(eager, graphed))
    worst_l = max(abs(x - y) / abs(x) for a, b in zip(eager, graphed) for x, y in zip(a[1:], b[1:]))
    print(f"\ngraphed vs eager fc_step: weights {worst_w:.2e}, priorities {worst_p:.2e}, losses {worst_l:.2e} (rel.)")
    assert worst_w <= 1e-5 and worst_l <= 1e-5 and worst_p <= 2e-3
    assert t_graphed._graph is not None and t_graphed.training_step == 4
    # publish other weights into the flat buffers of both: the next (replayed / eager) step starts from them
    torch.manual_seed(99)
    other = models.MuZeroNetwork(config).get_weights()
    losses = []
    for trainer in (t_eager, t_graphed):
        trainer.flat_weights.load_state_dict(other)
        trainer.update_lr()
        losses.append(trainer.update_weights(batches[4])[1])
    fresh = trainer_mod.Trainer({"weights": other, "training_step": 0, "optimizer_state": None}, config, device="cuda",
                                fc_step=True)
    want = fresh.update_weights(batches[4])[1]          # (the loss is computed before the optimizer moves anything)
    assert abs(losses[0] - want) <= 1e-6 * abs(want) and abs(losses[1] - want) <= 1e-6 * abs(want)
    assert abs(losses[1] - eager[3][1]) > 1e-3 * abs(want), "the published weights made no difference"


def test_fixture_g14_through_fc_step(mods, pkg, native):
    """The reference's recorded CartPole steps (two Adam steps) with the tolerances of the existing GPU test: losses 1e-4,
    priorities 2e-3, at least 97 % of the weights within 1e-4; the library path's share from the same run beside it."""
    from parity_helpers import load_golden
    from test_trainer_cpu import batch_of
    trainer_mod, _ = mods
    fx = load_golden("g14_trainer_cartpole")
    w = load_golden("cartpole_weights")
    shares = {}
    for fc_step in (False, True):
        config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
        config.batch_size = 32
        weights = {k: torch.from_numpy(w[k]) for k in w.files}
        trainer = trainer_mod.Trainer({"weights": weights, "training_step": 0, "optimizer_state": None}, config, device="cuda",
                                      fc_step=fc_step)
        within = total = 0
        for step in range(2):
            trainer.update_lr()
            assert trainer.optimizer.param_groups[0]["lr"] == float(fx[f"lr{step}"])
            batch = tuple(b.to("cuda") if torch.is_tensor(b) else b for b in batch_of(fx, True))
            priorities, *losses = trainer.update_weights(batch)
            if fc_step:
                np.testing.assert_allclose(losses, fx[f"losses{step}"], rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(priorities, fx[f"priorities{step}"], rtol=2e-3, atol=2e-3)
            for k, t in trainer.model.get_weights().items():
                d = np.abs(t.numpy() - fx[f"w{step}_{k}"])
                within, total = within + int((d <= 1e-4).sum()), total + d.size
        shares[fc_step] = within / total
    REPORT["whole_steps"]["g14_share_of_weights_within_1e-4"] = {"fc_step": shares[True], "library": shares[False]}
    print(f"\nG14: weights within 1e-4: fc_step {shares[True]:.4f}, library {shares[False]:.4f}")
    assert shares[True] >= 0.97


@pytest.mark.parametrize("first", [False, True], ids=["library-then-fc", "fc-then-library"])
def test_checkpoints_cross_between_the_two_paths(mods, first):
    trainer_mod, _ = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32)
    batches = cuda_batches(config, 32, 5, seed=11)
    writer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", fc_step=first)
    for bt in batches[:3]:
        writer.update_lr()
        writer.update_weights(bt)
    saved = {"weights": writer.model.get_weights(), "training_step": writer.training_step,
             "optimizer_state": writer.optimizer_state()}
    out = {}
    for fc_step in (False, True):
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", fc_step=fc_step)
        assert trainer.training_step == 3
        losses = []
        for bt in batches[3:]:
            trainer.update_lr()
            losses.append(trainer.update_weights(bt)[1])
        assert trainer.training_step == 5 and trainer._lr_host == config.lr_init * config.lr_decay_rate ** (4 / 4)
        out[fc_step] = (losses, {k: v.detach().clone() for k, v in trainer.model.state_dict().items()})
    # the weights and Adam's moments came through the checkpoint: the first loss after it is computed from the same
    # numbers by either path (1e-4, G14's figure for losses), and the two resumed trainers move alike -- at least 97 % of
    # the weights within 1e-4 after two more steps, G14's figure for two paths that round differently
    assert abs(out[True][0][0] - out[False][0][0]) <= 1e-4 * abs(out[False][0][0])
    close = sum(int(((out[True][1][k] - out[False][1][k]).abs() <= 1e-4).sum()) for k in out[True][1])
    assert close >= 0.97 * sum(v.numel() for v in out[True][1].values())


@pytest.mark.parametrize("graph", [False, True])
def test_train_steps_on_a_device_sampling_buffer(mods, graph):
    from parity_helpers import history_of, load_golden
    trainer_mod, models = mods
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    config, ckpt = cartpole_setup(mods, batch_size=32, replay_buffer_size=40, lr_decay_steps=4)
    fx = load_golden("g12_replay_cartpole")
    rb = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config, device_sampling=True)
    for g in range(len(fx["lengths"])):
        rb.save_game(history_of(sp, fx, g))
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, fc_step=True)
    before = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
    stored = {g: rb.download_priorities(g)[0].copy() for g in rb.buffer}
    losses = trainer.train_steps(rb, 4)
    assert trainer.training_step == 4 and len(losses) == 4 and all(np.isfinite(losses))
    assert all(bool((v != before[k]).any()) for k, v in trainer.model.state_dict().items())
    assert any(not np.array_equal(rb.download_priorities(g)[0], stored[g]) for g in rb.buffer), "no priority was updated"
    one_more = trainer.train_steps(rb, 1)
    assert trainer.training_step == 5 and len(one_more) == 4
    rb.close()
