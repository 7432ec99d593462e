"""The optimizer's step on the flat buffers as HIP launches (include/mztrain.h mztrain_opt_step, csrc/fc_optimizer.hip;
Trainer(fc_step=True, fc_optimizer=True)) on the MI355X.

The kernel against mztrain_opt_reference on the host, bit for bit, at every size where it takes another path (quads and the
scalar tail, one and many workgroups, pointers that are not 16-byte aligned), between NaN guard bands.  Then whole steps
through the Trainer: replayed on the host from the gradients read back, graphed against eager, checkpoints across the three
ways (library, fc_step, fc_step + fc_optimizer), fixture G14, train_steps, and a TwentyOne-shaped SGD configuration under
capture held to float64 by the training-step rule.  The worst ratios go into measure_out/fc_optimizer_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import fc_optimizer_reference as ref
from test_gpu_fc_train import cartpole_setup, cuda_batches, ratio, same_bits
from unroll_loss_reference import torch_reference, two_hot_rows

pytestmark = pytest.mark.gpu

GUARD = 256
REPORT = {"whole_steps": {}}
WAYS = {"library": {}, "fc_step": dict(fc_step=True), "fc_optimizer": dict(fc_step=True, fc_optimizer=True)}
NEW = WAYS["fc_optimizer"]
KERNEL_CASES = [(label, decay, offset) for label in ref.KINDS for decay in ref.DECAYS for offset in (0, 1)]


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fc_optimizer_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


class Guarded:
    """`n` floats between two NaN bands, `offset` floats past a 16-byte boundary."""

    def __init__(self, n, offset, values=None):
        self.buf = torch.full((n + 2 * GUARD + offset,), float("nan"), dtype=torch.float32, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.view = self.buf[self.lo:self.hi]
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        assert (self.view.data_ptr() % 16 == 0) == (offset == 0)

    def bands_untouched(self):
        host = self.buf.cpu().numpy()
        return bool(np.isnan(host[:self.lo]).all() and np.isnan(host[self.hi:]).all())

    def all_untouched(self):
        return bool(np.isnan(self.buf.cpu().numpy()).all())


# ---- the kernel against the host entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("label,decay,offset", KERNEL_CASES,
                         ids=[f"{l}-wd{d:g}-{'aligned' if o == 0 else 'offset-by-a-float'}" for l, d, o in KERNEL_CASES])
def test_kernel_equals_the_host_entry_bit_for_bit(native, label, decay, offset):
    lib = native.load()
    how = ref.KINDS[label]
    kind, momentum = how["kind"], how.get("momentum", 0.0)
    uses = {"moment1": kind == "Adam" or momentum != 0.0, "moment2": kind == "Adam"}
    lrs = ref.learning_rates()
    stream = torch.cuda.current_stream().cuda_stream
    for n in ref.SIZES:
        weights, grads = ref.make_case(n)
        want = ref.run_host_entry(native, kind, weights, grads, lrs, weight_decay=decay, momentum=momentum)
        w = Guarded(n, offset, weights)
        # a moment the kind does not use is handed over all the same, full of NaN: it must come back untouched
        moments = {key: Guarded(n, offset, np.zeros(n) if used else None) for key, used in uses.items()}
        g_dev = [Guarded(n, offset, g) for g in grads]
        lr = torch.zeros(1, dtype=torch.float64, device="cuda")
        done = torch.zeros(1, dtype=torch.int64, device="cuda")
        for g, rate in zip(g_dev, lrs):
            lr.fill_(rate)
            args = ref.opt_args(native, kind, n, w.view.data_ptr(), g.view.data_ptr(), moments["moment1"].view.data_ptr(),
                                moments["moment2"].view.data_ptr(), lr.data_ptr(), done.data_ptr(), weight_decay=decay,
                                momentum=momentum)
            rc = lib.mztrain_opt_step(ctypes.byref(args), stream)
            assert rc == 0, (rc, lib.mzmcts_last_error(None))
        torch.cuda.synchronize()
        assert int(done.item()) == ref.STEPS == want["steps_done"], n
        assert same_bits(w.view.cpu().numpy(), want["weights"]), (n, "weights")
        assert w.bands_untouched(), (n, "a guard band of the weights was written")
        for key, used in uses.items():
            if used:
                assert same_bits(moments[key].view.cpu().numpy(), want[key]), (n, key)
                assert moments[key].bands_untouched(), (n, key, "guard band")
            else:
                assert moments[key].all_untouched(), (n, key, "a moment the kind does not use was written")
        for g, host in zip(g_dev, grads):
            assert same_bits(g.view.cpu().numpy(), host) and g.bands_untouched(), (n, "the gradient was written")


# ---- whole steps through the Trainer ---------------------------------------------------------------------------------------
def flat_state(trainer):
    opt = trainer.optimizer
    return {"weights": trainer.flat_weights.flat.cpu().numpy().copy(), "moment1": opt.moment1.cpu().numpy().copy(),
            "moment2": opt.moment2.cpu().numpy().copy(), "steps_done": int(opt.steps_done.item())}


def test_fc_optimizer_needs_fc_step(mods):
    trainer_mod, _ = mods
    config, ckpt = cartpole_setup(mods)
    with pytest.raises(NotImplementedError, match="fc_step"):
        trainer_mod.Trainer(ckpt, config, device="cuda", fc_optimizer=True)


def test_whole_steps_are_the_host_entry_on_the_gradients_read_back(mods, native):
    trainer_mod, _ = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32)
    batches = cuda_batches(config, 32, 4, seed=5)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **NEW)
    start = flat_state(trainer)
    assert start["steps_done"] == 0 and not start["moment1"].any() and not start["moment2"].any()
    grads, lrs = [], []
    for bt in batches:
        trainer.update_lr()
        trainer.update_weights(bt)
        grads.append(trainer._flat_grad.cpu().numpy().copy())
        lrs.append(trainer._lr_host)
        assert trainer.optimizer.param_groups[0]["lr"] == trainer._lr_host and isinstance(trainer._lr_host, float)
    assert len(set(lrs)) == 4
    want = ref.run_host_entry(native, "Adam", start["weights"], grads, lrs, weight_decay=config.weight_decay)
    got = flat_state(trainer)
    for key in ("weights", "moment1", "moment2"):
        assert same_bits(got[key], want[key]), key
    assert got["steps_done"] == trainer.training_step == 4
    # the parameters are the flat buffer: what the model reports is what the launches wrote
    for name, parameter in trainer.model.named_parameters():
        at = trainer.flat_weights.offsets[name]
        assert same_bits(parameter.detach().cpu().numpy().reshape(-1), want["weights"][at:at + parameter.numel()]), name
    trainer.optimizer.zero_grad()
    assert same_bits(trainer._flat_grad.cpu().numpy(), grads[-1])


@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_graphed_equals_eager_bit_for_bit(mods, optimizer):
    trainer_mod, models = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32, optimizer=optimizer, momentum=0.9)
    batches = cuda_batches(config, 32, 5, seed=5)
    if optimizer == "SGD":
        with pytest.raises(NotImplementedError, match="captures an Adam step"):
            trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=True, fc_step=True)
    runs = []
    for graph in (False, True):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, **NEW)
        out = []
        for bt in batches[:4]:
            trainer.update_lr()
            out.append(trainer.update_weights(bt))
        runs.append((out, flat_state(trainer), trainer))
    (eager, s_eager, t_eager), (graphed, s_graphed, t_graphed) = runs
    assert t_graphed._graph is not None and t_graphed.training_step == 4
    assert s_eager["steps_done"] == s_graphed["steps_done"] == 4, "the warm-up before the capture left its steps behind"
    for key in ("weights", "moment1", "moment2"):
        assert same_bits(s_eager[key], s_graphed[key]), key
    assert s_eager["moment1"].any()
    for a, b in zip(eager, graphed):
        assert same_bits(a[0], b[0]), "priorities"
        assert same_bits(np.array(a[1:], dtype=np.float32), np.array(b[1:], dtype=np.float32)), "losses"
    # publish other weights into the flat buffers of both: the next (replayed / eager) step starts from them
    torch.manual_seed(99)
    other = models.MuZeroNetwork(config).get_weights()
    losses = []
    for trainer in (t_eager, t_graphed):
        trainer.flat_weights.load_state_dict(other)
        trainer.update_lr()
        losses.append(trainer.update_weights(batches[4])[1])
    fresh = trainer_mod.Trainer({"weights": other, "training_step": 0, "optimizer_state": None}, config, device="cuda", **NEW)
    want = fresh.update_weights(batches[4])[1]          # (the loss is computed before the optimizer moves anything)
    assert abs(losses[0] - want) <= 1e-6 * abs(want) and abs(losses[1] - want) <= 1e-6 * abs(want)
    # ... and not from the trained ones: a third trainer takes the same five steps with nothing published in between; its
    # loss differs by more than the 1e-6 within which the two above agree with the fresh trainer's
    plain = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **NEW)
    for bt in batches[:4]:
        plain.update_lr()
        plain.update_weights(bt)
    plain.update_lr()
    unpublished = plain.update_weights(batches[4])[1]
    assert abs(losses[1] - unpublished) > 1e-5 * abs(want), "the published weights made no difference"
    assert same_bits(flat_state(t_eager)["weights"], flat_state(t_graphed)["weights"])


@pytest.mark.parametrize("writer", list(WAYS))
def test_checkpoints_cross_between_the_three_ways(mods, writer):
    trainer_mod, models = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32)
    batches = cuda_batches(config, 32, 5, seed=11)
    first = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **WAYS[writer])
    for bt in batches[:3]:
        first.update_lr()
        first.update_weights(bt)
    saved = {"weights": first.model.get_weights(), "training_step": first.training_step,
             "optimizer_state": first.optimizer_state()}
    # torch's format, whichever way wrote it: a plain torch.optim.Adam takes it
    plain_model = models.MuZeroNetwork(config)
    plain = torch.optim.Adam(plain_model.parameters(), lr=config.lr_init, weight_decay=config.weight_decay)
    assert set(saved["optimizer_state"]["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
    plain.load_state_dict(copy.deepcopy(saved["optimizer_state"]))
    count = len(list(plain_model.parameters()))
    assert sorted(saved["optimizer_state"]["state"]) == list(range(count))
    for index, parameter in enumerate(plain_model.parameters()):
        entry = saved["optimizer_state"]["state"][index]
        assert sorted(entry) == ["exp_avg", "exp_avg_sq", "step"] and float(entry["step"]) == 3.0
        assert entry["exp_avg"].shape == parameter.shape and entry["exp_avg"].device.type == "cpu"
    assert isinstance(saved["optimizer_state"]["param_groups"][0]["lr"], float)
    out = {}
    for way, how in WAYS.items():
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", **how)
        assert trainer.training_step == 3
        if way == "fc_optimizer":       # the moments arrived as they were written
            assert int(trainer.optimizer.steps_done.item()) == 3
            again = trainer.optimizer_state()
            for index in range(count):
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(again["state"][index][key], saved["optimizer_state"]["state"][index][key]), (index, key)
        losses = []
        for bt in batches[3:]:
            trainer.update_lr()
            losses.append(trainer.update_weights(bt)[1])
        assert trainer.training_step == 5 and trainer._lr_host == config.lr_init * config.lr_decay_rate ** (4 / 4)
        out[way] = (losses, {k: v.detach().clone() for k, v in trainer.model.state_dict().items()})
    # the figures of test_checkpoints_cross_between_the_two_paths: first loss within 1e-4 relative, at least 97 % of the
    # weights within 1e-4 after two more steps, every way against the library's
    for way in ("fc_step", "fc_optimizer"):
        assert abs(out[way][0][0] - out["library"][0][0]) <= 1e-4 * abs(out["library"][0][0]), way
        close = sum(int(((out[way][1][k] - out["library"][1][k]).abs() <= 1e-4).sum()) for k in out[way][1])
        assert close >= 0.97 * sum(v.numel() for v in out[way][1].values()), way


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_checkpoints_cross(mods, momentum):
    """SGD's state holds no step count and, for momentum 0, nothing at all; a state without buffers loads as zeros."""
    trainer_mod, _ = mods
    config, ckpt = cartpole_setup(mods, lr_decay_steps=4, batch_size=32, optimizer="SGD", momentum=momentum)
    batches = cuda_batches(config, 32, 5, seed=13)
    out = {}
    for writer in ("library", "fc_optimizer"):
        first = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **WAYS[writer])
        for bt in batches[:3]:
            first.update_lr()
            first.update_weights(bt)
        saved = {"weights": first.model.get_weights(), "training_step": 3, "optimizer_state": first.optimizer_state()}
        assert (len(saved["optimizer_state"]["state"]) > 0) == (momentum != 0.0)
        for reader in ("library", "fc_optimizer"):
            trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", **WAYS[reader])
            for bt in batches[3:]:
                trainer.update_lr()
                trainer.update_weights(bt)
            out[writer, reader] = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
    base = out["library", "library"]
    for key, weights in out.items():
        close = sum(int(((weights[k] - base[k]).abs() <= 1e-4).sum()) for k in base)
        assert close >= 0.97 * sum(v.numel() for v in base.values()), key


def test_fixture_g14_through_the_flat_optimizer(mods, pkg, native):
    """The reference's recorded CartPole steps (two Adam steps) with the tolerances of the existing GPU test: losses 1e-4,
    priorities 2e-3, at least 97 % of the weights within 1e-4; the library path's share from the same run beside it."""
    from parity_helpers import load_golden
    from test_trainer_cpu import batch_of
    trainer_mod, _ = mods
    fx = load_golden("g14_trainer_cartpole")
    w = load_golden("cartpole_weights")
    shares = {}
    for way in ("library", "fc_optimizer"):
        config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
        config.batch_size = 32
        weights = {k: torch.from_numpy(w[k]) for k in w.files}
        trainer = trainer_mod.Trainer({"weights": weights, "training_step": 0, "optimizer_state": None}, config, device="cuda",
                                      **WAYS[way])
        within = total = 0
        for step in range(2):
            trainer.update_lr()
            assert trainer.optimizer.param_groups[0]["lr"] == float(fx[f"lr{step}"])
            batch = tuple(b.to("cuda") if torch.is_tensor(b) else b for b in batch_of(fx, True))
            priorities, *losses = trainer.update_weights(batch)
            if way == "fc_optimizer":
                np.testing.assert_allclose(losses, fx[f"losses{step}"], rtol=1e-4, atol=1e-4)
                np.testing.assert_allclose(priorities, fx[f"priorities{step}"], rtol=2e-3, atol=2e-3)
            for k, t in trainer.model.get_weights().items():
                d = np.abs(t.numpy() - fx[f"w{step}_{k}"])
                within, total = within + int((d <= 1e-4).sum()), total + d.size
        shares[way] = within / total
    REPORT["whole_steps"]["g14_share_of_weights_within_1e-4"] = shares
    print(f"\nG14: weights within 1e-4: fc_step + fc_optimizer {shares['fc_optimizer']:.4f}, library {shares['library']:.4f}")
    assert shares["fc_optimizer"] >= 0.97


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
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, **NEW)
    before = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
    stored = {g: rb.download_priorities(g)[0].copy() for g in rb.buffer}
    losses = trainer.train_steps(rb, 4)
    assert trainer.training_step == 4 and len(losses) == 4 and all(np.isfinite(losses))
    assert int(trainer.optimizer.steps_done.item()) == 4
    assert all(bool((v != before[k]).any()) for k, v in trainer.model.state_dict().items())
    assert any(not np.array_equal(rb.download_priorities(g)[0], stored[g]) for g in rb.buffer), "no priority was updated"
    one_more = trainer.train_steps(rb, 1)
    assert trainer.training_step == 5 and len(one_more) == 4 and int(trainer.optimizer.steps_done.item()) == 5
    rb.close()


def test_twentyone_shaped_sgd_under_capture_three_steps_vs_float64(mods, native):
    """TwentyOne's training settings (SGD, momentum 0.9, lr 0.03, 3 x 3 x 3 observations, two actions) on a fully-connected
    network: three captured steps of the new way against the same three steps in float64 on the CPU, the library being
    today's eager Trainer (torch forward, backward and SGD in float32 on the GPU)."""
    trainer_mod, models = mods
    config = importlib.import_module("muzero-hypermodel_amd.games.twentyone").MuZeroConfig()
    for key, value in dict(network="fullyconnected", batch_size=32, num_unroll_steps=5, lr_decay_steps=4, PER=True).items():
        setattr(config, key, value)
    assert config.optimizer == "SGD" and config.momentum == 0.9 and config.stacked_observations == 0
    torch.manual_seed(3)
    ckpt = {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}
    batches = cuda_batches(config, 32, 3, seed=7)
    runs = {}
    for way, how in (("native", dict(graph=True, **NEW)), ("library", {})):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **how)
        before = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
        for bt in batches:
            trainer.update_lr()
            trainer.update_weights(bt)
        runs[way] = {k: (v.detach().double().cpu() - before[k].double().cpu()) for k, v in trainer.model.state_dict().items()}
        if way == "native":
            assert trainer._graph is not None and int(trainer.optimizer.steps_done.item()) == 3
    # the same three steps in float64 on the CPU (the recipe of test_sgd_update_is_linear_in_the_gradient_...)
    model64 = models.MuZeroNetwork(config)
    model64.load_state_dict(copy.deepcopy(ckpt["weights"]))
    model64 = model64.double()
    model64._zero_reward_cache = None
    start = {k: v.detach().clone() for k, v in model64.state_dict().items()}
    optimizer = torch.optim.SGD(model64.parameters(), lr=config.lr_init, momentum=config.momentum,
                                weight_decay=config.weight_decay)

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
        worst[key], REPORT["whole_steps"].setdefault("twentyone_sgd_three_captured_steps", {})[key] = ratio(
            runs["native"][key].numpy(), runs["library"][key].numpy(), exact)
    top = max(worst, key=worst.get)
    print(f"\nthree captured SGD steps, TwentyOne-shaped: worst native error / allowed {worst[top]:.3f} ({top})")
    assert worst[top] <= 1.0, (top, worst[top])
