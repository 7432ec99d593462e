"""Device replay store (include/mzreplay.h) against the reference's ReplayBuffer (fixtures G12)
and the oracle restatement: priorities to float32 rounding, sampled indices / values / rewards / policies /
actions / gradient scales / stacked observations / importance weights bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from parity_helpers import history_of, load_golden
from test_oracle_replay import NAMES, cfg_of, games_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def config_of(fx, name):
    mod = importlib.import_module(f"muzero-hypermodel_amd.games.{name.split('_')[0]}")
    config = mod.MuZeroConfig()
    config.batch_size = int(fx["batch_size"])
    config.stacked_observations = int(fx["stacked_observations"])
    config.PER = bool(fx["PER"])
    assert config.td_steps == int(fx["td_steps"]) and config.num_unroll_steps == int(fx["num_unroll_steps"])
    assert config.seed == int(fx["seed"]) and float(config.discount) == float(fx["cfg_discount"])
    return config


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("packed", [False, True])
def test_replay_store_matches_reference(pkg, name, packed):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    fx = load_golden(f"g12_replay_{name}")
    config = config_of(fx, name)
    G = len(fx["lengths"])
    rb = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)
    if packed:
        L = fx["actions"].shape[1] - 1
        batch = sp.PackedGames(env_index=np.arange(G), length=fx["lengths"], observations=fx["observations"],
                               actions=fx["actions"], rewards=fx["rewards"], to_play=fx["to_play"],
                               child_visits=fx["child_visits"], root_values=fx["root_values"])
        assert L <= config.max_moves
        rb.save_games(batch)
    else:
        for g in range(G):
            rb.save_game(history_of(sp, fx, g))
    assert rb.num_played_games == G and rb.total_samples == int(fx["lengths"].sum())
    if config.PER:
        for g in range(G):
            n = int(fx["lengths"][g])
            want = fx["priorities"][g, :n]
            got = rb.buffer[g]["priorities"]
            # |root - target| ** alpha goes through the device's pow(): equal up to one float32 rounding step
            np.testing.assert_allclose(got, want, rtol=2e-7, atol=0)
            assert abs(rb.buffer[g]["game_priority"] - fx["game_priority"][g]) <= 2e-7 * fx["game_priority"][g]
            # sample with the reference's priorities, so that the draws below can be compared one for one
            rb.buffer[g]["priorities"] = want.copy()
            rb.buffer[g]["game_priority"] = fx["game_priority"][g]
    index_batch, (obs, act, val, rew, pol, weight, scale) = rb.get_batch()
    assert np.array_equal(np.array(index_batch), fx["index_batch"])
    assert np.array_equal(act.cpu().numpy(), fx["action_batch"])
    assert np.array_equal(val.cpu().numpy(), fx["value_batch"])            # fp64, the reference's summation order
    assert np.array_equal(rew.cpu().numpy(), fx["reward_batch"])
    assert np.array_equal(pol.cpu().numpy(), fx["policy_batch"])
    assert np.array_equal(scale.cpu().numpy(), fx["gradient_scale_batch"])
    assert np.array_equal(obs.cpu().numpy(), fx["observation_batch"])
    if config.PER:
        assert np.array_equal(weight, fx["weight_batch"])
    rb.close()


def test_replay_store_ring_and_priority_updates(pkg):
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    ro = importlib.import_module("replay_oracle")
    fx = load_golden("g12_replay_cartpole")
    config = config_of(fx, "cartpole")
    config.replay_buffer_size = 10                      # smaller than the 24 games: the oldest are dropped
    rb = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)
    for g in range(len(fx["lengths"])):
        rb.save_game(history_of(sp, fx, g))
    assert sorted(rb.buffer) == list(range(14, 24)) and rb.total_samples == int(fx["lengths"][14:].sum())
    games, cfg = games_of(fx, ro), cfg_of(fx)
    index_batch, (obs, act, val, rew, pol, weight, scale) = rb.get_batch()
    val = val.cpu().numpy()
    for b, (gid, pos) in enumerate(index_batch):
        assert 14 <= gid < 24
        for u in range(config.num_unroll_steps + 1):
            if pos + u < fx["lengths"][gid]:
                assert val[b, u] == ro.compute_target_value(games[gid], pos + u, cfg["td_steps"], cfg["discount"])
    # update_priorities (replay_buffer.py:197-220)
    gid, pos = index_batch[0]
    new = np.full((1, config.num_unroll_steps + 1), 7.5, dtype=np.float32)
    rb.update_priorities(new, [(gid, pos)])
    n = rb.buffer[gid]["length"]
    assert (rb.buffer[gid]["priorities"][pos: min(n, pos + 11)] == 7.5).all() and rb.buffer[gid]["game_priority"] == 7.5
    rb.close()


def test_reanalyse_values_and_targets(pkg):
    """Reanalyse on the device store vs fixture G13 (the reference's per-game step and the targets built on top)."""
    from parity_helpers import cartpole_model_and_weights
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    models_mod = importlib.import_module("muzero-hypermodel_amd.models")
    fx = load_golden("g13_reanalyse_cartpole")
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    _, weights = cartpole_model_and_weights(models_mod, config, "cpu")
    G = len(fx["lengths"])
    rb = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config)
    for g in range(G):
        rb.save_game(history_of(sp, fx, g))
    re = rb_mod.Reanalyse({"weights": weights, "num_reanalysed_games": 0}, config)
    for g in range(G):
        n = int(fx["lengths"][g])
        assert np.array_equal(rb.game_observations(g).cpu().numpy().reshape(n, -1),
                              fx["observations"][g, :n].reshape(n, -1))          # stacked_observations == 0 here
        gid, values = re.reanalyse_game(rb, g)
        want = fx["reanalysed"][g, :n]
        np.testing.assert_allclose(values.cpu().numpy(), want, rtol=3e-5, atol=1e-5)   # fp32 network, decoded values
        rb.set_reanalysed_values(g, want)      # the reference's own values: the targets below compare bit for bit
    assert re.num_reanalysed_games == G
    slots = fx["pairs"][:, 0].astype(np.int32)
    positions = fx["pairs"][:, 1].astype(np.int32)
    out = rb.make_targets(slots, positions, fx["action_targets"].astype(np.int32))
    assert np.array_equal(out["value"].cpu().numpy(), fx["value_targets"])       # float32 accumulation where bootstrapped
    assert np.array_equal(out["reward"].cpu().numpy(), fx["reward_targets"])
    assert np.array_equal(out["policy"].cpu().numpy(), fx["policy_targets"])
    assert np.array_equal(out["action"].cpu().numpy(), fx["action_targets"])
    rb.save_game(history_of(sp, fx, 0))        # a new game in a reanalysed slot forgets the old values
    rb.close()


def test_trainer_on_device_matches_reference(pkg):
    """Trainer.update_weights on the MI355X from CUDA-tensor batches vs the reference's CPU run (fixture G14, CartPole
    FC network, two Adam steps): learning rates equal, losses to 1e-5, and EVERY weight within 2e-6 of the reference's
    after each step (measured: 3e-7).  Adam's first steps are lr * g / (|g| + eps) -- the sign of the gradient -- so this
    also says that no gradient of this network is zero up to rounding."""
    from test_trainer_cpu import run_steps
    fx = load_golden("g14_trainer_cartpole")
    tr, out = run_steps(pkg, fx, "cuda", True)
    assert next(tr.model.parameters()).is_cuda
    for step, (lr, priorities, losses, weights) in enumerate(out):
        assert lr == float(fx[f"lr{step}"])
        np.testing.assert_allclose(losses, fx[f"losses{step}"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(priorities, fx[f"priorities{step}"], rtol=2e-3, atol=2e-3)   # sqrt(|.|): steep at 0
        for k, got in weights.items():
            assert np.abs(got - fx[f"w{step}_{k}"]).max() <= 2e-6, (step, k)


def test_resnet_trainer_on_device_matches_reference(pkg):
    """Fixture G16 on the MI355X: two Trainer steps on the TicTacToe residual network (trainer.py:124-298; training-mode
    BatchNorm, 3x3 / 1x1 convolutions forward and backward through PyTorch-ROCm, 20 unrolled positions).

    What can differ from the reference's CPU run, and why -- each asserted:
    * the unroll is a 20-fold iteration of dynamics + per-plane min-max rescale under batch statistics, and for these
      weights it amplifies a rounding difference by < 2x per unrolled position (measured 1.8x: 2e-6 at the root, 0.4 at
      position 20).  So the logits of position k agree with the CPU run of the same modules (which the CPU suite pins to
      the reference at 2e-6) within 1e-5 * 2^k, the first positions at 1e-5;
    * hence the losses agree to 5e-4 relative (measured 1.4e-4) and a gradient to a few percent of its tensor's largest
      entry (measured <= 6.2 %);
    * Adam's first step moves a weight by lr * g / (|g| + eps) = lr * sign(g): after step 0 an entry may leave the
      reference's weight ONLY if the reference's own gradient (recorded in the fixture) is below 10 % of its tensor's
      largest -- small enough for the deviation above to flip its sign -- and then by at most 2 lr; every other entry
      agrees to 1e-6.  Measured: 243 of 21 715 entries, largest relative gradient among them 4 %;
    * after step 1 (weights one flipped step apart) the tensors follow the reference's update as in the CPU test."""
    from synth import synthetic_state_dict
    from test_trainer_cpu import batch_of
    fx = load_golden("g16_trainer_tictactoe")
    tr_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    config.batch_size = 24
    template = models.MuZeroNetwork(config).state_dict()
    weights = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(template, 0).items()}

    def trainer(device):
        return tr_mod.Trainer({"weights": {k: v.clone() for k, v in weights.items()}, "training_step": 0,
                               "optimizer_state": None}, config, device=device)

    def batch(device):
        return tuple(b.to(device) if torch.is_tensor(b) else b for b in batch_of(fx, True))

    # the unroll, position by position, against the CPU run of the same modules
    logits = {}
    for device in ("cpu", "cuda"):
        tr = trainer(device)
        b = tr._batch_on_device(batch(device))
        logits[device] = [[t.detach().double().cpu() for t in step] for step in tr._unroll(b["observations"], b["actions"])]
    growth = []
    for k, (cpu_step, gpu_step) in enumerate(zip(logits["cpu"], logits["cuda"])):
        worst = 0.0
        for x, y in zip(cpu_step, gpu_step):
            finite = torch.isfinite(x)                       # (the root position's reward logits are log(one_hot))
            worst = max(worst, float((x[finite] - y[finite]).abs().max()))
        growth.append(worst)
        assert worst <= 1e-5 * 2.0 ** k, (k, worst)
    assert max(growth[:3]) <= 1e-5
    print("logit deviation per unrolled position:", " ".join(f"{g:.1e}" for g in growth))

    tr = trainer("cuda")
    lr = float(config.lr_init)
    for step in range(2):
        tr.update_lr()
        assert tr._lr_host == float(fx[f"lr{step}"])
        priorities, total, v, r, p = tr.update_weights(batch("cuda"))
        grads = {k: prm.grad.detach().cpu().numpy() for k, prm in tr.model.named_parameters()}
        got_w = {k: t.detach().cpu().numpy() for k, t in tr.model.get_weights().items()}
        # (step 1 runs on weights of which ~1 % sit 2 lr away from the reference's, through the same 20-fold unroll:
        # measured 0.9 % on the losses)
        np.testing.assert_allclose([total, v, r, p], fx[f"losses{step}"], rtol=5e-4 if step == 0 else 2e-2)
        if step == 0:
            off = total_entries = 0
            for k, g_gpu in grads.items():
                g_ref = fx[f"g0_{k}"]
                scale = float(np.abs(g_ref).max())
                assert np.abs(g_gpu - g_ref).max() <= 0.1 * scale, k               # measured <= 6.2 %
                dev = np.abs(got_w[k] - fx[f"w0_{k}"])
                moved = dev > 1e-6
                assert (np.abs(g_ref)[moved] <= 0.1 * scale).all(), k               # only sign-flippable entries leave
                assert dev.max() <= 2 * lr + 1e-6, k
                off += int(moved.sum())
                total_entries += dev.size
            print(f"entries that left the reference's weights after step 0: {off} of {total_entries}")
            assert off <= 0.03 * total_entries
        else:
            worst = 0.0
            for k, got in got_w.items():
                want = fx[f"w1_{k}"]
                if got.dtype.kind == "f":
                    # the second Adam step is lr * m / (sqrt(v) + eps) with m, v mixing both gradients: percent-level
                    # gradient differences show as a fraction of the step (measured: tensor means within 0.21 of it)
                    moved = np.abs(want - weights[k].numpy()).mean()
                    worst = max(worst, float(np.abs(got - want).mean() / (moved + 1e-12))) if moved > 1e-6 else worst
                    assert np.abs(got - want).mean() <= 0.35 * moved + 1e-7, (k, np.abs(got - want).mean(), moved)
                    if "running_" not in k:
                        assert np.abs(got - want).max() <= 4.5 * lr, k
                else:
                    assert np.array_equal(got, want), k
            print(f"after step 1: worst tensor-mean deviation / mean movement = {worst:.3f}")
