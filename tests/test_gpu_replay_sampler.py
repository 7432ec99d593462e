"""The replay store's device sampler (ReplayBuffer(device_sampling=True): include/mzreplay.h mzreplay_sample_batch,
mzreplay_make_batch_device, mzreplay_update_priorities; arithmetic in csrc/replay_sampler.h) on the MI355X: against the
reference's recorded batches (fixtures G12), against the host sampling path draw for draw -- through priority updates,
ring wrap-around and a sweep of shapes -- and under Trainer.train_steps against host-sampled training steps."""
import copy
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parity_helpers import history_of, load_golden
from test_gpu_replay import config_of
from test_oracle_replay import NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
START = {"num_played_games": 0, "num_played_steps": 0}


@pytest.fixture(scope="module")
def mods(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return (importlib.import_module("muzero-hypermodel_amd.replay_buffer"),
            importlib.import_module("muzero-hypermodel_amd.self_play"))


def cast32(t):
    return t.float().cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_device_sampler_matches_reference(mods, name):
    rb_mod, sp = mods
    fx = load_golden(f"g12_replay_{name}")
    config = config_of(fx, name)
    G = len(fx["lengths"])
    rb = rb_mod.ReplayBuffer(START, {}, config, device_sampling=True)
    for g in range(G):
        rb.save_game(history_of(sp, fx, g))
    if config.PER:
        for g in range(G):
            n = int(fx["lengths"][g])
            got, got_game = rb.download_priorities(g)          # what mzreplay_add_games left on the device
            np.testing.assert_allclose(got, fx["priorities"][g, :n], rtol=2e-7, atol=0)
            assert abs(got_game - fx["game_priority"][g]) <= 2e-7 * fx["game_priority"][g]
            rb.buffer[g]["priorities"] = fx["priorities"][g, :n]   # the reference's own, so the draws compare one for one
            assert np.array_equal(rb.buffer[g]["priorities"], fx["priorities"][g, :n])
            assert rb.buffer[g]["game_priority"] == fx["game_priority"][g]
    index_batch, (obs, act, val, rew, pol, weight, scale) = rb.get_batch()
    assert np.array_equal(np.array(index_batch.tolist()), fx["index_batch"])
    assert act.dtype == torch.int64 and val.dtype == rew.dtype == pol.dtype == scale.dtype == torch.float32
    assert np.array_equal(act.cpu().numpy(), fx["action_batch"])
    for got, key in ((val, "value_batch"), (rew, "reward_batch"), (pol, "policy_batch"), (scale, "gradient_scale_batch"),
                     (obs, "observation_batch")):
        assert np.array_equal(got.cpu().numpy(), cast32(torch.from_numpy(fx[key]))), key   # the trainer's cast
    if config.PER:
        assert np.array_equal(weight.cpu().numpy().view(np.uint32), fx["weight_batch"].view(np.uint32))
    else:
        assert weight is None
    rb.close()


def synthetic_config(A, max_moves, batch, capacity, per, unroll=5, seed=3):
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    config.action_space = list(range(A))
    config.observation_shape = (1, 1, 2)
    config.max_moves, config.batch_size, config.replay_buffer_size = max_moves, batch, capacity
    config.PER, config.num_unroll_steps, config.td_steps, config.seed = per, unroll, 3, seed
    return config


def synthetic_games(sp, rs, config, n_games, lengths=None):
    A, L = len(config.action_space), config.max_moves
    length = np.asarray(lengths if lengths is not None else rs.randint(1, L + 1, size=n_games), dtype=np.int32)
    visits = rs.random_sample((n_games, L, A)) + 0.01
    return sp.PackedGames(env_index=np.arange(n_games), length=length,
                          observations=rs.random_sample((n_games, L + 1, 1, 1, 2)).astype(np.float32),
                          actions=rs.randint(0, A, size=(n_games, L + 1)).astype(np.int32),
                          rewards=rs.random_sample((n_games, L + 1)), to_play=np.zeros((n_games, L + 1), dtype=np.int32),
                          child_visits=visits / visits.sum(axis=2, keepdims=True),
                          root_values=rs.random_sample((n_games, L)) * 4)


def assert_same_batch(host, dev, per):
    (h_index, h_batch), (d_index, d_batch) = host, dev
    assert d_index.tolist() == [list(map(int, pair)) for pair in h_index]
    for i, (h, d) in enumerate(zip(h_batch, d_batch)):
        if i == 5:
            if per:
                assert np.array_equal(d.cpu().numpy().view(np.uint32), np.asarray(h, dtype=np.float32).view(np.uint32))
            continue
        want = h.cpu().numpy() if i == 1 else cast32(h)
        assert np.array_equal(d.cpu().numpy(), want), i


def assert_same_priorities(host, dev):
    assert list(host.buffer) == list(dev.buffer)
    for gid, entry in host.buffer.items():
        got, got_game = dev.download_priorities(gid)
        assert np.array_equal(got.view(np.uint32), np.asarray(entry["priorities"], dtype=np.float32).view(np.uint32)), gid
        assert got_game == entry["game_priority"], gid


def test_lock_step_with_host_path_through_updates_and_evictions(mods):
    rb_mod, sp = mods
    config = synthetic_config(A=3, max_moves=24, batch=64, capacity=20, per=True, unroll=5, seed=9)
    rs = np.random.RandomState(4)
    host = rb_mod.ReplayBuffer(START, {}, config)
    dev = rb_mod.ReplayBuffer(START, {}, config, device_sampling=True)
    first = synthetic_games(sp, rs, config, 12)
    host.save_games(first)
    dev.save_games(first)
    for gid, entry in host.buffer.items():       # same starting priorities, to the bit (pow() differs host / device only
        dev.load_priorities(gid, entry["priorities"])   # in who rounds: both stores computed them on the device)
    U1 = config.num_unroll_steps + 1
    menu = np.array([0, 1e-12, 1e3, 0.5, 2.0], dtype=np.float32)
    for round_ in range(50):
        h, d = host.get_batch(), dev.get_batch()
        assert_same_batch(h, d, True)
        if round_ % 3 == 1:                      # new games arrive between the draw and its update: the ring wraps and
            more = synthetic_games(sp, rs, config, int(rs.randint(1, 9)))      # sampled games leave before their update
            host.save_games(more)
            dev.save_games(more)
        fresh = rs.choice(menu, size=(config.batch_size, U1)).astype(np.float32)
        fresh[rs.random_sample(fresh.shape) < 0.5] += np.float32(rs.random_sample())
        if round_ % 2:
            dev.update_priorities(torch.from_numpy(fresh).cuda(), d[0])       # the trainer's tensor and index object
        else:
            dev.update_priorities(fresh, d[0].tolist())
        host.update_priorities(fresh, h[0])
        assert_same_priorities(host, dev)
    assert host.num_played_games > 3 * config.replay_buffer_size          # the ring went round
    state = dev.sampler_state()
    want = host.rng.get_state()
    assert state[2] == want[2] and np.array_equal(state[1], want[1])
    host.close()
    dev.close()


SWEEP = [  # (A, games, batch, max_moves, unroll)
    (1, 1, 1, 1, 5), (2, 2, 127, 7, 5), (3, 7, 128, 40, 5), (9, 129, 129, 9, 20), (121, 129, 512, 121, 121),
    (2, 10000, 128, 30, 10), (9, 10000, 512, 9, 20), (3, 1, 129, 300, 3), (121, 7, 127, 50, 0),
]


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("shape", SWEEP)
def test_sweep_against_host_path(mods, shape, per):
    rb_mod, sp = mods
    A, n_games, batch, max_moves, unroll = shape
    config = synthetic_config(A, max_moves, batch, max(n_games, 2) if n_games < 10000 else 10000, per, unroll,
                              seed=A * 1000 + batch)
    rs = np.random.RandomState(n_games + batch)
    lengths = rs.randint(1, max_moves + 1, size=n_games)
    lengths[0], lengths[-1] = max_moves, 1 if n_games > 1 else max_moves       # both ends of the range
    games = synthetic_games(sp, rs, config, n_games, lengths)
    host = rb_mod.ReplayBuffer(START, {}, config)
    dev = rb_mod.ReplayBuffer(START, {}, config, device_sampling=True)
    host.save_games(games)
    dev.save_games(games)
    if per:
        for gid, entry in host.buffer.items():
            got, got_game = dev.download_priorities(gid)
            assert np.array_equal(got, entry["priorities"]) and got_game == entry["game_priority"]
    for _ in range(3):
        assert_same_batch(host.get_batch(), dev.get_batch(), per)
    state, want = dev.sampler_state(), host.rng.get_state()
    assert state[2] == want[2] and np.array_equal(state[1], want[1])
    host.close()
    dev.close()


@pytest.mark.parametrize("graph", [False, True])
def test_train_steps_equals_host_sampled_steps(mods, graph):
    rb_mod, sp = mods
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    config.batch_size, config.replay_buffer_size, config.lr_decay_steps = 32, 40, 4
    fx = load_golden("g12_replay_cartpole")
    torch.manual_seed(1)
    ckpt = {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}
    runs = []
    for device_sampling in (False, True):
        rb = rb_mod.ReplayBuffer(START, {}, config, device_sampling=device_sampling)
        for g in range(len(fx["lengths"])):
            rb.save_game(history_of(sp, fx, g))
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph)
        if device_sampling:
            losses = trainer.train_steps(rb, 4)
            stored = {g: rb.download_priorities(g) for g in rb.buffer}
        else:
            for _ in range(4):
                index_batch, batch = rb.get_batch()
                trainer.update_lr()
                priorities, *losses = trainer.update_weights(batch)
                rb.update_priorities(priorities, index_batch)
            stored = {g: (e["priorities"], e["game_priority"]) for g, e in rb.buffer.items()}
        runs.append((trainer.training_step, trainer._lr_host, losses, stored,
                     {k: v.clone() for k, v in trainer.model.state_dict().items()}))
        rb.close()
    (h_step, h_lr, h_losses, h_stored, h_w), (d_step, d_lr, d_losses, d_stored, d_w) = runs
    assert h_step == d_step == 4 and h_lr == d_lr
    np.testing.assert_allclose(d_losses, h_losses, rtol=1e-5)
    assert max(float((h_w[k] - d_w[k]).abs().max()) for k in h_w) <= 1e-5
    for g in h_stored:      # same batches, same kernels, same order: the stored priorities are the same floats
        assert np.array_equal(np.asarray(h_stored[g][0], dtype=np.float32), d_stored[g][0]), g
        assert h_stored[g][1] == d_stored[g][1]


def test_closed_cartpole_loop_reproduces_the_host_sampled_log():
    """tools/train_cartpole.py --device-sampling against the recorded host-sampled run: every column but the seconds."""
    want = [json.loads(line) for line in open(os.path.join(ROOT, "profiles", "r03_train_cartpole_e128.jsonl"))]
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_cartpole.py"), "--envs", "128", "--iterations",
                           "60", "--device-sampling"], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    got = [json.loads(line) for line in proc.stdout.splitlines() if line.startswith("{")]
    out_dir = os.environ.get("MZ_OUT_DIR", os.path.join(ROOT, "measure_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "train_cartpole_e128_device_sampling.jsonl"), "w") as f:
        f.write("".join(json.dumps(row) + "\n" for row in got))
    assert len(got) == len(want) == 60
    for g, w in zip(got, want):
        g, w = dict(g), dict(w)
        g.pop("seconds"), w.pop("seconds")
        assert g == w, (g, w)
