"""Weight gradients folded and the optimizer applied in one HIP launch (include/mztrain.h mztrain_fold_step,
csrc/grad_fold.hip; Trainer(native_optimizer=True)) on the MI355X.

The launch against mztrain_fold_reference on the host, bit for bit, on the case list of tests/grad_fold_reference.py, between
NaN guard bands, with the gradient buffer pre-filled with NaN, twice; captured after one eager call and replayed on other slot
contents.  Then whole steps through the Trainer: one eager step against the four-flag trainer (gradients and running
statistics bit for bit, weights and moments the host optimizer replayed on the gradients read back), captured against eager
bit for bit under Adam and SGD, train_steps, checkpoints crossing both ways, a per-call fallback that raises, inference after
flagged steps, and four steps at a decaying rate held to a float64 twin by the training-step rule (native error <= 4
max(library error, 4 * 2^-24 max|value|), the library being the four-flag trainer with torch's Adam).  The worst ratio and
the largest weight difference go into measure_out/native_optimizer_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import fc_optimizer_reference as optref
import grad_fold_reference as ref
from bn_epilogue_reference import ratio
from unroll_loss_reference import torch_reference

pytestmark = pytest.mark.gpu

GUARD = 256
REPORT = {}
FOUR = dict(native_epilogue=True, native_conv=True, native_heads=True, native_rescale=True)
FIVE = dict(native_optimizer=True, **FOUR)
OPT_CASES = [(label, decay) for label in ref.KINDS for decay in ref.DECAYS]
OPT_IDS = [f"{l}-wd{d:g}" for l, d in OPT_CASES]
LAYOUTS = ref.the_case_list()


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "native_optimizer_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


# ---- the launch against the host entry ---------------------------------------------------------------------------------------
class Guarded:
    """`values` between two NaN bands; `shift` floats past a 16-byte boundary."""

    def __init__(self, values, shift=0):
        n = len(values)
        self.buf = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=torch.float32, device="cuda")
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        assert (self.view.data_ptr() % 16 == 0) == (shift % 4 == 0)

    def host(self):
        return self.view.cpu().numpy()

    def bands_untouched(self):
        host = self.buf.cpu().numpy()
        return bool(np.isnan(host[:self.lo]).all() and np.isnan(host[self.hi:]).all())


class Device:
    """A handle and the device buffers of one case; the gradient buffer starts full of NaN."""

    def __init__(self, native, layout, kind, momentum, weights, shift=0):
        self.native, self.lib, self.layout, self.kind, self.momentum = native, native.load(), layout, kind, momentum
        start = ref.start_state(layout, weights)
        self.buffers = {"weights": Guarded(start["weights"], shift), "grads": Guarded(np.full(layout.n, np.nan), shift),
                        "moment1": Guarded(start["moment1"], shift), "moment2": Guarded(start["moment2"], shift)}
        self.staging = Guarded(np.full(layout.staging_floats, np.nan), shift)
        self.lr = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.done = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.handle = ctypes.c_void_p()
        rc = self.lib.mztrain_fold_create(layout.segments(native), len(layout.counts), layout.n, layout.staging_floats,
                                          torch.cuda.current_device(), ctypes.byref(self.handle))
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))
        rc = self.lib.mztrain_fold_set_uses(self.handle, ref.uses_array(layout.uses), len(layout.uses))
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))

    def close(self):
        torch.cuda.synchronize()
        self.lib.mztrain_fold_destroy(self.handle)

    def queue(self, weight_decay):
        adam = self.kind == "Adam"
        b = self.buffers
        args = ref.fold_args(self.native, self.kind, self.layout.n, b["weights"].view.data_ptr(), b["grads"].view.data_ptr(),
                             b["moment1"].view.data_ptr() if adam or self.momentum != 0.0 else None,
                             b["moment2"].view.data_ptr() if adam else None, self.lr.data_ptr(), self.done.data_ptr(),
                             self.staging.view.data_ptr(), self.layout.staging_floats, weight_decay=weight_decay,
                             momentum=self.momentum)
        rc = self.lib.mztrain_fold_step(self.handle, ctypes.byref(args), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))

    def load(self, staging, rate):
        self.staging.view.copy_(torch.from_numpy(staging))
        self.lr.fill_(rate)

    def check(self, want, what):
        torch.cuda.synchronize()
        layout = self.layout
        inside = layout.inside()
        used = np.zeros(layout.n, dtype=bool)
        for at, count, uses in zip(layout.offsets, layout.counts, layout.uses):
            used[at:at + count] = uses > 0
        assert int(self.done.item()) == want["steps_done"], what
        for key, guarded in self.buffers.items():
            got = guarded.host()
            assert guarded.bands_untouched(), (what, key, "guard band")
            if key == "grads":          # written where a segment was used, NaN as before everywhere else
                assert ref.same_bits(got[used], want[key][used]) and np.isnan(got[~used]).all(), (what, key)
            else:
                assert ref.same_bits(got, want[key]), (what, key)
                assert (got[~inside] == ref.SENTINEL).all(), (what, key, "a float outside every segment was written")
        assert self.staging.bands_untouched()


@pytest.mark.parametrize("label,decay", OPT_CASES, ids=OPT_IDS)
def test_the_launch_equals_the_host_entry_bit_for_bit(native, label, decay):
    kind, momentum = ref.KINDS[label]["kind"], ref.KINDS[label].get("momentum", 0.0)
    lrs = ref.learning_rates()
    # the case list, and the first mixed layout once more with every base pointer one float past a 16-byte boundary
    runs = [(name, layout, 0) for name, layout in LAYOUTS] + [("mixed-uses-aligned-bases-shifted", LAYOUTS[3][1], 1)]
    assert "mixed-uses-aligned" == LAYOUTS[3][0]
    for name, layout, shift in runs:
        weights, stagings = layout.make_case()
        want = ref.run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
        for attempt in range(2):
            device = Device(native, layout, kind, momentum, weights, shift)
            for staging, rate in zip(stagings, lrs):
                device.load(staging, rate)
                device.queue(decay)
            device.check(want, (name, attempt))
            device.close()


@pytest.mark.parametrize("label", list(ref.KINDS))
def test_a_captured_launch_replays_on_other_slot_contents(native, label):
    kind, momentum = ref.KINDS[label]["kind"], ref.KINDS[label].get("momentum", 0.0)
    lrs = ref.learning_rates()
    for name, layout in (LAYOUTS[3], LAYOUTS[7]):
        weights, stagings = layout.make_case(seed=5)
        want = ref.run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=1e-4, momentum=momentum)
        device = Device(native, layout, kind, momentum, weights)
        device.load(stagings[0], lrs[0])
        device.queue(1e-4)                                       # one eager call
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            device.queue(1e-4)
        torch.cuda.synchronize()
        assert int(device.done.item()) == 1, "the capture itself ran the step"
        for staging, rate in zip(stagings[1:], lrs[1:]):
            device.load(staging, rate)
            graph.replay()
        device.check(want, name)
        del graph
        device.close()


def test_the_handles_refusals(native):
    lib = native.load()
    layout = ref.Layout([5, 257], [1, 2], capacity=3)
    weights, stagings = layout.make_case()
    device = Device(native, layout, "Adam", 0.0, weights)

    def refused(rc, text):
        message = (lib.mzmcts_last_error(None) or b"").decode()
        assert rc == native.ERR_INVALID and text in message, (rc, message)

    refused(lib.mztrain_fold_set_uses(device.handle, ref.uses_array([1, 4]), 2), "uses outside [0, capacity] (segment 1)")
    refused(lib.mztrain_fold_set_uses(device.handle, ref.uses_array([1]), 1), "n_segments is not the handle's")
    refused(lib.mztrain_fold_set_uses(device.handle, None, 2), "null uses")
    b = device.buffers
    pointers = (b["weights"].view.data_ptr(), b["grads"].view.data_ptr(), b["moment1"].view.data_ptr(),
                b["moment2"].view.data_ptr(), device.lr.data_ptr(), device.done.data_ptr(), device.staging.view.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    for n, floats, text in ((layout.n + 1, layout.staging_floats, "opt.n is not"), (layout.n, layout.staging_floats - 1,
                                                                                    "staging_floats below")):
        args = ref.fold_args(native, "Adam", n, *pointers, floats)
        refused(lib.mztrain_fold_step(device.handle, ctypes.byref(args), stream), text)
    fresh = ctypes.c_void_p()
    assert lib.mztrain_fold_create(layout.segments(native), 2, layout.n, layout.staging_floats, torch.cuda.current_device(),
                                   ctypes.byref(fresh)) == 0
    args = ref.fold_args(native, "Adam", layout.n, *pointers, layout.staging_floats)
    refused(lib.mztrain_fold_step(fresh, ctypes.byref(args), stream), "mztrain_fold_set_uses has not been called")
    lib.mztrain_fold_destroy(fresh)
    torch.cuda.synchronize()
    assert ref.same_bits(b["weights"].host(), ref.start_state(layout, weights)["weights"]), "a refused call wrote"
    device.close()


# ---- whole steps through the Trainer ---------------------------------------------------------------------------------------------
def setup(models, **over):
    from test_gpu_bn_epilogue import tictactoe_setup
    config, ckpt = tictactoe_setup(models, unroll=5, seed=over.pop("seed", 3))
    config.weight_decay = 1e-4
    for key, value in over.items():
        setattr(config, key, value)
    return config, ckpt


def batches_of(config, count, seed, size=8):
    from test_gpu_bn_epilogue import make_batch
    return [tuple(t.cuda() for t in make_batch(config, size, seed=seed + i)) for i in range(count)]


def flat_state(trainer):
    opt = trainer.optimizer
    return {"weights": trainer.flat_weights.flat.cpu().numpy().copy(), "moment1": opt.moment1.cpu().numpy().copy(),
            "moment2": opt.moment2.cpu().numpy().copy(), "steps_done": int(opt.steps_done.item())}


def statistics(trainer):
    return {k: v.detach().cpu().numpy().copy() for k, v in trainer.model.state_dict().items()
            if k.endswith(("running_mean", "running_var"))}


def test_the_refusals_that_need_a_model_on_the_gpu(mods):
    trainer_mod, models = mods
    config, ckpt = setup(models)
    with pytest.raises(NotImplementedError, match=r"native_optimizer=True\) is the residual networks' way; fc_step"):
        trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", fc_step=True, **FIVE)
    config.resnet_fc_reward_layers = [8, 8]                       # a reward head the head launches do not cover
    torch.manual_seed(3)
    ckpt = {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}
    with pytest.raises(NotImplementedError, match=r"no HIP training launch covers the module of parameter "
                                                  r"dynamics_network\.module\.conv1x1_reward\.weight"):
        trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **FIVE)
    trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **FOUR)      # the four flags alone take that network


def test_one_eager_step_against_the_four_flag_trainer(native, mods):
    trainer_mod, models = mods
    config, ckpt = setup(models)
    batch = batches_of(config, 1, seed=17)[0]
    new = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **FIVE)
    old = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **FOUR)
    assert isinstance(old.optimizer, torch.optim.Adam) and isinstance(new.optimizer, trainer_mod.FoldOptimizer)
    start = flat_state(new)
    out_new = new.update_weights(batch)
    out_old = old.update_weights(batch)
    assert ref.same_bits(out_new[0], out_old[0]) and out_new[1:] == out_old[1:], "the loss is computed before anything moves"
    assert all(p.grad is None for p in new.model.parameters())
    grads = new.gradients()
    theirs = {name: p.grad for name, p in old.model.named_parameters()}
    stats_new, stats_old = statistics(new), statistics(old)
    assert list(grads) == list(theirs) and len(grads) + len(stats_new) == 58
    for name, view in grads.items():
        assert view.shape == theirs[name].shape and ref.same_bits(view.cpu().numpy(), theirs[name].cpu().numpy()), name
    for name in stats_old:
        assert ref.same_bits(stats_new[name], stats_old[name]), name
    # what the parameters' uses were: the representation network's once, the others once per position they saw
    uses = dict(zip(new.optimizer.sink.names, new.optimizer.uploaded_uses))
    assert set(uses.values()) == {1, 5, 6} and all(
        u == (1 if n.startswith("representation") else 5 if n.startswith("dynamics") else 6) for n, u in uses.items())
    # weights and moments: the flat-buffer optimizer's host entry on the gradients read back, parameter by parameter
    flat_grad = new._flat_grad.cpu().numpy().copy()
    want = optref.run_host_entry(native, "Adam", start["weights"], [flat_grad], [new._lr_host], weight_decay=1e-4)
    got = flat_state(new)
    assert got["steps_done"] == 1
    inside = np.zeros(new.flat_weights.numel, dtype=bool)
    for name, p in new.model.named_parameters():
        at = new.flat_weights.offsets[name]
        inside[at:at + p.numel()] = True
    for key in ("weights", "moment1", "moment2"):
        assert ref.same_bits(got[key][inside], want[key][inside]), key
    # outside the parameters: no moment, no gradient, and the statistics are the forward launches' alone (checked above)
    assert not got["moment1"][~inside].any() and not got["moment2"][~inside].any() and not flat_grad[~inside].any()
    assert (~inside).sum() == sum(v.size for v in stats_new.values())


@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_captured_equals_eager_bit_for_bit(mods, optimizer):
    trainer_mod, models = mods
    config, ckpt = setup(models, optimizer=optimizer, momentum=0.9, lr_decay_rate=0.8, lr_decay_steps=4)
    batches = batches_of(config, 3, seed=40)
    runs = []
    for graph in (False, True):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, **FIVE)
        out = []
        for bt in batches:
            trainer.update_lr()
            out.append(trainer.update_weights(bt))
        runs.append((out, flat_state(trainer), trainer))
    (eager, s_eager, _), (graphed, s_graphed, t_graphed) = runs
    assert t_graphed._graph is not None and t_graphed.training_step == 3
    assert s_eager["steps_done"] == s_graphed["steps_done"] == 3, "the warm-up before the capture left its steps behind"
    for key in ("weights", "moment1", "moment2"):
        assert ref.same_bits(s_eager[key], s_graphed[key]), key
    assert s_eager["moment1"].any() and (optimizer == "SGD" or s_eager["moment2"].any())
    for a, b in zip(eager, graphed):
        assert ref.same_bits(a[0], b[0]), "priorities"
        assert ref.same_bits(np.array(a[1:], dtype=np.float32), np.array(b[1:], dtype=np.float32)), "losses"
    assert {k: int(v) for k, v in t_graphed.model.state_dict().items() if k.endswith("num_batches_tracked")} == \
        {k: int(v) for k, v in runs[0][2].model.state_dict().items() if k.endswith("num_batches_tracked")}


def tictactoe_games(sp, config, n_games, seed):
    rs = np.random.RandomState(seed)
    A, L = len(config.action_space), config.max_moves
    visits = rs.random_sample((n_games, L, A)) + 0.01
    return sp.PackedGames(env_index=np.arange(n_games), length=rs.randint(5, L + 1, size=n_games).astype(np.int32),
                          observations=rs.random_sample((n_games, L + 1) + tuple(config.observation_shape)).astype(np.float32),
                          actions=rs.randint(0, A, size=(n_games, L + 1)).astype(np.int32),
                          rewards=rs.random_sample((n_games, L + 1)), to_play=np.zeros((n_games, L + 1), dtype=np.int32),
                          child_visits=visits / visits.sum(axis=2, keepdims=True), root_values=rs.random_sample((n_games, L)))


@pytest.mark.parametrize("graph", [False, True])
def test_train_steps_on_a_device_sampling_buffer(mods, graph):
    trainer_mod, models = mods
    rb_mod = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    config, ckpt = setup(models, batch_size=8, replay_buffer_size=40, lr_decay_steps=4)
    rb = rb_mod.ReplayBuffer({"num_played_games": 0, "num_played_steps": 0}, {}, config, device_sampling=True)
    rb.save_games(tictactoe_games(sp, config, 12, seed=2))
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, **FIVE)
    before = trainer.flat_weights.flat.clone()
    losses = trainer.train_steps(rb, 3)
    assert trainer.training_step == 3 and len(losses) == 4 and all(np.isfinite(losses))
    assert int(trainer.optimizer.steps_done.item()) == 3
    assert bool((trainer.flat_weights.flat != before).any())
    trainer.train_steps(rb, 1)
    assert trainer.training_step == 4 and int(trainer.optimizer.steps_done.item()) == 4
    rb.close()


def test_a_per_call_fallback_raises_and_names_the_parameter(mods):
    trainer_mod, models = mods
    config, ckpt = setup(models)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **FIVE)
    batch = batches_of(config, 1, seed=3)[0]
    trainer.update_weights(batch)
    name, module = next((n, m) for n, m in trainer.model.named_modules()
                        if isinstance(m, models.BoardConv2d) and m.__dict__.get("_train_on") and n.startswith("prediction"))
    module.__dict__["_train_on"] = False                          # its calls now take torch's convolution, per call
    with pytest.raises(NotImplementedError, match=(name + ".weight").replace(".", r"\.") + " came through autograd"):
        trainer.update_weights(batch)


@pytest.mark.parametrize("graph", [False, True])
def test_inference_after_flagged_training_equals_an_unflagged_twins(mods, graph):
    """The fold launch writes the weights behind their version counters; the trainer moves the counters itself, after an
    eager step and after a replay."""
    trainer_mod, models = mods
    config, ckpt = setup(models)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", graph=graph, **FIVE)
    observations = torch.rand((8,) + tuple(config.observation_shape), device="cuda")
    action = torch.randint(0, 9, (8, 1), device="cuda")

    def infer(model):
        model.eval()
        with torch.no_grad():
            value, reward, policy, state = model.initial_inference(observations)
            out = model.recurrent_inference(state, action)
        model.train()
        return [t.clone() for t in (value, policy, state, *out)]

    infer(trainer.model)                                           # fills the inference caches from the initial weights
    for bt in batches_of(config, 2, seed=30):
        trainer.update_weights(bt)
    twin = models.MuZeroNetwork(config)
    twin.set_weights(copy.deepcopy(trainer.model.get_weights()))
    twin.cuda()
    for a, b in zip(infer(trainer.model), infer(twin)):
        assert torch.equal(a, b)
    # publish: an actor-side flat buffer receives what the launches wrote
    weights_mod = importlib.import_module("muzero-hypermodel_amd.weights")
    actor = models.MuZeroNetwork(config).cuda()
    flat = weights_mod.FlatWeights(actor)
    trainer.publish(flat)
    assert torch.equal(flat.flat, trainer.flat_weights.flat)


# ---- four steps at a decaying rate, and checkpoints crossing, against a float64 twin -------------------------------------------
def tensors(model):
    return {k: v.detach().double().cpu().numpy().copy() for k, v in model.state_dict().items() if v.dtype.is_floating_point}


@pytest.fixture(scope="module")
def four_steps(native, mods):
    """Computed once: from a checkpoint an unflagged trainer wrote after three steps (moments three steps old: from zero
    moments Adam's first updates are lr * g / (|g| + eps) whatever the size of g, and elements whose gradient is rounding noise
    then move by a sizeable part of lr in any float32 run), four steps with a learning rate that decays every step --
      library   the four-flag trainer, torch's Adam
      native    Trainer(native_optimizer=True)
      to_old    two flagged steps, its checkpoint into a four-flag trainer, two more
      to_new    two four-flag steps, its checkpoint into a flagged trainer, two more
      exact     the same model and torch's Adam in float64 on the CPU."""
    from test_gpu_bn_epilogue import follow
    from test_gpu_unroll_loss import _scalar_to_support64
    trainer_mod, models = mods
    config, ckpt = setup(models, seed=8, lr_decay_rate=0.8, lr_decay_steps=4)
    batches = batches_of(config, 7, seed=60)
    writer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda")
    follow(writer, batches[:3])

    def saved_by(trainer):
        return {"weights": copy.deepcopy(trainer.model.get_weights()), "training_step": trainer.training_step,
                "optimizer_state": trainer.optimizer_state()}

    saved = saved_by(writer)
    runs = {}
    for name, first, second in (("library", FOUR, FOUR), ("native", FIVE, FIVE), ("to_old", FIVE, FOUR), ("to_new", FOUR, FIVE)):
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", **first)
        follow(trainer, batches[3:5])
        if first is not second:
            middle = saved_by(trainer)
            assert middle["training_step"] == 5 and sorted(middle["optimizer_state"]["state"]) == list(range(
                len(list(trainer.model.parameters()))))
            assert all(float(e["step"]) == 5.0 for e in middle["optimizer_state"]["state"].values())
            trainer = trainer_mod.Trainer(copy.deepcopy(middle), config, device="cuda", **second)
        follow(trainer, batches[5:])
        assert trainer.training_step == 7
        runs[name] = tensors(trainer.model)
    model64 = models.MuZeroNetwork(config)
    model64.set_weights(copy.deepcopy(saved["weights"]))
    model64 = model64.double()
    model64._zero_reward_cache = None
    model64.refresh_inference_constants()
    model64.train()
    optimizer = torch.optim.Adam(model64.parameters(), lr=config.lr_init, weight_decay=config.weight_decay)
    optimizer.load_state_dict(copy.deepcopy(saved["optimizer_state"]))
    helpers = types.SimpleNamespace(scalar_to_support=_scalar_to_support64, support_to_scalar=models.support_to_scalar)
    for index, bt in enumerate(batches[3:]):
        for group in optimizer.param_groups:
            group["lr"] = config.lr_init * config.lr_decay_rate ** ((3 + index) / config.lr_decay_steps)
        obs, act, val, rew, pol, weight, scale = (t.cpu() for t in bt)
        steps = trainer_mod.Trainer._unroll(types.SimpleNamespace(model=model64), obs.double(), act.long().unsqueeze(-1))
        b64 = {"values": val.double(), "rewards": rew.double(), "policies": pol.double(), "gradient_scales": scale.double(),
               "weights": weight.double() if config.PER else None}
        loss, _, _ = torch_reference(trainer_mod, helpers, [s[0] for s in steps], [s[1] for s in steps], [s[2] for s in steps],
                                     b64, config.support_size, config.value_loss_weight, config.PER_alpha)
        optimizer.zero_grad()
        loss.mean().backward()
        optimizer.step()
    runs["exact"] = tensors(model64)
    return runs


@pytest.mark.parametrize("way", ["native", "to_old", "to_new"])
def test_four_steps_meet_the_training_step_rule(four_steps, way):
    """native: figures from the MI355X are in DESIGN.md 7.17 (worst ratio, largest weight difference to the library)."""
    exact, library, mine = four_steps["exact"], four_steps["library"], four_steps[way]
    assert set(exact) == set(library) == set(mine) and len(exact) == 58
    worst, entries = {}, {}
    for name, x64 in exact.items():
        worst[name], entries[name] = ratio(mine[name], library[name], x64)
    top = max(worst, key=worst.get)
    apart = max(float(np.abs(mine[k] - library[k]).max()) for k in exact)
    REPORT[way] = {"worst_ratio": worst[top], "worst_tensor": top, "largest_weight_difference_to_library": apart,
                   "entry": entries[top]}
    print(f"\nfour steps, {way}: worst native error / allowed {worst[top]:.3f} ({top}); largest difference to the four-flag "
          f"trainer {apart:.3e}")
    assert worst[top] <= 1.0, (way, top, entries[top])
