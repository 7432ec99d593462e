"""The 3 x 3 convolutions of a residual network in training as HIP launches (csrc/conv_train.hip, include/mztrain.h
mztrain_conv_*) on the GPU: the pack, forward, data-gradient and weight-gradient launches against the host entries bit for
bit between NaN guard bands on every shape of tests/conv_train_reference.SHAPES (every forward form either side of its
samples per workgroup, one, two and three slices of the weight gradient), twice and captured; exact on integer data against
torch's float64; against float64 by the project's training-step rule with torch's own float32 convolution and autograd on the
GPU as the library; exact properties of the autograd Function and the modules; one whole training step three ways against the
float64 model; and the flagged trainer captured into a hipGraph.  The ratios go into measure_out/conv_train_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import conv_train_reference as ref
from bn_epilogue_reference import ratio
from unroll_loss_reference import torch_reference

pytestmark = pytest.mark.gpu

GUARD = 252          # floats of NaN either side of a device tensor: a multiple of 4, the convolution launches move 16 bytes
ODD_GUARD = 251      # ... and an odd count for the weight gradient, which assumes no alignment beyond a float's
REPORT = {"kernel_vs_float64": {}, "whole_step": {}}
IDS = ["B{}-{}to{}-{}x{}-dx{}".format(*s) for s in ref.SHAPES]


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "conv_train_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Guarded:
    """A float32 device tensor of `shape` between two NaN bands (NaN itself where `values` is None)."""

    def __init__(self, shape, values=None, guard=GUARD):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
        self.lo, self.hi = guard, guard + n
        self.view = self.buf[self.lo:self.hi].view(shape)
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        return self.view.cpu().numpy()

    def bands_untouched(self):
        host = self.buf.cpu().numpy()
        return bool(np.isnan(host[:self.lo]).all() and np.isnan(host[self.hi:]).all())


class Launches:
    """The four launches of one shape on guarded tensors; queue() puts them on the current stream."""

    def __init__(self, native, shape, x, w, dy):
        self.native, self.lib, self.shape = native, native.load(), shape
        b, cin, cout, h, wd, dx_planes = shape
        lib = self.lib
        self.t = {"x": Guarded(x.shape, x), "w": Guarded(w.shape, w), "dy": Guarded(dy.shape, dy),
                  "x_odd": Guarded(x.shape, x, ODD_GUARD), "dy_odd": Guarded(dy.shape, dy, ODD_GUARD),
                  "packed": Guarded((lib.mzmcts_board_conv_packed_floats(cin, cout),)),
                  "affine": Guarded((2 * native.CONV_AFFINE,)),
                  "y": Guarded((b, cout, h, wd)), "dw": Guarded(w.shape, guard=ODD_GUARD)}
        if dx_planes:
            self.t["packed_dx"] = Guarded((lib.mzmcts_board_conv_packed_floats(cout, dx_planes),))
            self.t["dx"] = Guarded((b, dx_planes, h, wd))

    def queue(self):
        native, lib, t = self.native, self.lib, self.t
        b, cin, cout, h, wd, dx_planes = self.shape
        stream = torch.cuda.current_stream().cuda_stream
        dims = dict(batch=b, cin=cin, cout=cout, height=h, width=wd)
        calls = [("mztrain_conv_pack", native.MzTrainConvPackArgs(
            weight=t["w"].ptr(), packed=t["packed"].ptr(), packed_dx=t["packed_dx"].ptr() if dx_planes else None,
            affine=t["affine"].ptr(), cin=cin, cout=cout, dx_planes=dx_planes)),
            ("mztrain_conv_forward", native.MzTrainConvForwardArgs(
                x=t["x"].ptr(), packed=t["packed"].ptr(), affine=t["affine"].ptr(), weight=None, y=t["y"].ptr(), **dims))]
        if dx_planes:
            calls.append(("mztrain_conv_dgrad", native.MzTrainConvDgradArgs(
                dy=t["dy"].ptr(), packed_dx=t["packed_dx"].ptr(), affine=t["affine"].ptr(), weight=None, dx=t["dx"].ptr(),
                dx_planes=dx_planes, **dims)))
        calls.append(("mztrain_conv_wgrad", native.MzTrainConvWgradArgs(x=t["x_odd"].ptr(), dy=t["dy_odd"].ptr(),
                                                                        dw=t["dw"].ptr(), **dims)))
        for name, args in calls:
            rc = getattr(lib, name)(ctypes.byref(args), stream)
            assert rc == 0, (name, rc, lib.mzmcts_last_error(None))

    def load(self, x, w, dy):
        with torch.no_grad():
            for key, value in (("x", x), ("x_odd", x), ("w", w), ("dy", dy), ("dy_odd", dy)):
                self.t[key].view.copy_(torch.from_numpy(value))

    def results(self):
        torch.cuda.synchronize()
        for key, tensor in self.t.items():
            assert tensor.bands_untouched(), f"{key}: a guard band was written"
        return {key: self.t[key].host() for key in ("y", "dx", "dw", "packed", "packed_dx", "affine") if key in self.t}


def run_device(native, shape, x, w, dy):
    launches = Launches(native, shape, x, w, dy)
    launches.queue()
    got = launches.results()
    for key, value in (("x", x), ("w", w), ("dy", dy)):
        assert same_bits(launches.t[key].host(), value), f"{key} was written"
    return got


def run_host(native, shape, x, w, dy):
    lib = native.load()
    dx_planes = shape[5]
    packed, packed_dx, affine = ref.host_pack(native, lib, w, dx_planes)
    want = {"y": ref.host_forward(native, lib, x, w), "dw": ref.host_wgrad(native, lib, x, dy), "packed": packed,
            "affine": affine}
    if dx_planes:
        want["dx"], want["packed_dx"] = ref.host_dgrad(native, lib, dy, w, dx_planes), packed_dx
    return want


def assert_same(got, want, what=""):
    assert set(got) == set(want)
    for key, value in want.items():
        assert same_bits(got[key], value), f"{what}{key}: bits differ"


def tictactoe_scaled(shape, seed):
    """Random normal data at the magnitudes a TicTacToe step shows: activations of order 1 (post-ReLU states lie in [0, 1],
    batch-norm outputs around 1), weights of order 0.1 (Kaiming-uniform at 16 channels), gradients of order 1e-3."""
    return ref.normal_case(shape, seed, x_scale=1.0, w_scale=0.1, dy_scale=1e-3)


# ---- bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_give_the_host_entries_bits(native, shape):
    """y, dx, dw, both packings and the ones | zeros pair, bit for bit; a second run gives the same bits."""
    x, w, dy = tictactoe_scaled(shape, seed=1)
    want = run_host(native, shape, x, w, dy)
    first = run_device(native, shape, x, w, dy)
    assert_same(first, want)
    assert_same(run_device(native, shape, x, w, dy), first, "second run: ")


@pytest.mark.parametrize("shape", [(33, 17, 16, 3, 3, 16), (21, 64, 64, 3, 3, 0), (17, 17, 16, 6, 6, 16), (5, 80, 64, 6, 7, 64)],
                         ids=lambda s: "B{}-{}to{}-{}x{}-dx{}".format(*s))
def test_captured_launches_replay_the_eager_bits(native, shape):
    """The four launches captured into a hipGraph on one set of inputs and replayed on another: the host entries' bits of
    the second set -- the replay repacks the weight it finds."""
    first, second = tictactoe_scaled(shape, seed=2), tictactoe_scaled(shape, seed=3)
    launches = Launches(native, shape, *first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches.queue()                                          # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches.queue()
    launches.load(*second)
    graph.replay()
    assert_same(launches.results(), run_host(native, shape, *second), "replayed: ")


# ---- exact on integers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_are_exact_on_integers(native, shape):
    """x in [-3, 3], w and dy in [-2, 2]: every partial sum is far below 2^24, so the three outputs equal torch's float64
    convolution and autograd on the CPU exactly, whatever the order of the sums."""
    x, w, dy = ref.integer_case(shape, seed=5)
    got = run_device(native, shape, x, w, dy)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xt, wt, padding=1)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    assert np.array_equal(got["y"], y.detach().numpy())
    assert np.array_equal(got["dw"], wt.grad.numpy())
    if shape[5]:
        assert np.array_equal(got["dx"], xt.grad.numpy()[:, :shape[5]])


# ---- against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_meet_the_training_step_rule(native, shape):
    """native error <= 4 max(library error, 4 * 2^-24 max|x64|) per tensor; the library is torch's float32 convolution and
    its autograd on the GPU, on the same tensors.  With 64 channels a float32 chain of 576 to 720 terms is by itself at 0.7
    to 1.2 of what the floor term alone would allow in y and dx (computed from the host entries, which give the kernels'
    bits); the library's float32 sums err alike, which is what the max in the rule is for.  Measured worst ratios on the
    MI355X: y 0.94, dx 0.74, dw 0.33."""
    x, w, dy = tictactoe_scaled(shape, seed=7)
    dx_planes = shape[5]
    got = run_device(native, shape, x, w, dy)
    xt, wt = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(w).cuda().requires_grad_()
    y = torch.nn.functional.conv2d(xt, wt, padding=1)
    y.backward(torch.from_numpy(dy).cuda())
    library = {"y": y.detach().cpu().numpy(), "dx": xt.grad.cpu().numpy()[:, :dx_planes], "dw": wt.grad.cpu().numpy()}
    exact = {"y": ref.forward(x, w), "dw": ref.wgrad_exact(x, dy)}
    if dx_planes:
        exact["dx"] = ref.dgrad(dy, w, dx_planes)
    report = {key: ratio(got[key], library[key], exact[key]) for key in exact}
    label = "B{}-{}to{}-{}x{}-dx{}".format(*shape)
    REPORT["kernel_vs_float64"][label] = {key: entry for key, (_, entry) in report.items()}
    print(f"\n{label}: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in report.items()))
    top = max(report, key=lambda k: report[k][0])
    assert report[top][0] <= 1.0, (top, report[top][1])


# ---- properties -------------------------------------------------------------------------------------------------------------
def module_of(models, w):
    conv = models.conv3x3(w.shape[1], w.shape[0]).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
    assert conv.native_training(True)
    return conv


def through_the_module(models, shape, x, w, dy, strided):
    conv = module_of(models, w)

    def dev(a):
        t = torch.from_numpy(a).cuda()
        if strided:
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert not t.is_contiguous()
        return t

    xt = dev(x).requires_grad_()
    assert conv.takes_training_path(xt)
    y = conv(xt)
    assert type(y.grad_fn).__name__.startswith("_TrainingConv3x3")
    y.backward(dev(dy))
    back = lambda t: t.detach().cpu().numpy()
    return {"y": back(y), "dx": back(xt.grad), "dw": back(conv.weight.grad)}


def test_non_contiguous_inputs_give_the_contiguous_bits(native, mods):
    _, models = mods
    shape = (5, 16, 16, 6, 6, 16)
    x, w, dy = tictactoe_scaled(shape, seed=11)
    want = {k: v for k, v in run_host(native, shape, x, w, dy).items() if k in ("y", "dx", "dw")}
    assert_same(through_the_module(models, shape, x, w, dy, strided=False), want, "contiguous: ")
    assert_same(through_the_module(models, shape, x, w, dy, strided=True), want, "strided: ")


def test_an_unaligned_view_gives_the_same_bits(native, mods):
    """A contiguous view that starts 36 bytes into its storage (one 3 x 3 plane) is copied to an aligned tensor first."""
    _, models = mods
    shape = (4, 1, 16, 3, 3, 0)
    x, w, dy = tictactoe_scaled(shape, seed=12)
    conv = module_of(models, w)
    wide = torch.from_numpy(np.concatenate([x[:1], x])).cuda()
    view = wide[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    y = conv(view)
    y.backward(torch.from_numpy(dy).cuda())
    want = run_host(native, shape, x, w, dy)
    assert same_bits(y.detach().cpu().numpy(), want["y"]) and same_bits(conv.weight.grad.cpu().numpy(), want["dw"])


def test_gradients_nobody_needs_are_none(native, mods):
    _, models = mods
    shape = (6, 16, 16, 3, 3, 16)
    x, w, dy = tictactoe_scaled(shape, seed=13)
    conv = module_of(models, w)
    xt = torch.from_numpy(x).cuda()                                # no gradient asked for: no data-gradient launch
    y = conv(xt)
    assert type(y.grad_fn).__name__.startswith("_TrainingConv3x3")
    y.backward(torch.from_numpy(dy).cuda())
    assert xt.grad is None and same_bits(conv.weight.grad.cpu().numpy(), run_host(native, shape, x, w, dy)["dw"])
    conv.weight.grad = None
    conv.weight.requires_grad_(False)
    xt.requires_grad_()
    conv(xt).backward(torch.from_numpy(dy).cuda())
    assert conv.weight.grad is None and same_bits(xt.grad.cpu().numpy(), run_host(native, shape, x, w, dy)["dx"])
    with torch.no_grad():
        assert not conv.takes_training_path(xt)                    # gradients disabled: torch's convolution
    obs = torch.from_numpy(x[:, :3].copy()).cuda().requires_grad_()
    stem = module_of(models, w[:, :3].copy())                       # 3 planes that need a gradient: no packing covers them
    assert stem.training_dx_planes() == 0 and not stem.takes_training_path(obs) and stem.takes_training_path(obs.detach())
    assert type(stem(obs).grad_fn).__name__.startswith("Conv")


def test_a_nan_in_one_samples_gradient_reaches_dw_and_only_that_samples_dx(native):
    shape = (6, 16, 16, 3, 3, 16)
    x, w, dy = tictactoe_scaled(shape, seed=14)
    base = run_device(native, shape, x, w, dy)
    poisoned = dy.copy()
    poisoned[4, 3, 1, 1] = np.nan
    got = run_device(native, shape, x, w, poisoned)
    others = [0, 1, 2, 3, 5]
    assert same_bits(got["dx"][others], base["dx"][others]) and np.isnan(got["dx"][4]).all()     # 3 x 3: every tap reaches
    assert np.isnan(got["dw"][3]).all()                            # a border tap multiplies a zero: NaN there too
    rest = [c for c in range(16) if c != 3]
    assert same_bits(got["dw"][rest], base["dw"][rest]) and same_bits(got["y"], base["y"])


def test_the_dynamics_input_gets_a_gradient_for_its_state_planes_only(native, mods):
    """The action plane goes in apart from the state: the Function returns the data gradient of the 16 state planes -- the
    host entry's bits -- and None for the plane, even for a plane that asks for a gradient; an input that needs a gradient
    on all 17 planes takes torch's convolution; and a flagged model's dynamics() follows an unflagged twin."""
    _, models = mods
    shape = (6, 17, 16, 3, 3, 16)
    x, w, dy = tictactoe_scaled(shape, seed=15)
    conv = module_of(models, w)
    state = torch.from_numpy(x[:, :16].copy()).cuda().requires_grad_()
    plane = torch.from_numpy(x[:, 16:].copy()).cuda().requires_grad_()
    assert conv.takes_training_path(state, extra_plane=True) and conv.training_dx_planes() == 16
    y = conv.training_forward(state, plane)
    y.backward(torch.from_numpy(dy).cuda())
    want = run_host(native, shape, x, w, dy)
    assert plane.grad is None and state.grad.shape == (6, 16, 3, 3)
    assert same_bits(y.detach().cpu().numpy(), want["y"]) and same_bits(state.grad.cpu().numpy(), want["dx"])
    assert same_bits(conv.weight.grad.cpu().numpy(), want["dw"])
    whole = torch.from_numpy(x).cuda().requires_grad_()
    assert not conv.takes_training_path(whole) and type(conv(whole).grad_fn).__name__.startswith("Conv")
    assert conv.takes_training_path(whole.detach())

    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    torch.manual_seed(4)
    model = models.MuZeroNetwork(config).cuda().train()
    twin = copy.deepcopy(model)
    assert model.native_training_conv(True) >= 5 and twin.native_training_conv(False) == 0
    action = torch.randint(0, 9, (8, 1), device="cuda")
    start = torch.rand(8, 16, 3, 3, device="cuda")
    grads = []
    for net in (model, twin):
        hidden = start.clone().requires_grad_()
        next_state, reward = net.dynamics(hidden, action)
        (next_state.sum() + reward.sum()).backward()
        grads.append((hidden.grad.clone(), net.dynamics_network.module.conv.weight.grad.clone()))
    for a, b in zip(*grads):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


def test_inference_after_flagged_training_equals_an_unflagged_twins(native, mods):
    """The training packings are buffers of their own: after flagged steps the model's inference paths (whose caches were
    filled before the steps) give the bits of a fresh model that took the same weights."""
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=2)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", native_conv=True)
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
    for i in range(2):
        trainer.update_weights(tuple(t.cuda() for t in make_batch(config, 8, seed=30 + i)))
    twin = models.MuZeroNetwork(config)
    twin.set_weights(copy.deepcopy(trainer.model.get_weights()))
    twin.cuda()
    for a, b in zip(infer(trainer.model), infer(twin)):
        assert torch.equal(a, b)


# ---- a whole step -----------------------------------------------------------------------------------------------------------
def test_one_training_step_three_ways_vs_float64(native, mods):
    """The construction of test_one_training_step_with_and_without_the_flag_vs_float64: the TicTacToe residual config with 5
    unrolled steps, B = 8, one update_weights with Trainer(native_conv=True), one with native_epilogue as well and one with
    neither (the library); every parameter gradient and every batch norm's running statistics of both flagged ways against
    the same model in float64 on the CPU, per tensor native error <= 4 max(library error, 4 u max|x64|)."""
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    from test_gpu_unroll_loss import _scalar_to_support64
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=5)
    batch = make_batch(config, 8, seed=17)
    ways = {"conv": dict(native_conv=True), "conv+epilogue": dict(native_conv=True, native_epilogue=True), "library": {}}
    runs = {}
    for name, flags in ways.items():
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **flags)
        convs = [m for m in trainer.model.modules() if isinstance(m, models.BoardConv2d)]
        assert len(convs) >= 5 and all(bool(m.__dict__.get("_train_on")) is bool(flags) for m in convs)
        trainer.update_weights(tuple(t.cuda() for t in batch))
        tensors = {k: p.grad.detach().double().cpu() for k, p in trainer.model.named_parameters() if p.grad is not None}
        state = trainer.model.state_dict()
        tensors.update({k: v.detach().double().cpu() for k, v in state.items() if k.endswith(("running_mean", "running_var"))})
        runs[name] = tensors
    model64 = models.MuZeroNetwork(config)
    model64.set_weights(copy.deepcopy(ckpt["weights"]))
    model64 = model64.double()
    model64._zero_reward_cache = None
    model64.refresh_inference_constants()
    model64.train()
    observations, actions, values, rewards, policies, weights, scales = batch
    steps = trainer_mod.Trainer._unroll(types.SimpleNamespace(model=model64), observations.double(),
                                        actions.long().unsqueeze(-1))
    b64 = {"values": values.double(), "rewards": rewards.double(), "policies": policies.double(),
           "gradient_scales": scales.double(), "weights": weights.double() if config.PER else None}
    helpers = types.SimpleNamespace(scalar_to_support=_scalar_to_support64, support_to_scalar=models.support_to_scalar)
    loss, _, _ = torch_reference(trainer_mod, helpers, [s[0] for s in steps], [s[1] for s in steps], [s[2] for s in steps],
                                 b64, config.support_size, config.value_loss_weight, config.PER_alpha)
    loss.mean().backward()
    exact = {k: p.grad.detach() for k, p in model64.named_parameters() if p.grad is not None}
    exact.update({k: v.detach() for k, v in model64.state_dict().items() if k.endswith(("running_mean", "running_var"))})
    assert set(exact) == set(runs["conv"]) == set(runs["conv+epilogue"]) == set(runs["library"]) and len(exact) >= 20
    for way in ("conv", "conv+epilogue"):
        worst = {}
        REPORT["whole_step"][way] = {}
        for name, x64 in exact.items():
            worst[name], REPORT["whole_step"][way][name] = ratio(runs[way][name].numpy(), runs["library"][name].numpy(),
                                                                 x64.numpy())
        top = max(worst, key=worst.get)
        print(f"\nwhole step, {way}: {len(worst)} tensors, worst native error / allowed {worst[top]:.3f} ({top})")
        assert worst[top] <= 1.0, (way, top, REPORT["whole_step"][way][top])


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_graphed_flagged_trainer_resumes_from_an_unflagged_checkpoint_and_follows_the_eager_one(native, mods):
    """Trainer(graph=True, native_conv=True), built from a checkpoint that an unflagged eager trainer wrote after three steps,
    over four steps with a decaying learning rate and a batch that changes between replays: it follows the eager flagged
    trainer resumed from the same checkpoint within 1e-5 on the weights (the tolerance, and the reason for not starting from
    fresh weights, of the epilogue's test of the same name).  Replays repack: after the run every module's forward packing
    is the packing of the weights the LAST step started from, not of the weights the capture saw."""
    from test_gpu_bn_epilogue import assert_follows, follow, make_batch, tictactoe_setup
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=5, seed=8)
    config.lr_decay_rate, config.lr_decay_steps = 0.8, 4          # a decay that shows within a few steps
    batches = [tuple(t.cuda() for t in make_batch(config, 16, seed=60 + i)) for i in range(7)]
    writer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda")
    follow(writer, batches[:3])
    saved = {"weights": copy.deepcopy(writer.model.get_weights()), "training_step": writer.training_step,
             "optimizer_state": writer.optimizer_state()}
    runs = []
    for graph in (False, True):
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", graph=graph, native_conv=True)
        convs = [m for m in trainer.model.modules() if isinstance(m, models.BoardConv2d)]
        assert trainer.training_step == 3 and all(m.__dict__.get("_train_on") for m in convs)
        out, before_last = [], None
        for i, bt in enumerate(batches[3:]):
            trainer.update_lr()
            if i == 3:
                before_last = [m.weight.detach().cpu().numpy().copy() for m in convs]
            out.append(trainer.update_weights(bt))
        runs.append((out, {k: v.clone() for k, v in trainer.model.state_dict().items()}))
        assert trainer.training_step == 7
        for conv, weight in zip(convs, before_last):
            packed, packed_dx, _ = conv.training_buffers()
            want, want_dx, _ = ref.host_pack(native, native.load(), weight, conv.training_dx_planes())
            assert same_bits(packed.cpu().numpy(), want), "the last step did not repack"
            assert packed_dx is None or same_bits(packed_dx.cpu().numpy(), want_dx)
            assert not same_bits(conv.weight.detach().cpu().numpy(), weight)
    assert_follows(runs[0], runs[1], "resumed, graphed vs eager, both native_conv")
