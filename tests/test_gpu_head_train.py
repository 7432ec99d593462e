"""The reward / value / policy heads of a residual network in training as HIP launches (csrc/head_train.hip, include/mztrain.h
mztrain_heads_*) on the GPU: the forward launch and the two backward launches against the host entries between NaN guard bands
on every shape of tests/head_train_reference.SHAPES -- bit for bit on integer data whose pre-activations are all positive,
within the header's ulp bound on random data --, twice and captured; against float64 by the project's training-step rule with
torch's own float32 modules and autograd on the GPU as the library; exact properties of the autograd Function; one whole
training step against the float64 model; and the flagged trainer captured into a hipGraph.  The ratios go into
measure_out/head_train_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import head_train_reference as ref
from bn_epilogue_reference import ratio
from unroll_loss_reference import torch_reference

pytestmark = pytest.mark.gpu

GUARD = 251          # floats of NaN either side of a device tensor; odd: the launches assume no alignment beyond a float's
REPORT = {"kernel_vs_float64": {}, "whole_step": {}}
IDS = [ref.shape_id(s) for s in ref.SHAPES]


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "head_train_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Launches:
    """The three launches of one case on device tensors between NaN bands; queue() puts them on the current stream."""

    def __init__(self, native, case, pre=None):
        self.native, self.lib, self.shape, self.pre = native, native.load(), case["shape"], pre
        self.inputs = [k for k in case if k != "shape"]
        dims = {k: case[k].shape for k in self.inputs}
        dims.update(ref.output_shapes(self.shape))
        self.buf, self.view = {}, {}
        for key, shape in dims.items():
            n = int(np.prod(shape))
            self.buf[key] = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
            self.view[key] = self.buf[key][GUARD:GUARD + n].view(shape)
        self.load(case)

    def load(self, case):
        with torch.no_grad():
            for key in self.inputs:
                self.view[key].copy_(torch.from_numpy(np.ascontiguousarray(case[key])))

    def queue(self, want_dx=True, wanted=ref.PARAMS):
        stream = torch.cuda.current_stream().cuda_stream
        address = lambda name: self.view[name].data_ptr()
        args = ref.forward_args(self.native, self.shape, address)
        rc = self.lib.mztrain_heads_forward(ctypes.byref(args), stream)
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))
        if self.pre is not None:                              # the directed pre-activations, -0.0 included, as they stand
            for k, value in self.pre.items():
                self.view[f"pre{k}"].copy_(torch.from_numpy(value))
        args = ref.backward_args(self.native, self.shape, address, want_dx=want_dx, wanted=wanted)
        rc = self.lib.mztrain_heads_backward(ctypes.byref(args), stream)
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))

    def results(self, case):
        torch.cuda.synchronize()
        for key, buf in self.buf.items():
            host = buf.cpu().numpy()
            assert np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all(), f"{key}: a guard band was written"
        for key in self.inputs:
            assert same_bits(self.view[key].cpu().numpy(), case[key]), f"{key} was written"
        return {key: self.view[key].cpu().numpy() for key in ref.output_shapes(self.shape)}


def run_device(native, case, pre=None):
    launches = Launches(native, case, pre)
    launches.queue()
    return launches.results(case)


def assert_same(got, want, what=""):
    assert set(got) == set(want)
    for key, value in want.items():
        assert same_bits(got[key], value), f"{what}{key}: bits differ"


def assert_within_ulp_bound(got, host, case, pre=None, what=""):
    tol = ref.ulp_bounds(case, ref.run64(case, pre=pre))
    assert set(tol) == set(host) == set(got)
    for key, bound in tol.items():
        excess = np.abs(got[key].astype(np.float64) - host[key].astype(np.float64)) - bound
        assert not np.isnan(got[key]).any() and float(excess.max()) <= 0.0, f"{what}{key}: {float(excess.max()):.3e} over the bound"


# ---- bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_give_the_host_entries_bits_on_positive_integers(native, shape):
    """Every fc1 pre-activation is a positive integer: no expm1f, no expf, and every output bit for bit; a second run too.
    The outputs also equal the float64 yardstick exactly."""
    case = ref.integer_case(shape, seed=5)
    want = ref.run_host_entry(native, case)
    first = run_device(native, case)
    assert_same(first, want)
    assert_same(run_device(native, case), first, "second run: ")
    exact = ref.run64(case)
    for key in want:
        assert np.array_equal(first[key].astype(np.float64), exact[key]), key


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_stay_within_the_ulp_bound_of_the_host_entries(native, shape):
    """Random data with pre-activations on both sides of zero: flat, pre and dfc2_b, which no ELU reaches, bit for bit; every
    other output within what MZTRAIN_HEADS_ELU_ULPS ulps of ELU and of its slope propagate to (ref.ulp_bounds); a second
    run gives the first one's bits."""
    case = ref.normal_case(shape, seed=1)
    host = ref.run_host_entry(native, case)
    assert any((host[f"pre{k}"] < 0).any() for k in range(len(shape[3])))
    first = run_device(native, case)
    assert_within_ulp_bound(first, host, case)
    for k in range(len(shape[3])):
        for key in (f"flat{k}", f"pre{k}", f"dfc2_b{k}"):
            assert same_bits(first[key], host[key]), key
    assert_same(run_device(native, case), first, "second run: ")


def test_the_directed_pre_activations_against_the_host_entries(native):
    """-20, -1, -1e-4, -0.0, +0.0, 1e-4 written into `pre` between the forward and the backward launches."""
    case = ref.directed_case()
    pre = {k: np.tile(np.array(ref.DIRECTED_PRE, dtype=np.float32), (case["shape"][0], 1)) for k in range(2)}
    host, got = ref.run_host_entry(native, case, pre=pre), run_device(native, case, pre=pre)
    assert_within_ulp_bound(got, host, case, pre=pre)
    for k in range(2):                                        # the slope at both zeros and on the positive side is exactly 1
        assert same_bits(got[f"dpre{k}"][:, 3:], host[f"dpre{k}"][:, 3:])


CAPTURED = [ref.SHAPES[0], ref.SHAPES[3], (17, 5, 6, ((3, 5, 4), (2, 3, 6))), (3, 8, 9, ((2, 5, 1), (2, 5, 121)))]


@pytest.mark.parametrize("shape", CAPTURED, ids=[ref.shape_id(s) for s in CAPTURED])
def test_captured_launches_replay_the_eager_bits(native, shape):
    """The three launches captured into a hipGraph on one set of inputs and replayed on another give the bits of an eager
    run on the second set."""
    first, second = ref.normal_case(shape, seed=2), ref.normal_case(shape, seed=3)
    eager = run_device(native, second)
    launches = Launches(native, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches.queue()                                          # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches.queue()
    launches.load(second)
    graph.replay()
    assert_same(launches.results(second), eager, "replayed: ")


def test_unwanted_outputs_are_left_alone(native):
    """dx == NULL and NULL gradient pointers: those tensors keep their NaN fill, the others keep their bits."""
    shape = (5, 4, 9, ((3, 7, 5), (2, 6, 2)))
    case = ref.normal_case(shape, seed=4)
    full = run_device(native, case)
    launches = Launches(native, case)
    launches.queue(want_dx=False, wanted=("conv_b", "fc1_w"))
    got = launches.results(case)
    for key, value in got.items():
        if key == "dx" or (key[0] == "d" and key[1:-1] in ref.PARAMS and key[1:-1] not in ("conv_b", "fc1_w")):
            assert np.isnan(value).all(), key
        else:
            assert same_bits(value, full[key]), key


# ---- against float64 ------------------------------------------------------------------------------------------------------
def check_the_rule(native, case, label):
    got = run_device(native, case)
    library = ref.run_torch(case, torch.float32, "cuda")
    exact = ref.run64(case)
    report = {key: ratio(got[key], library[key], exact[key]) for key in ref.outputs(case["shape"])}
    REPORT["kernel_vs_float64"][label] = {key: entry for key, (_, entry) in report.items()}
    top = max(report, key=lambda k: report[k][0])
    print(f"\n{label}: worst {top} {report[top][0]:.3f}")
    assert report[top][0] <= 1.0, (top, report[top][1])


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_kernels_meet_the_training_step_rule(native, shape):
    """native error <= 4 max(library error, 4 * 2^-24 max|x64|) per tensor, the saved flat and pre and the intermediate dpre
    and dflat included; the library is torch's float32 expression of the modules and its autograd on the GPU."""
    check_the_rule(native, ref.normal_case(shape, seed=7), ref.shape_id(shape))


def test_the_directed_pre_activations_meet_the_rule(native):
    check_the_rule(native, ref.directed_case(), "directed")


# ---- properties -------------------------------------------------------------------------------------------------------------
def heads_of(models, case, on=True):
    """[(conv, fc, flat size)] of torch modules that hold the case's parameters, switched to the HIP training path."""
    b, c, p, shapes = case["shape"]
    heads = []
    for k, (r, hd, o) in enumerate(shapes):
        conv, fc = models.PointwiseConv2d(c, r).cuda(), models.mlp(r * p, [hd], o).cuda()
        with torch.no_grad():
            for param, name in zip((conv.weight, conv.bias, fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias), ref.PARAMS):
                param.copy_(torch.from_numpy(case[f"{name}{k}"]).view(param.shape))
        conv.native_training = on
        heads.append((conv, fc, r * p))
    return heads


def through_the_function(models, case, x, x_grad=True):
    heads = heads_of(models, case)
    x = x.requires_grad_() if x_grad else x
    assert models._heads_take_training_path(x, heads)
    logits = models.conv_heads(x, heads)
    assert all(type(t.grad_fn).__name__.startswith("_TrainingHeads") for t in logits)
    sum((t * torch.from_numpy(case[f"dlogits{k}"]).cuda()).sum() for k, t in enumerate(logits)).backward()
    back = lambda t: t.detach().cpu().numpy()
    out = {f"logits{k}": back(t) for k, t in enumerate(logits)}
    if x_grad:
        out["dx"] = back(x.grad).reshape(case["x"].shape)
    for k, (conv, fc, _) in enumerate(heads):
        for param, name in zip((conv.weight, conv.bias, fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias), ref.PARAMS):
            out[f"d{name}{k}"] = back(param.grad).reshape(case[f"{name}{k}"].shape)
    return out, heads


def board(case, height):
    b, c, p, _ = case["shape"]
    return torch.from_numpy(case["x"]).cuda().view(b, c, height, p // height)


def test_non_contiguous_and_unaligned_inputs_give_the_contiguous_bits(native, mods):
    _, models = mods
    case = ref.normal_case((5, 16, 9, ref.TICTACTOE), seed=11, dlogits_scale=1.0)
    launched = run_device(native, case)
    want = {k: v for k, v in launched.items() if not k.startswith(("flat", "pre", "dpre", "dflat"))}
    assert_same(through_the_function(models, case, board(case, 3))[0], want, "contiguous: ")
    strided = board(case, 3).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not strided.is_contiguous()
    assert_same(through_the_function(models, case, strided)[0], want, "strided: ")
    wide = torch.cat([board(case, 3).reshape(-1)[:9], board(case, 3).reshape(-1)])
    view = wide[9:].view(5, 16, 3, 3)                             # starts 36 bytes into its storage
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert_same(through_the_function(models, case, view)[0], want, "unaligned: ")


def test_gradients_nobody_needs_are_none(native, mods):
    _, models = mods
    case = ref.normal_case((6, 16, 9, ref.TICTACTOE), seed=13, dlogits_scale=1.0)
    want = run_device(native, case)
    x = board(case, 3).requires_grad_()
    heads = heads_of(models, case)
    frozen = [heads[0][0].bias, heads[1][1][0].weight, heads[1][1][2].bias]
    captured = {}
    original = models._TrainingHeads.backward

    def spy(ctx, *grads):
        captured["returned"] = original(ctx, *grads)
        return captured["returned"]

    models._TrainingHeads.backward = staticmethod(spy)
    try:
        got, _ = through_the_function(models, case, board(case, 3), x_grad=False)     # no dx asked for: none computed
        assert captured["returned"][0] is None and all(g is not None for g in captured["returned"][2:])
        assert "dx" not in got and all(same_bits(got[k], want[k]) for k in got)
        for param in frozen:
            param.requires_grad_(False)
        logits = models.conv_heads(x, heads)
        sum((t * torch.from_numpy(case[f"dlogits{k}"]).cuda()).sum() for k, t in enumerate(logits)).backward()
    finally:
        models._TrainingHeads.backward = staticmethod(original)
    returned = captured["returned"]
    assert len(returned) == 14 and returned[1] is None
    none_at = [i for i, g in enumerate(returned) if g is None]
    assert none_at == [1, 2 + 1, 2 + 6 + 2, 2 + 6 + 5]            # n_heads, conv_b of head 0, fc1_w and fc2_b of head 1
    assert all(p.grad is None for p in frozen) and same_bits(x.grad.cpu().numpy().reshape(want["dx"].shape), want["dx"])
    assert same_bits(heads[0][0].weight.grad.cpu().numpy().reshape(16, 16), want["dconv_w0"])
    with torch.no_grad():
        assert not models._heads_take_training_path(x, heads)      # gradients disabled: the inference launch or torch
    assert not models._heads_take_training_path(x.double(), heads) and not models._heads_take_training_path(x.cpu(), heads)
    assert not models._heads_take_training_path(x[:, :15], heads)


def test_a_nan_in_one_sample_stays_in_that_samples_rows_and_reaches_every_weight_gradient(native, mods):
    _, models = mods
    case = ref.normal_case((6, 16, 9, ref.TICTACTOE), seed=14, dlogits_scale=1.0)

    def run(x):
        heads = heads_of(models, case)
        x = x.clone().requires_grad_()
        logits = models.conv_heads(x, heads)
        sum((t * t).sum() for t in logits).backward()
        params = [p for conv, fc, _ in heads for p in (conv.weight, conv.bias, fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias)]
        return [t.detach().cpu().numpy() for t in logits], x.grad.cpu().numpy(), [p.grad.cpu().numpy() for p in params]

    clean = run(board(case, 3))
    poisoned = board(case, 3).clone()
    poisoned[4, 7, 1, 1] = float("nan")
    logits, dx, grads = run(poisoned)
    others = [0, 1, 2, 3, 5]
    for got, base in zip(logits, clean[0]):
        assert np.isnan(got[4]).all() and same_bits(got[others], base[others])
    assert np.isnan(dx[4]).all() and same_bits(dx[others], clean[1][others])
    assert all(np.isnan(g).any() for g in grads)
    for g in (grads[1], grads[3], grads[4], grads[5], grads[7], grads[9], grads[10], grads[11]):   # biases and fc2: every entry
        assert np.isnan(g).all()


def test_inference_after_flagged_training_equals_an_unflagged_twins(native, mods):
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=2)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", native_heads=True)
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
def test_one_training_step_with_the_heads_and_with_all_three_flags_vs_float64(native, mods):
    """The construction of test_gpu_conv_train's whole step: the TicTacToe residual config with 5 unrolled steps, B = 8, one
    update_weights with Trainer(native_heads=True), one with native_conv and native_epilogue as well and one with none (the
    library); every parameter gradient and every batch norm's running statistics of both flagged ways against the same model
    in float64 on the CPU, per tensor native error <= 4 max(library error, 4 u max|x64|)."""
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    from test_gpu_unroll_loss import _scalar_to_support64
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=5)
    batch = make_batch(config, 8, seed=17)
    ways = {"heads": dict(native_heads=True),
            "heads+conv+epilogue": dict(native_heads=True, native_conv=True, native_epilogue=True), "library": {}}
    runs = {}
    for name, flags in ways.items():
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **flags)
        assert [conv.native_training for conv, _ in trainer.model.training_heads()] == [bool(flags)] * 3
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
    assert set(exact) == set(runs["heads"]) == set(runs["heads+conv+epilogue"]) == set(runs["library"]) and len(exact) == 58
    for way in ("heads", "heads+conv+epilogue"):
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
    """Trainer(graph=True, native_heads=True), built from a checkpoint that an unflagged eager trainer wrote after three steps,
    over four steps with a decaying learning rate and a batch that changes between replays: it follows the eager flagged
    trainer resumed from the same checkpoint within 1e-5 on the weights (the tolerance, and the reason for not starting from
    fresh weights, of the epilogue's test of the same name)."""
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
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", graph=graph, native_heads=True)
        assert trainer.training_step == 3 and all(conv.native_training for conv, _ in trainer.model.training_heads())
        runs.append(follow(trainer, batches[3:]))
        assert trainer.training_step == 7
    assert_follows(runs[0], runs[1], "resumed, graphed vs eager, both native_heads")
