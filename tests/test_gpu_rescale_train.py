"""The backward of the hidden state's min-max rescale in training as one HIP launch (csrc/rescale_train.hip, include/mztrain.h
mztrain_rescale_*) on the GPU: the launch against the host entry, bit for bit, between NaN guard bands on every shape and data
kind of tests/rescale_train_reference -- the shapes at which the plan's other limits decide included --, twice and captured;
exactly torch's float64 on the integer cases; against float64 by the project's training-step rule with torch's own float32
expression and autograd on the GPU as the library; the autograd Function's behaviour; one whole training step against the
float64 model; and the flagged trainer captured into a hipGraph.  The ratios go into measure_out/rescale_train_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import rescale_train_reference as ref
from bn_epilogue_reference import ratio
from unroll_loss_reference import torch_reference

pytestmark = pytest.mark.gpu

GUARD = 251          # floats of NaN either side of a device tensor; odd: the launch assumes no alignment beyond a float's
REPORT = {"kernel_vs_float64": {}, "whole_step": {}}
ALL_SHAPES = ref.SHAPES + ref.LARGE_SHAPES
IDS = [ref.shape_id(s) for s in ALL_SHAPES]


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "rescale_train_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Launch:
    """The launch of one shape on device tensors between NaN bands; queue() puts it on the current stream."""

    def __init__(self, native, shape):
        self.native, self.lib, self.shape = native, native.load(), shape
        n = shape[0] * shape[1]
        self.buf = {key: torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda") for key in ("x", "g", "dx")}
        self.view = {key: buf[GUARD:GUARD + n].view(shape) for key, buf in self.buf.items()}

    def load(self, case):
        with torch.no_grad():
            for key in ("x", "g"):
                self.view[key].copy_(torch.from_numpy(case[key]))

    def queue(self):
        args = ref.backward_args(self.native, self.view["x"].data_ptr(), self.view["g"].data_ptr(), self.view["dx"].data_ptr(),
                                 *self.shape)
        rc = self.lib.mztrain_rescale_backward(ctypes.byref(args), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, self.lib.mzmcts_last_error(None))

    def result(self, case):
        torch.cuda.synchronize()
        for key, buf in self.buf.items():
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), f"{key}: a guard band was written"
        for key in ("x", "g"):
            assert same_bits(self.view[key].cpu().numpy(), case[key]), f"{key} was written"
        return self.view["dx"].cpu().numpy()


def run_device(native, case, launch=None):
    launch = launch or Launch(native, case["x"].shape)
    launch.load(case)
    launch.view["dx"].fill_(float("nan"))
    launch.queue()
    return launch.result(case)


# ---- bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_the_launch_gives_the_host_entrys_bits(native, shape):
    """Every data kind (two of them on the two large shapes, which are there for the plan's limits); dx is NaN before each
    launch, so every entry is seen to be written; a second launch gives the first one's bits."""
    launch = Launch(native, shape)
    for kind in ref.KINDS if shape in ref.SHAPES else ("relu", "span2e-5"):
        case = ref.make_case(shape, kind, seed=1)
        first = run_device(native, case, launch)
        assert same_bits(first, ref.run_host_entry(native, case)), kind
        assert same_bits(run_device(native, case, launch), first), f"{kind}, second run"


@pytest.mark.parametrize("shape", ref.INTEGER_SHAPES, ids=[ref.shape_id(s) for s in ref.INTEGER_SHAPES])
def test_the_launch_is_exact_on_integers(native, mods, shape):
    case = ref.integer_case(shape, seed=7)
    assert ref.integer_bound(case) < 2 ** 24
    _, theirs = ref.run_torch(mods[1], case, torch.float64)
    assert np.array_equal(run_device(native, case).astype(np.float64), theirs)


def test_the_directed_cases_give_the_host_entrys_bits(native):
    for name, case in ref.directed_cases().items():
        assert same_bits(run_device(native, case), ref.run_host_entry(native, case)), name


def test_grad_x_may_be_grad_out(native):
    case = ref.make_case((37, 42), "relu", seed=2)
    want = run_device(native, case)
    x, g = (torch.from_numpy(case[key]).cuda() for key in ("x", "g"))
    args = ref.backward_args(native, x.data_ptr(), g.data_ptr(), g.data_ptr(), 37, 42)
    assert native.load().mztrain_rescale_backward(ctypes.byref(args), torch.cuda.current_stream().cuda_stream) == 0
    assert same_bits(g.cpu().numpy(), want)


CAPTURED = [(16, 9), (17, 42), (2 * 128, 121), (5, 128), (37, 1)]


@pytest.mark.parametrize("shape", CAPTURED, ids=[ref.shape_id(s) for s in CAPTURED])
def test_a_captured_launch_replays_the_eager_bits(native, shape):
    """Captured into a hipGraph after one eager call on one set of inputs and replayed on another: the bits of an eager run
    on the second set."""
    first, second = ref.make_case(shape, "relu", seed=2), ref.make_case(shape, "normal", seed=3)
    eager = run_device(native, second)
    launch = Launch(native, shape)
    launch.load(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch.queue()                                            # the eager call, on a side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch.queue()
    launch.load(second)
    launch.view["dx"].fill_(float("nan"))
    graph.replay()
    assert same_bits(launch.result(second), eager)


# ---- against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=[ref.shape_id(s) for s in ref.SHAPES])
def test_the_launch_meets_the_training_step_rule(native, mods, shape):
    """native error <= 4 max(library error, 4 * 2^-24 max|g_p / s|): the library is torch's float32 expression with autograd
    on the GPU, both errors are measured against torch's float64 expression with autograd.  The floor is not max|dx|: dx is
    a sum of terms of the size of g / s that cancel, for P <= 2 to zero."""
    worst = {}
    for kind in ref.KINDS:
        case = ref.make_case(shape, kind, seed=7)
        got = run_device(native, case)
        _, library = ref.run_torch(mods[1], case, torch.float32, "cuda")
        _, exact = ref.run_torch(mods[1], case, torch.float64)
        worst[kind], REPORT["kernel_vs_float64"][f"{ref.shape_id(shape)} {kind}"] = ratio(got, library, exact, scale=ref.terms(case))
    top = max(worst, key=worst.get)
    print(f"\n{ref.shape_id(shape)}: worst {top} {worst[top]:.3f}")
    assert worst[top] <= 1.0, (top, REPORT["kernel_vs_float64"][f"{ref.shape_id(shape)} {top}"])


# ---- the autograd Function ---------------------------------------------------------------------------------------------------------
def board(array, height):
    rows, p = array.shape
    return torch.from_numpy(array).cuda().view(rows // 4, 4, height, p // height)


def through_the_function(models, raw, grad):
    raw = raw.requires_grad_()
    assert models._rescale_takes_training_path(raw, None, True)
    out = models.board_rescale(raw, native_training=True)
    assert type(out.grad_fn).__name__.startswith("_TrainingRescale")
    out.backward(grad)
    return out.detach().cpu().numpy().reshape(-1, raw.shape[2] * raw.shape[3]), raw.grad.cpu().numpy().reshape(-1, raw.shape[2] * raw.shape[3])


def test_the_functions_forward_is_the_inference_launch_and_its_backward_the_new_one(native, mods):
    _, models = mods
    case = ref.make_case((24, 42), "relu", seed=11)
    with torch.no_grad():
        inference = models.board_rescale(board(case["x"], 6)).cpu().numpy().reshape(24, 42)
    torch_y, _ = ref.run_torch(models, case, torch.float32, "cuda")
    out, dx = through_the_function(models, board(case["x"], 6), board(case["g"], 6))
    assert same_bits(out, inference) and same_bits(out, torch_y) and same_bits(dx, run_device(native, case))


def test_non_contiguous_inputs_and_gradients_give_the_contiguous_bits(native, mods):
    _, models = mods
    case = ref.make_case((24, 9), "relu", seed=12)
    want = run_device(native, case)
    strided = lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    raw, grad = strided(board(case["x"], 3)), strided(board(case["g"], 3))
    assert not raw.is_contiguous() and not grad.is_contiguous()
    assert same_bits(through_the_function(models, raw, board(case["g"], 3))[1], want)
    assert same_bits(through_the_function(models, board(case["x"], 3), grad)[1], want)
    assert same_bits(through_the_function(models, strided(board(case["x"], 3)), grad)[1], want)
    wide = torch.cat([board(case["x"], 3).reshape(-1)[:3], board(case["x"], 3).reshape(-1)])
    view = wide[3:].view(6, 4, 3, 3)                               # starts 12 bytes into its storage
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert same_bits(through_the_function(models, view, board(case["g"], 3))[1], want)


def test_a_raw_that_needs_no_gradient_launches_nothing(native, mods):
    _, models = mods
    lib = native.load()
    case = ref.make_case((24, 9), "relu", seed=13)
    calls = []
    original = lib.mztrain_rescale_backward

    def counting(*args):
        calls.append(args)
        return original(*args)

    lib.mztrain_rescale_backward = counting
    try:
        raw = board(case["x"], 3)
        assert not models._rescale_takes_training_path(raw, None, True)
        weight = torch.ones(6, 4, 3, 3, device="cuda", requires_grad=True)
        out = models.board_rescale(raw, native_training=True)
        assert out.grad_fn is None
        (out * weight).sum().backward()
        direct = models._TrainingRescale.apply(raw)
        assert direct.grad_fn is None and not direct.requires_grad and torch.equal(direct, out)
        ctx = types.SimpleNamespace(needs_input_grad=(False,), saved_tensors=(raw,))
        assert models._TrainingRescale.backward(ctx, board(case["g"], 3)) is None
        assert calls == []
        with torch.no_grad():                                      # gradients disabled, other dtypes and devices, an `out`
            assert not models._rescale_takes_training_path(raw.clone().requires_grad_(), None, True)
        wanted = raw.clone().requires_grad_()
        assert not models._rescale_takes_training_path(wanted.double(), None, True)
        assert not models._rescale_takes_training_path(wanted.cpu(), None, True)
        assert not models._rescale_takes_training_path(wanted, torch.empty_like(raw), True)
        assert not models._rescale_takes_training_path(wanted, None, False)
        assert not models._rescale_takes_training_path(torch.zeros(2, 4, 12, 12, device="cuda", requires_grad=True), None, True)
        through_the_function(models, wanted, board(case["g"], 3))
        assert len(calls) == 1
    finally:
        lib.mztrain_rescale_backward = original


def test_a_nan_in_one_plane_stays_in_that_plane(native, mods):
    _, models = mods
    case = ref.make_case((24, 9), "relu", seed=14)
    clean_out, clean_dx = through_the_function(models, board(case["x"], 3), board(case["g"], 3))
    case["x"][13, 5] = np.nan
    out, dx = through_the_function(models, board(case["x"], 3), board(case["g"], 3))
    others = [r for r in range(24) if r != 13]
    assert np.isnan(out[13]).all() and np.isnan(dx[13]).all()
    assert same_bits(out[others], clean_out[others]) and same_bits(dx[others], clean_dx[others])


def test_inference_after_flagged_training_equals_an_unflagged_twins(native, mods):
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=2)
    trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", native_rescale=True)
    assert trainer.model.native_rescale is True
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


# ---- a whole step -------------------------------------------------------------------------------------------------------------------
ALL_FOUR = dict(native_rescale=True, native_heads=True, native_conv=True, native_epilogue=True)


def test_one_training_step_with_the_rescale_and_with_all_four_flags_vs_float64(native, mods):
    """The construction of test_gpu_head_train's whole step: the TicTacToe residual config with 5 unrolled steps, B = 8, one
    update_weights with Trainer(native_rescale=True), one with the three earlier flags as well and one with none (the
    library); every parameter gradient and every batch norm's running statistics of both flagged ways against the same model
    in float64 on the CPU, per tensor native error <= 4 max(library error, 4 u max|x64|).  The flagged steps run six
    _TrainingRescale nodes each."""
    from test_gpu_bn_epilogue import make_batch, tictactoe_setup
    from test_gpu_unroll_loss import _scalar_to_support64
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=5)
    batch = make_batch(config, 8, seed=17)
    ways = {"rescale": dict(native_rescale=True), "all four": ALL_FOUR, "library": {}}
    runs, launches = {}, {}
    lib = native.load()
    original = lib.mztrain_rescale_backward
    for name, flags in ways.items():
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", **flags)
        assert trainer.model.native_rescale is bool(flags)
        calls = []
        lib.mztrain_rescale_backward = lambda *args, calls=calls: calls.append(1) or original(*args)
        try:
            trainer.update_weights(tuple(t.cuda() for t in batch))
        finally:
            lib.mztrain_rescale_backward = original
        launches[name] = len(calls)
        tensors = {k: p.grad.detach().double().cpu() for k, p in trainer.model.named_parameters() if p.grad is not None}
        state = trainer.model.state_dict()
        tensors.update({k: v.detach().double().cpu() for k, v in state.items() if k.endswith(("running_mean", "running_var"))})
        runs[name] = tensors
    assert launches == {"rescale": 6, "all four": 6, "library": 0}
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
    assert set(exact) == set(runs["rescale"]) == set(runs["all four"]) == set(runs["library"]) and len(exact) == 58
    for way in ("rescale", "all four"):
        worst = {}
        REPORT["whole_step"][way] = {}
        for name, x64 in exact.items():
            worst[name], REPORT["whole_step"][way][name] = ratio(runs[way][name].numpy(), runs["library"][name].numpy(),
                                                                 x64.numpy())
        top = max(worst, key=worst.get)
        print(f"\nwhole step, {way}: {len(worst)} tensors, worst native error / allowed {worst[top]:.3f} ({top})")
        assert worst[top] <= 1.0, (way, top, REPORT["whole_step"][way][top])


# ---- capture --------------------------------------------------------------------------------------------------------------------------
def test_graphed_flagged_trainer_resumes_from_an_unflagged_checkpoint_and_follows_the_eager_one(native, mods):
    """Trainer(graph=True, native_rescale=True), built from a checkpoint that an unflagged eager trainer wrote after three
    steps, over four steps with a decaying learning rate and a batch that changes between replays: it follows the eager
    flagged trainer resumed from the same checkpoint within 1e-5 on the weights (the tolerance, and the reason for not
    starting from fresh weights, of the epilogue's test of the same name)."""
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
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", graph=graph, native_rescale=True)
        assert trainer.training_step == 3 and trainer.model.native_rescale is True
        runs.append(follow(trainer, batches[3:]))
        assert trainer.training_step == 7
    assert_follows(runs[0], runs[1], "resumed, graphed vs eager, both native_rescale")
