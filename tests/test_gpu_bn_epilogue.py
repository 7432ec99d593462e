"""The training epilogue relu(batch_norm(x) [+ residual]) as HIP launches (csrc/bn_epilogue.hip, include/mztrain.h
mztrain_epilogue_*) on the GPU: the kernels against the host entries bit for bit between NaN guard bands on every shape of
tests/bn_epilogue_reference.SHAPES (both sides of the one switch of form, a channel kept in LDS up to 4096 values or read
again beyond); against the float64 yardstick by the project's training-step rule with torch's own float32 expression on the
GPU as the library, three special channels included; exact properties; one whole training step with and without
Trainer(native_epilogue=True) against the float64 model; and the flagged trainer captured into a hipGraph.  The ratios go
into measure_out/bn_epilogue_report.json."""
import copy
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import bn_epilogue_reference as ref
from unroll_loss_reference import torch_reference

pytestmark = pytest.mark.gpu

GUARD = 251          # floats of NaN either side of every device tensor; odd, so that no payload is 16-byte aligned
REPORT = {"kernel_vs_float64": {}, "whole_step": {}}
CASES = [(shape, with_residual) for shape in ref.SHAPES for with_residual in (False, True)]
CASE_IDS = [ref.shape_id(s) + ("-residual" if r else "") for s, r in CASES]


@pytest.fixture(scope="module")
def native(pkg):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    yield importlib.import_module("muzero-hypermodel_amd._native")
    out_dir = os.environ.get("MZ_OUT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                          "measure_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bn_epilogue_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def mods(pkg):
    return (importlib.import_module("muzero-hypermodel_amd.trainer"), importlib.import_module("muzero-hypermodel_amd.models"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Guarded:
    """A float32 device tensor of `shape` between two NaN bands (NaN itself where `values` is None)."""

    def __init__(self, shape, values=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.lo, self.hi = GUARD, GUARD + n
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


def run_device(native, case):
    """Forward and backward through the device entries on guarded tensors: the tensors of ref.run_host_entry.  Inputs must
    come back unchanged and every guard band untouched."""
    lib = native.load()
    shape = case["shape"]
    c = shape[1]
    t = {k: Guarded(case[k].shape, case[k]) for k in ("x", "gamma", "beta", "running_mean", "running_var", "dy")}
    if case["residual"] is not None:
        t["residual"] = Guarded(shape, case["residual"])
    for key in ("out", "dx"):
        t[key] = Guarded(shape)
    if case["residual"] is not None:
        t["dresidual"] = Guarded(shape)
    for key in ("mean", "invstd", "dgamma", "dbeta"):
        t[key] = Guarded((c,))
    address = lambda key: t[key].ptr() if key in t else None
    stream = torch.cuda.current_stream().cuda_stream
    args = ref.forward_args(native, shape, address("x"), address("residual"), address("gamma"), address("beta"),
                            address("running_mean"), address("running_var"), address("out"), address("mean"),
                            address("invstd"))
    rc = lib.mztrain_epilogue_forward(ctypes.byref(args), stream)
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    args = ref.backward_args(native, shape, address("dy"), address("x"), address("out"), address("gamma"), address("mean"),
                             address("invstd"), address("dx"), address("dresidual"), address("dgamma"), address("dbeta"))
    rc = lib.mztrain_epilogue_backward(ctypes.byref(args), stream)
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    torch.cuda.synchronize()
    for key, tensor in t.items():
        assert tensor.bands_untouched(), f"{key}: a guard band was written"
    for key in ("x", "gamma", "beta", "dy", "residual"):
        if key in t:
            assert same_bits(t[key].host(), case[key]), f"{key} was written"
    got = {key: t[key].host() for key in ("out", "running_mean", "running_var", "dx", "dgamma", "dbeta", "mean", "invstd")}
    got["dresidual"] = t["dresidual"].host() if "dresidual" in t else None
    return got


def assert_same(got, want, what=""):
    for key, value in want.items():
        if value is None:
            assert got[key] is None, key
        else:
            assert same_bits(got[key], value), f"{what}{key}: bits differ"


# ---- the kernels against the host entries -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,with_residual", CASES, ids=CASE_IDS)
def test_kernels_give_the_host_entries_bits(native, shape, with_residual):
    """Output, saved statistics, running statistics and all four gradients, bit for bit.  256x2x4x4 (M = 4096) is the largest
    channel kept in LDS, 241x2x1x17 (M = 4097) the smallest read again; the kernel has one workgroup per channel at every
    size, so that is its only switch."""
    case = ref.make_case(shape, with_residual)
    assert_same(run_device(native, case), ref.run_host_entry(native, case))


# ---- against float64 ------------------------------------------------------------------------------------------------------
def check_rule(native, case, label):
    got = run_device(native, case)
    exact, library = ref.run64(case), ref.run_torch(case, torch.float32, device="cuda")
    report = ref.ratios(got, library, exact)
    REPORT["kernel_vs_float64"][label] = {key: entry for key, (_, entry) in report.items()}
    top = max(report, key=lambda k: report[k][0])
    print(f"\n{label}: " + ", ".join(f"{k} {v[0]:.3f}" for k, v in report.items()))
    assert report[top][0] <= 1.0, (top, report[top][1])
    return got


@pytest.mark.parametrize("shape,with_residual", CASES, ids=CASE_IDS)
def test_kernels_meet_the_training_step_rule(native, shape, with_residual):
    check_rule(native, ref.make_case(shape, with_residual, seed=1), ref.shape_id(shape) + ("-residual" if with_residual else ""))


@pytest.mark.parametrize("special", ["constant", "offset", "zeros"])
@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
def test_kernels_meet_the_rule_on_the_special_channels(native, special, with_residual):
    """A channel of one constant (variance 0), a channel of mean 1e4 and deviation 1, and batch-norm outputs that are exactly
    0 at some elements (the mask is 0 there, as torch's)."""
    case = ref.make_case((64, 16, 3, 3), with_residual, special=special)
    got = check_rule(native, case, f"{special}{'-residual' if with_residual else ''}")
    if special == "zeros":
        zero = case["x"][:, 0] == 0
        assert zero.any() and not got["out"][:, 0][zero].any()
        if with_residual:
            assert not got["dresidual"][:, 0][zero].any()
    if special == "constant":
        assert np.isfinite(got["dx"]).all() and np.isfinite(got["out"]).all()


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def permuted(case, order):
    out = dict(case)
    for key in ("x", "dy", "residual"):
        if case[key] is not None:
            out[key] = np.ascontiguousarray(case[key][:, order])
    for key in ("gamma", "beta", "running_mean", "running_var"):
        out[key] = np.ascontiguousarray(case[key][order])
    return out


def test_permuting_channels_permutes_outputs_and_gradients(native):
    case = ref.make_case((3, 15, 3, 3), True)
    order = np.random.RandomState(4).permutation(15)
    base, moved = run_device(native, case), run_device(native, permuted(case, order))
    for key, value in base.items():
        want = value[:, order] if value.ndim == 4 else value[order]
        assert same_bits(moved[key], want), key


def test_a_nan_in_one_channel_leaves_every_other_channels_bits(native):
    case = ref.make_case((5, 4, 6, 7), True)
    poisoned = copy.deepcopy(case)
    poisoned["x"][2, 1, 3, 4] = np.nan
    base, got = run_device(native, case), run_device(native, poisoned)
    others = [0, 2, 3]
    for key, value in base.items():
        if value.ndim == 4:
            assert same_bits(got[key][:, others], value[:, others]), key
        else:
            assert same_bits(got[key][others], value[others]), key
    assert np.isnan(got["out"][:, 1]).all() and np.isnan(got["running_mean"][1])


def test_two_runs_give_the_same_bits(native):
    case = ref.make_case((130, 2, 11, 11), True)
    assert_same(run_device(native, case), run_device(native, case))


def module_of(models, case):
    c = case["shape"][1]
    bn = models.BatchNorm2d(c, eps=ref.EPS, momentum=ref.MOMENTUM).cuda()
    with torch.no_grad():
        for name, key in (("weight", "gamma"), ("bias", "beta"), ("running_mean", "running_mean"), ("running_var", "running_var")):
            getattr(bn, name).copy_(torch.from_numpy(case[key]))
    bn.native_training = True
    return bn.train()


def through_the_module(models, case, strided):
    """conv_epilogue on the switched-on batch norm and autograd's backward; `strided`: every tensor input is a
    non-contiguous view (channels-last storage; the gradient a slice of a wider tensor)."""
    bn = module_of(models, case)

    def dev(a):
        t = torch.from_numpy(a).cuda()
        if strided:
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert not t.is_contiguous()
        return t

    x = dev(case["x"]).requires_grad_()
    residual = dev(case["residual"]).requires_grad_() if case["residual"] is not None else None
    out = models.conv_epilogue(x, bn, residual)
    assert type(out.grad_fn).__name__.startswith("_TrainingEpilogue")
    dy = torch.from_numpy(case["dy"]).cuda()
    if strided:
        dy = torch.stack([dy, dy], dim=-1)[..., 0]
    out.backward(dy)
    back = lambda t: t.detach().cpu().numpy()
    assert int(bn.num_batches_tracked) == 1
    return {"out": back(out), "running_mean": back(bn.running_mean), "running_var": back(bn.running_var), "dx": back(x.grad),
            "dresidual": back(residual.grad) if residual is not None else None, "dgamma": back(bn.weight.grad),
            "dbeta": back(bn.bias.grad)}


@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
def test_non_contiguous_inputs_give_the_contiguous_bits(native, mods, with_residual):
    _, models = mods
    case = ref.make_case((5, 4, 6, 7), with_residual)
    want = ref.run_host_entry(native, case)
    del want["mean"], want["invstd"]
    assert_same(through_the_module(models, case, strided=False), want, "contiguous: ")
    assert_same(through_the_module(models, case, strided=True), want, "strided: ")


def test_gradients_nobody_needs_are_none_and_one_value_per_channel_is_torchs_error(native, mods):
    _, models = mods
    case = ref.make_case((5, 4, 6, 7), True)
    bn = module_of(models, case)
    x = torch.from_numpy(case["x"]).cuda()
    residual = torch.from_numpy(case["residual"]).cuda()
    out = models.conv_epilogue(x, bn, residual)            # only the parameters require a gradient
    out.backward(torch.from_numpy(case["dy"]).cuda())
    want = ref.run_host_entry(native, case)
    assert x.grad is None and residual.grad is None
    assert same_bits(bn.weight.grad.cpu().numpy(), want["dgamma"]) and same_bits(bn.bias.grad.cpu().numpy(), want["dbeta"])
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training, got input size"):
        models.conv_epilogue(torch.zeros(1, 4, 1, 1, device="cuda"), bn)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training, got input size"):
        torch.nn.BatchNorm2d(4).cuda().train()(torch.zeros(1, 4, 1, 1, device="cuda"))


def test_eval_after_a_native_training_forward_uses_freshly_folded_constants(native, mods):
    """The launch writes the running statistics behind their version counters: the forward drops the folded eval-mode
    scale and shift, so the next eval() forward folds again."""
    _, models = mods
    case = ref.make_case((64, 16, 3, 3), False)
    bn = module_of(models, case)
    x = torch.from_numpy(case["x"]).cuda()
    bn.eval()
    before = models.conv_epilogue(x, bn).clone()          # fills the cache from the initial statistics
    bn.train()
    models.conv_epilogue(x, bn)
    bn.eval()
    after = models.conv_epilogue(x, bn).clone()
    bn.refold()
    fresh = models.conv_epilogue(x, bn)
    assert torch.equal(after, fresh) and not torch.equal(after, before)
    scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    want = torch.relu(torch.addcmul((bn.bias - bn.running_mean * scale).view(1, -1, 1, 1), x, scale.view(1, -1, 1, 1)))
    assert float((after - want).detach().abs().max()) <= 1e-5 * float(want.detach().abs().max())


# ---- a whole step -----------------------------------------------------------------------------------------------------------
def tictactoe_setup(models, unroll, seed=3):
    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    config.num_unroll_steps = unroll
    torch.manual_seed(seed)
    model = models.MuZeroNetwork(config)
    ckpt = {"weights": copy.deepcopy(model.get_weights()), "training_step": 0, "optimizer_state": None}
    return config, ckpt


def make_batch(config, B, seed):
    K1, A = config.num_unroll_steps + 1, len(config.action_space)
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B,) + tuple(config.observation_shape), generator=g), torch.randint(0, A, (B, K1), generator=g),
            torch.randn(B, K1, generator=g) * 10, torch.randn(B, K1, generator=g),
            torch.softmax(torch.randn(B, K1, A, generator=g), dim=2), torch.rand(B, generator=g) + 0.5,
            torch.randint(1, K1 + 1, (B, K1), generator=g).float())


def test_one_training_step_with_and_without_the_flag_vs_float64(native, mods):
    """The construction of test_parameter_gradients_of_one_training_step_vs_float64: the TicTacToe residual config with 5
    unrolled steps, B = 8, one update_weights with Trainer(native_epilogue=True) and one without (the library); every
    parameter gradient and every batch norm's running statistics against the same model in float64 on the CPU, per tensor
    native error <= 4 max(library error, 4 u max|x64|).  num_batches_tracked is equal in both runs."""
    from test_gpu_unroll_loss import _scalar_to_support64
    trainer_mod, models = mods
    config, ckpt = tictactoe_setup(models, unroll=5)
    batch = make_batch(config, 8, seed=17)
    runs = {}
    for flag in (True, False):
        trainer = trainer_mod.Trainer(copy.deepcopy(ckpt), config, device="cuda", native_epilogue=flag)
        norms = [m for m in trainer.model.modules() if isinstance(m, models.BatchNorm2d)]
        assert all(getattr(m, "native_training", False) is flag for m in norms) and len(norms) >= 5
        trainer.update_weights(tuple(t.cuda() for t in batch))
        tensors = {k: p.grad.detach().double().cpu() for k, p in trainer.model.named_parameters() if p.grad is not None}
        state = trainer.model.state_dict()
        tensors.update({k: v.detach().double().cpu() for k, v in state.items() if k.endswith(("running_mean", "running_var"))})
        runs[flag] = (tensors, {k: int(v) for k, v in state.items() if k.endswith("num_batches_tracked")})
    assert runs[True][1] == runs[False][1] and max(runs[True][1].values()) == 6 and min(runs[True][1].values()) == 1
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
    exact.update({k: v.detach() for k, v in model64.state_dict().items() if k.endswith(("running_mean", "running_var"))})
    assert set(exact) == set(runs[True][0]) == set(runs[False][0]) and len(exact) >= 20
    worst = {}
    for name, x64 in exact.items():
        worst[name], entry = ref.ratio(runs[True][0][name].numpy(), runs[False][0][name].numpy(), x64.numpy())
        REPORT["whole_step"][name] = entry
    top = max(worst, key=worst.get)
    print(f"\nwhole step: {len(worst)} tensors, worst native error / allowed {worst[top]:.3f} ({top})")
    assert worst[top] <= 1.0, (top, REPORT["whole_step"][top])


# ---- capture ------------------------------------------------------------------------------------------------------------------
def follow(trainer, batches):
    out = []
    for bt in batches:
        trainer.update_lr()
        out.append(trainer.update_weights(bt))
    return out, {k: v.clone() for k, v in trainer.model.state_dict().items()}


def assert_follows(eager, graphed, what):
    (out_e, w_e), (out_g, w_g) = eager, graphed
    worst_w = max(float((w_e[k].double() - w_g[k].double()).abs().max()) for k in w_e)
    worst_p = max(float(np.abs(a[0] - b[0]).max()) for a, b in zip(out_e, out_g))
    worst_l = max(abs(x - y) / abs(x) for a, b in zip(out_e, out_g) for x, y in zip(a[1:], b[1:]))
    print(f"\n{what}: weights {worst_w:.2e}, priorities {worst_p:.2e}, losses {worst_l:.2e} (rel.)")
    assert worst_w <= 1e-5 and worst_l <= 1e-5 and worst_p <= 2e-3


def test_graphed_flagged_trainer_resumes_from_an_unflagged_checkpoint_and_follows_the_eager_one(native, mods):
    """Trainer(graph=True, native_epilogue=True), built from a checkpoint that an unflagged eager trainer wrote after three
    steps, over four steps with a decaying learning rate and a batch that changes between replays: it follows the eager
    flagged trainer resumed from the same checkpoint within the tolerances of test_graphed_step_equals_eager_step (1e-5 on
    weights and losses, 2e-3 on priorities); batch-norm statistics and num_batches_tracked are part of the compared state.

    The four steps start from a checkpoint and not from fresh weights because of Adam, not of the capture.  From zero
    moments Adam's first updates are lr * g / (|g| + eps) whatever the size of g, so elements whose gradient is rounding
    noise move by a sizeable part of lr, and capturable Adam (the graphed trainer's) and eager Adam round differently.  On
    this network from fresh weights the graphed trainer of the parent commit, without the flag, is 2.05e-4 from its own
    eager twin after four steps (with the flag: 2.05e-4 in one run, 5.4e-4 in another process), while two eager runs agree
    bit for bit; both figures measured on the MI355X.  With the moments three steps old the same comparison is at 4e-7."""
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
        trainer = trainer_mod.Trainer(copy.deepcopy(saved), config, device="cuda", graph=graph, native_epilogue=True)
        assert trainer.training_step == 3
        lrs = []
        out = []
        for bt in batches[3:]:
            trainer.update_lr()
            lrs.append(trainer._lr_host)
            out.append(trainer.update_weights(bt))
        runs.append((out, {k: v.clone() for k, v in trainer.model.state_dict().items()}))
        assert trainer.training_step == 7 and lrs == sorted(lrs, reverse=True) and len(set(lrs)) == 4
        tracked = [int(v) for k, v in runs[-1][1].items() if k.endswith("num_batches_tracked")]
        assert max(tracked) == 7 * 6 and min(tracked) == 7
    assert_follows(runs[0], runs[1], "resumed, graphed vs eager, both flagged")


def test_a_captured_epilogue_replays_the_eager_bits(native, mods):
    """Forward and backward of one epilogue captured into a hipGraph and replayed on new inputs: the host entries' bits, the
    running statistics advanced by the replay."""
    _, models = mods
    case = ref.make_case((64, 16, 3, 3), True)
    other = ref.make_case((64, 16, 3, 3), True, seed=5)
    bn = module_of(models, case)
    x = torch.from_numpy(other["x"]).cuda().requires_grad_()
    residual = torch.from_numpy(other["residual"]).cuda().requires_grad_()
    dy = torch.from_numpy(other["dy"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        models.conv_epilogue(x, bn, residual).backward(dy)          # warm-up on a side stream, undone below
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = residual.grad = bn.weight.grad = bn.bias.grad = None
    with torch.cuda.graph(graph):
        out = models.conv_epilogue(x, bn, residual)
        out.backward(dy)
    with torch.no_grad():
        for tensor, key in ((x, "x"), (residual, "residual"), (dy, "dy"), (bn.running_mean, "running_mean"),
                            (bn.running_var, "running_var")):
            tensor.copy_(torch.from_numpy(case[key]))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.run_host_entry(native, case)
    back = lambda t: t.detach().cpu().numpy()
    got = {"out": back(out), "running_mean": back(bn.running_mean), "running_var": back(bn.running_var), "dx": back(x.grad),
           "dresidual": back(residual.grad), "dgamma": back(bn.weight.grad), "dbeta": back(bn.bias.grad)}
    del want["mean"], want["invstd"]
    assert_same(got, want, "replayed: ")
