"""The backward of the hidden state's min-max rescale in training (csrc/rescale_train.h, include/mztrain.h mztrain_rescale_*)
without a GPU, through the host entry on host arrays.

The float64 restatement of the rule (tests/rescale_train_reference.run64) is first held to torch's float64 expression with
autograd on every shape and data kind of the GPU list.  The host entry is then held to the restatement as the header states it
(float32 up to y, float64 after: run_rule) bit for bit on all of them, and EXACTLY to run64 and to torch's float64 on integer
cases built so that every quotient is dyadic; on directed cases; five deliberate defects of the rule are each seen on a named
case; the header as a stand-alone program under the address and undefined-behaviour sanitizers gives the entry's bits; the plan
at its edges; every refusal of the query, the entries and the Trainer; the struct against a C program; and the switch left off."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import rescale_train_reference as ref
from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
IDS = [ref.shape_id(s) for s in ref.SHAPES]


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


@pytest.fixture(scope="module")
def models(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_the_float64_restatement_is_torch_in_float64(models, shape, kind):
    """Within 1e-12 of the larger of max|dx| and max|g / s|: dx is a sum of terms of the size of g / s that cancel -- to
    zero for P <= 2 -- so the size of dx alone says nothing about the rounding on the way."""
    case = ref.make_case(shape, kind, seed=3)
    mine = ref.run64(case)
    _, theirs = ref.run_torch(models, case, torch.float64)
    scale = max(float(np.abs(theirs).max()), ref.terms(case))
    assert mine.shape == theirs.shape and float(np.abs(mine - theirs).max()) <= 1e-12 * scale


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_the_host_entry_gives_the_rules_bits(native, shape, kind):
    """The header's operations restated in numpy -- float32 up to y, float64 sums in ascending order, one rounding -- give
    the host entry's bits, and both stay within float32's rounding of the float64 restatement: 4 u max|g / s| for the
    float32 y and span, and the last rounding."""
    case = ref.make_case(shape, kind, seed=5)
    got = ref.run_host_entry(native, case)
    assert same_bits(got, ref.run_rule(case))
    exact = ref.run64(case)
    span = case["x"].astype(np.float64).max(axis=1) - case["x"].astype(np.float64).min(axis=1)
    if kind not in ("span5e-6", "span2e-5") and not ((span > 0) & (span < 1e-4)).any():
        # (a span of a few float32 ulps of x is itself off by a sizeable fraction: those kinds are held to the bits alone)
        scale = max(float(np.abs(exact).max()), ref.terms(case))
        assert float(np.abs(got - exact).max()) <= 8 * shape[1] * ref.U * scale


@pytest.mark.parametrize("shape", ref.INTEGER_SHAPES, ids=[ref.shape_id(s) for s in ref.INTEGER_SHAPES])
def test_the_host_entry_is_exact_on_integers(native, models, shape):
    case = ref.integer_case(shape, seed=7)
    assert ref.integer_bound(case) < 2 ** 24
    got = ref.run_host_entry(native, case).astype(np.float64)
    exact = ref.run64(case)
    _, theirs = ref.run_torch(models, case, torch.float64)
    assert np.array_equal(got, exact) and np.array_equal(got, theirs)


def test_the_directed_cases(native, models):
    cases = ref.directed_cases()
    got = {name: ref.run_host_entry(native, case) for name, case in cases.items()}
    for name, case in cases.items():
        assert same_bits(got[name], ref.run_rule(case)), name
    assert not got["a single position"].any() and not np.signbit(got["a single position"]).any()     # exactly +0
    # a constant plane: s = 1e-5f, y = 0, every position at both extremes: dx_p = (g_p - mean(g)) / s
    case = cases["a constant plane"]
    s = np.float64(np.float32(1e-5))
    want = (case["g"].astype(np.float64) - case["g"].astype(np.float64).mean()) / s
    assert np.allclose(got["a constant plane"], want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    assert np.abs(got["a constant plane"]).max() > 1e4
    # all but one at the minimum: the eight zeros share dlo, the maximum takes dhi alone and comes out at zero
    case = cases["every position at the minimum but one"]
    g, x = case["g"][0].astype(np.float64), case["x"][0].astype(np.float64)
    s0, s1 = g.sum(), g[4]
    want = g / 2.5 + np.where(x == 0, -(s0 - s1) / 2.5 / 8, -s1 / 2.5)
    assert np.allclose(got["every position at the minimum but one"][0], want, rtol=1e-6, atol=1e-7)
    assert abs(got["every position at the minimum but one"][0, 4]) <= 1e-7
    # -0.0 and +0.0 are one minimum of four positions; torch's float64 counts them so too
    case = cases["both zeros as tied minima"]
    _, theirs = ref.run_torch(models, case, torch.float64)
    assert np.allclose(got["both zeros as tied minima"], theirs, rtol=1e-6, atol=1e-6)
    swapped = {"x": np.abs(case["x"]), "g": case["g"]}
    assert same_bits(ref.run_host_entry(native, swapped), got["both zeros as tied minima"])
    # float64 sums keep what float32 sums lose; the integers make torch's float64 exact as well
    case = cases["float32 sums lose"]
    _, theirs = ref.run_torch(models, case, torch.float64)
    assert np.array_equal(got["float32 sums lose"].astype(np.float64), theirs) and got["float32 sums lose"][0, 0] == 2.0 ** 23
    assert ref.run_rule(case, defect="sums in float32")[0, 0] == 2.0 ** 23 + 2


@pytest.mark.parametrize("defect,where", sorted(ref.DEFECTS.items()))
def test_a_defect_of_the_rule_is_seen_on_its_case(native, defect, where):
    """The host entry gives the sound rule's bits and leaves the broken one by 1e-2 of the largest term at least -- on the
    integers of the float32 sums' case by the 2 that S0 loses."""
    case = ref.directed_cases()[where] if where in ref.directed_cases() else ref.make_case((12, 9), where, seed=9)
    got, sound, broken = ref.run_host_entry(native, case), ref.run_rule(case), ref.run_rule(case, defect=defect)
    assert same_bits(got, sound)
    least = 2.0 if defect == "sums in float32" else 1e-2 * ref.terms(case)
    assert float(np.abs(got.astype(np.float64) - broken).max()) >= least


def test_a_nan_stays_in_its_plane(native):
    case = ref.make_case((6, 9), "relu", seed=11)
    clean = ref.run_host_entry(native, case)
    case["x"][2, 4] = np.nan
    got = ref.run_host_entry(native, case)
    others = [0, 1, 3, 4, 5]
    assert np.isnan(got[2]).all() and same_bits(got[others], clean[others])
    case = ref.make_case((6, 9), "relu", seed=11)
    case["g"][3, 0] = np.nan                 # in the gradient: its own position and, through S0 and S1, the plane's extremes
    got = ref.run_host_entry(native, case)
    x = case["x"][3]
    reached = (x == x.min()) | (x == x.max())
    reached[0] = True
    assert np.isnan(got[3][reached]).all() and same_bits(got[3][~reached], clean[3][~reached])
    assert same_bits(got[[0, 1, 2, 4, 5]], clean[[0, 1, 2, 4, 5]])


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_the_plan_at_its_edges(lib):
    """The library's plan is the restatement's; both tiles fit a CU's LDS, the stride is odd and holds a row, every row lies
    in exactly one workgroup, a workgroup has a thread per row; small launches reach many CUs."""
    row_counts = [1, 2, 15, 16, 17, 255, 256, 257, 1024, 4095, 4096, 4097, 16 * 256 + 1, 157 * 256, 157 * 256 + 1, 158 * 256 + 1,
                  255 * 256, 255 * 256 + 1, 256 * 256 + 1, 1 << 20, (1 << 31) // 128 - 1]
    for row_len in (1, 2, 9, 36, 42, 64, 121, 127, 128):
        for rows in row_counts:
            rc, got = ref.library_plan(lib, rows, row_len)
            grid, block, per_group, stride, lds = got
            assert rc == 0 and got == ref.plan(rows, row_len), (rows, row_len, got)
            assert lds == 2 * 4 * per_group * stride <= ref.LDS_BYTES
            assert stride % 2 == 1 and row_len <= stride <= row_len + 1
            assert 1 <= per_group <= block == 256
            assert (grid - 1) * per_group < rows <= grid * per_group
    assert ref.library_plan(lib, 64 * 16, 9)[1][:3] == (64, 256, 16)          # TicTacToe at batch 64: 64 workgroups, not 4
    assert ref.library_plan(lib, 64 * 64, 42)[1][:3] == (256, 256, 16)        # Connect4 at batch 64
    assert ref.library_plan(lib, 1 << 20, 128)[1][2:] == (158, 129, 2 * 4 * 158 * 129)      # all of a CU's LDS but 784 bytes
    assert ref.library_plan(lib, 1 << 20, 9)[1][2] == 256
    for shape in ref.LARGE_SHAPES:
        assert ref.plan(*shape)[2] in (256, 158)
    for rows, row_len in ((0, 9), (4, 0), (4, 129), ((1 << 31) // 9 + 1, 9)):
        rc, got = ref.library_plan(lib, rows, row_len)
        assert rc == -1 and got == (0, 0, 0, 0, 0)
    assert lib.mztrain_rescale_backward_plan(4, 9, None) == -1


# ---- the support query and the refusals -----------------------------------------------------------------------------------------
def test_supported(lib):
    message = lambda: (lib.mzmcts_last_error(None) or b"").decode()
    for rows, row_len in ref.SHAPES + ref.LARGE_SHAPES + [(1, 128), ((1 << 31) // 128 - 1, 128), ((1 << 31) - 1, 1)]:
        assert lib.mztrain_rescale_supported(rows, row_len) == 1, (rows, row_len)
    for args, text in [((4, 0), "row_len (H * W) must lie in [1, 128]"), ((4, 129), "row_len"), ((4, -1), "row_len"),
                       ((0, 9), "rows must be positive"), ((-5, 9), "rows must be positive"),
                       (((1 << 31) // 128, 128), "below 2^31"), ((1 << 31, 1), "below 2^31"), ((1 << 40, 9), "below 2^31")]:
        assert lib.mztrain_rescale_supported(*args) == 0, args
        assert message().startswith("mztrain_rescale_supported:") and text in message(), (args, message())


@pytest.mark.parametrize("entry", ["mztrain_rescale_backward", "mztrain_rescale_reference_backward"])
def test_refusals(native, lib, entry):
    """Decided on the arguments alone: the pointers are never followed (they point nowhere) and no device is touched."""
    reference = "reference" in entry

    def check(args, text, why):
        function = getattr(lib, entry)
        pointer = ctypes.byref(args) if args is not None else None
        rc = function(pointer) if reference else function(pointer, None)
        message = (lib.mzmcts_last_error(None) or b"").decode()
        assert rc == native.ERR_INVALID and text in message and message.startswith(entry + ":"), (why, rc, message)

    good = dict(x=0x1000, grad_out=0x2000, grad_x=0x3000, rows=32, row_len=9)
    check(None, "null args", "null args")
    for name in ("x", "grad_out", "grad_x"):
        check(ref.backward_args(native, **{**good, name: None}), "null pointer in args", name)
    for rows in (0, -1, (1 << 31) // 9 + 1):
        check(ref.backward_args(native, **{**good, "rows": rows}), "rows", rows)
    for row_len in (0, -3, 129):
        check(ref.backward_args(native, **{**good, "row_len": row_len}), "row_len", row_len)


def test_the_argument_struct_matches_its_ctypes_mirror(native, tmp_path):
    name = "mztrain_rescale_backward_args"
    fields = c_fields("mztrain.h", name)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mztrain.h"', "int main(void) {",
             f'    printf("%zu", sizeof({name}));']
    lines += [f'    printf(" %zu", offsetof({name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, *offsets = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    mirror = native.MzTrainRescaleBackwardArgs
    assert [n for n, *_ in mirror._fields_] == fields == ["x", "grad_out", "grad_x", "rows", "row_len"]
    assert ctypes.sizeof(mirror) == size and [getattr(mirror, f).offset for f in fields] == offsets


# ---- the header under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("rescale_train") / "rescale_train_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "rescale_train_check.cpp")],
                   check=True)
    return exe


@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_header_under_the_sanitizers(native, lib, program, tmp_path, kind):
    """The stand-alone program gives the host entry's bits, and the library's plan, on every shape of the list."""
    for shape in ref.SHAPES:
        case = ref.make_case(shape, kind, seed=13)
        source, result = tmp_path / "case.bin", tmp_path / "out.bin"
        with open(source, "wb") as f:
            f.write(struct.pack("<qi", *shape))
            f.write(case["x"].tobytes())
            f.write(case["g"].tobytes())
        done = subprocess.run([program, str(source), str(result)], capture_output=True, text=True)
        assert done.returncode == 0, (shape, done.stderr)
        raw = np.fromfile(result, dtype=np.uint8)
        dx = raw[:-40].view(np.float32).reshape(shape)
        assert same_bits(dx, ref.run_host_entry(native, case)), shape
        assert tuple(raw[-40:].view(np.int64)) == ref.library_plan(lib, *shape)[1], shape


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def checkpoint(game, **changes):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    for key, value in changes.items():
        setattr(config, key, value)
    return {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}, config


def test_trainer_refuses_a_fully_connected_network(pkg):
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    ckpt, config = checkpoint("cartpole")
    with pytest.raises(NotImplementedError, match="native_rescale=True.*residual networks"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_rescale=True)
    with pytest.raises(NotImplementedError, match="native_rescale=True.*residual networks"):     # before fc_step's refusals
        trainer_mod.Trainer(ckpt, config, device="cpu", native_rescale=True, fc_step=True)


def test_trainer_refuses_a_board_of_more_than_128_positions(pkg):
    """12 x 12 = 144 positions; the refusal comes before the question of where the model lives."""
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    ckpt, config = checkpoint("tictactoe", observation_shape=(3, 12, 12))
    with pytest.raises(NotImplementedError, match=r"native_rescale=True\) covers hidden-state planes of at most 128 positions.*144"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_rescale=True)


def test_trainer_refuses_a_model_off_the_gpu(pkg):
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    ckpt, config = checkpoint("tictactoe")
    with pytest.raises(NotImplementedError, match="native_rescale=True.*must be on the GPU"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_rescale=True)
    with pytest.raises(NotImplementedError, match="native_heads=True.*must be on the GPU"):       # after native_heads' refusals
        trainer_mod.Trainer(ckpt, config, device="cpu", native_rescale=True, native_heads=True)


@pytest.mark.parametrize("game,plane", [("tictactoe", 9), ("connect4", 42), ("gomoku", 121)])
def test_the_configs_hidden_planes_are_covered(pkg, lib, game, plane):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    model = models.MuZeroNetwork(config)
    assert model.hidden_plane == plane and lib.mztrain_rescale_supported(2 * config.channels, plane) == 1
    assert (2 * config.channels, plane) in ref.SHAPES


def graph_nodes(tensor):
    names, todo = [], [tensor.grad_fn]
    while todo:
        node = todo.pop()
        if node is not None:
            names.append(type(node).__name__)
            todo.extend(fn for fn, _ in node.next_functions)
    return sorted(names)


def test_the_switch_left_off_keeps_the_torch_path(pkg):
    """Off, or on for tensors that are not on the GPU: board_rescale builds the autograd graph of the torch expression --
    the same node types as the expression written out -- and gives its output and its gradient bit for bit."""
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    torch.manual_seed(2)
    model = models.MuZeroNetwork(config).train()
    assert model.native_rescale is False

    def written_out(raw):
        low, high = raw.amin(dim=(2, 3), keepdim=True), raw.amax(dim=(2, 3), keepdim=True)
        span = high - low
        span = torch.where(span < 1e-5, span + 1e-5, span)
        return (raw - low) / span

    data = torch.relu(torch.randn(4, 16, 3, 3))
    weight = torch.randn(4, 16, 3, 3)
    x0 = data.clone().requires_grad_()
    want = written_out(x0)
    (want * weight).sum().backward()
    observation = torch.rand((4,) + tuple(config.observation_shape))
    state_nodes = graph_nodes(model.representation(observation))
    for on in (False, True, False):
        assert model.native_training_rescale(on) is model and model.native_rescale is on
        x = data.clone().requires_grad_()
        assert not models._rescale_takes_training_path(x, None, on)
        got = models.board_rescale(x, native_training=on)
        assert torch.equal(got, want) and graph_nodes(got) == graph_nodes(want) and "_TrainingRescale" not in " ".join(graph_nodes(got))
        (got * weight).sum().backward()
        assert torch.equal(x.grad, x0.grad)
        state = model.representation(observation)
        assert graph_nodes(state) == state_nodes and "_TrainingRescale" not in " ".join(state_nodes)
        action = torch.randint(0, 9, (4, 1))
        next_state, _ = model.dynamics(state, action)
        assert "_TrainingRescale" not in " ".join(graph_nodes(next_state))
    assert torch.equal(models.board_rescale(data), written_out(data))             # the two-argument call of before
