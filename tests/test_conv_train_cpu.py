"""The training convolutions (csrc/conv_train.h, include/mztrain.h mztrain_conv_*) without a GPU, through the host entries on
host arrays.

The yardstick (tests/conv_train_reference.py, float64 numpy) is first held to torch's float64 conv2d with autograd (1e-12) on
every shape of the GPU list, and five deliberate defects of it are each seen on a named tensor.  The host entries are then
held to the yardstick EXACTLY on integer data, where float32 is exact whatever the order of the sums, together with the
adjoint identities; the slice fold on data built so that a float32 fold loses what a float64 fold keeps; the packings against
numpy; the header as a stand-alone program under the address and undefined-behaviour sanitizers, which must give the entries'
bits; the weight gradient's launch plan at its edges; every refusal; the structs against a C program; the Trainer's three
refusals, and the switch left off."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import conv_train_reference as ref
from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
IDS = ["B{}-{}to{}-{}x{}-dx{}".format(*s) for s in ref.SHAPES]


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


@pytest.fixture(scope="module")
def lib(native):
    return native.load()


def torch64(x, w, dy):
    """(y, dx over ALL input planes, dw) of torch's conv2d and its autograd in float64 on the CPU."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xt, wt, padding=1)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy()


def test_the_slice_length_is_the_headers(native, lib):
    assert lib.mztrain_conv_slice() == native.CONV_SLICE == 64


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_the_float64_yardstick_is_torch_in_float64(shape):
    x, w, dy = ref.normal_case(shape, seed=3, dy_scale=1.0)
    dx_planes = shape[5]
    y, dx, dw = torch64(x, w, dy)
    mine = {"y": (ref.forward(x, w), y), "dw": (ref.wgrad_exact(x, dy), dw)}
    if dx_planes:
        mine["dx"] = (ref.dgrad(dy, w, dx_planes), dx[:, :dx_planes])
    for key, (got, want) in mine.items():
        scale = max(1.0, float(np.abs(want).max()))
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-12 * scale, key


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_the_host_entries_are_exact_on_integers(native, lib, shape):
    """x in [-3, 3], w and dy in [-2, 2]: every partial sum stays below 2^24, so float32 is exact and the entries equal the
    float64 yardstick, and torch's float64 autograd, exactly; the adjoint identities hold in integers."""
    x, w, dy = ref.integer_case(shape, seed=5)
    dx_planes = shape[5]
    y, dw = ref.host_forward(native, lib, x, w), ref.host_wgrad(native, lib, x, dy)
    ty, tdx, tdw = torch64(x, w, dy)
    assert np.array_equal(y, ref.forward(x, w)) and np.array_equal(y, ty)
    assert np.array_equal(dw, ref.wgrad(x, dy, native.CONV_SLICE)) and np.array_equal(dw, tdw)
    assert not np.signbit(y[y == 0]).any()                       # acc * 1 + 0: no -0 comes out
    inner = int((y.astype(np.int64) * dy.astype(np.int64)).sum())
    assert inner == int((w.astype(np.int64) * dw.astype(np.int64)).sum())
    if dx_planes:
        dx = ref.host_dgrad(native, lib, dy, w, dx_planes)
        assert dx.shape == (shape[0], dx_planes, shape[3], shape[4])
        assert np.array_equal(dx, ref.dgrad(dy, w, dx_planes)) and np.array_equal(dx, tdx[:, :dx_planes])
        if dx_planes == shape[1]:
            assert inner == int((x.astype(np.int64) * dx.astype(np.int64)).sum())


def fold_case(slice_length):
    """One product of 2^24 in slice 0 and a 1 in each of four later slices, all on dw[0][0][1][1]: a float32 fold keeps 2^24,
    the float64 fold the rule asks for gives 2^24 + 4."""
    b, p = 40, 9                                                  # 360 indices: 6 slices of 64
    x = np.zeros((b, 1, 3, 3), dtype=np.float32)
    dy = np.zeros((b, 16, 3, 3), dtype=np.float32)
    x.reshape(-1)[0], dy[0, 0].reshape(-1)[0] = 4096.0, 4096.0
    for s in range(1, 5):
        k = s * slice_length + 3
        x.reshape(b * p)[k], dy[k // p, 0].reshape(-1)[k % p] = 1.0, 1.0
    return x, dy


def test_the_slice_sums_are_folded_in_float64(native, lib):
    x, dy = fold_case(native.CONV_SLICE)
    dw = ref.host_wgrad(native, lib, x, dy)
    assert dw[0, 0, 1, 1] == 2.0 ** 24 + 4
    assert ref.wgrad(x, dy, native.CONV_SLICE, defect="fold_in_float32")[0, 0, 1, 1] == 2.0 ** 24


@pytest.mark.parametrize("defect,tensor", [("taps_not_flipped", "dx"), ("channels_not_transposed", "dx"), ("border_wraps", "y"),
                                           ("border_wraps", "dw"), ("fold_in_float32", "dw"), ("action_plane_in_dx", "dx")])
def test_a_defect_of_the_yardstick_is_seen_on_its_tensor(native, lib, defect, tensor):
    """On integer data the host entries equal the sound yardstick exactly; the broken one leaves them on the named tensor."""
    shape = (5, 17, 16, 3, 3, 16) if defect == "action_plane_in_dx" else (40, 16, 16, 3, 3, 16)
    x, w, dy = ref.integer_case(shape, seed=9)
    if defect == "fold_in_float32":                               # integers large enough for a float32 fold to round
        x, dy = fold_case(native.CONV_SLICE)
    if tensor == "y":
        got, sound, broken = ref.host_forward(native, lib, x, w), ref.forward(x, w), ref.forward(x, w, defect=defect)
    elif tensor == "dx":
        got, sound, broken = ref.host_dgrad(native, lib, dy, w, 16), ref.dgrad(dy, w, 16), ref.dgrad(dy, w, 16, defect=defect)
    else:
        got = ref.host_wgrad(native, lib, x, dy)
        sound, broken = ref.wgrad(x, dy, native.CONV_SLICE), ref.wgrad(x, dy, native.CONV_SLICE, defect=defect)
    assert np.array_equal(got, sound), (defect, tensor)
    assert broken.shape != got.shape or not np.array_equal(got, broken), (defect, tensor)
    if defect == "action_plane_in_dx":
        assert broken.shape[1] == 17 and got.shape[1] == 16 and np.abs(broken[:, 16]).max() > 0


@pytest.mark.parametrize("cin", [1, 3, 16, 17, 64, 65, 80])
@pytest.mark.parametrize("cout", [16, 64])
def test_the_packings(native, lib, cin, cout):
    """The forward packing is mzmcts_board_conv_pack's layout restated in numpy; the data-gradient packing of w is the
    forward packing of the transposed, flipped, truncated weight built in numpy."""
    rng = np.random.default_rng(cin * 100 + cout)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)

    def layout(weight):
        co, ci = weight.shape[:2]
        groups = (ci + 15) // 16
        full = np.zeros((9 * groups + 2, 4, co, 4), dtype=np.float32)              # [tap * NG + grp][kk][n][g]
        for tap in range(9):
            for c in range(ci):
                full[tap * groups + c // 16, (c % 16) // 4, :, c % 4] = weight.reshape(co, ci, 9)[:, c, tap]
        return full.reshape(-1)

    for dx_planes in (0, 16, 64):
        if dx_planes > cin:
            continue
        packed, packed_dx, affine = ref.host_pack(native, lib, w, dx_planes)
        assert np.array_equal(packed, layout(w))
        assert np.array_equal(affine, np.r_[np.ones(64, np.float32), np.zeros(64, np.float32)])
        if dx_planes:
            virtual = ref.virtual_weight(w, dx_planes)
            assert virtual.shape == (dx_planes, cout, 3, 3) and virtual[3, 5, 0, 2] == w[5, 3, 2, 0]
            assert np.array_equal(packed_dx, layout(virtual))
            assert np.array_equal(packed_dx, ref.host_pack(native, lib, virtual, 0)[0])
        else:
            assert packed_dx is None


# ---- the launch plan ----------------------------------------------------------------------------------------------------------
def plan(lib, batch, cin, cout, h, w):
    out = (ctypes.c_int64 * 5)(*([-7] * 5))
    return lib.mztrain_conv_wgrad_plan(batch, cin, cout, h, w, out), list(out)


@pytest.mark.parametrize("cin,cout,h,w", [(1, 16, 3, 3), (16, 16, 3, 3), (17, 16, 6, 6), (64, 64, 6, 7), (65, 64, 3, 3),
                                          (80, 64, 6, 7)])
def test_the_weight_gradient_plan_at_its_edges(native, lib, cin, cout, h, w):
    p = h * w
    most = lib.mztrain_conv_max_batch(cin, cout, h, w)
    assert most == (2 ** 31 - 1 - 64) // (max(cin, cout) * p)
    edges = {1, 64 // p, 64 // p + 1, 16 * 64 // p, 16 * 64 // p + 1, 32 * 64 // p + 1, 64, most}
    for batch in sorted(edges):
        rc, (grid, block, lds, slices, rounds) = plan(lib, batch, cin, cout, h, w)
        assert rc == 0, batch
        assert grid == (cout // 16) * -(-cin * 9 // 16) and block == 1024 and lds == 16 * 256 * 4
        assert slices == -(-batch * p // 64) and rounds == -(-slices // 16)
        assert lds <= 160 * 1024 and block <= 1024 and 0 < grid < 2 ** 31
    for batch in (0, -1, most + 1):
        assert plan(lib, batch, cin, cout, h, w) == (native.ERR_INVALID, [0] * 5)
    for bad in ((0, cout, h, w), (81, cout, h, w), (cin, 32, h, w), (cin, cout, 11, 11), (cin, cout, 7, 6), (49, 16, 3, 3)):
        assert plan(lib, 4, *bad)[0] == native.ERR_INVALID and lib.mztrain_conv_max_batch(*bad) == -1


def test_supported(lib):
    for cin, cout, h, w, need, want in [(16, 16, 3, 3, 16, 1), (16, 16, 3, 3, 0, 1), (17, 16, 3, 3, 16, 1), (17, 16, 3, 3, 17, 0),
                                        (65, 64, 6, 7, 64, 1), (65, 64, 6, 7, 65, 0), (65, 64, 6, 7, 16, 1), (16, 16, 6, 6, 64, 0),
                                        (3, 16, 3, 3, 3, 0), (3, 16, 3, 3, 0, 1), (80, 64, 6, 6, 64, 1), (81, 64, 6, 6, 0, 0),
                                        (16, 32, 3, 3, 0, 0), (128, 128, 11, 11, 0, 0), (16, 16, 3, 3, -16, 0),
                                        # 16 output channels: the workgroup's planes fit LDS up to 48 / 32 / 64 input channels
                                        (48, 16, 3, 3, 16, 1), (49, 16, 3, 3, 0, 0), (32, 16, 6, 6, 16, 1), (33, 16, 6, 6, 0, 0),
                                        (64, 16, 6, 7, 64, 1), (64, 16, 6, 7, 16, 1), (65, 16, 6, 7, 0, 0),
                                        # ... and so does the data gradient 64 -> 16
                                        (65, 64, 3, 3, 16, 0), (65, 64, 6, 6, 16, 0), (80, 64, 3, 3, 64, 1)]:
        assert lib.mztrain_conv_supported(cin, cout, h, w, need) == want, (cin, cout, h, w, need)
        if want:
            assert lib.mzmcts_board_conv_supported(cin, cout, h, w)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def good(native, entry, **over):
    shape = dict(batch=4, cin=17, cout=16, height=3, width=3)
    if "pack" in entry:
        fields = dict(weight=0x1000, packed=0x2000, packed_dx=0x3000, affine=0x4000, cin=17, cout=16, dx_planes=16)
        cls = native.MzTrainConvPackArgs
    elif "forward" in entry:
        fields = dict(x=0x1000, packed=0x2000, affine=0x3000, weight=0x4000, y=0x5000, **shape)
        cls = native.MzTrainConvForwardArgs
    elif "dgrad" in entry:
        fields = dict(dy=0x1000, packed_dx=0x2000, affine=0x3000, weight=0x4000, dx=0x5000, dx_planes=16, **shape)
        cls = native.MzTrainConvDgradArgs
    else:
        fields = dict(x=0x1000, dy=0x2000, dw=0x3000, **shape)
        cls = native.MzTrainConvWgradArgs
    fields.update(over)
    return cls(**fields)


ENTRIES = ["mztrain_conv_pack", "mztrain_conv_forward", "mztrain_conv_dgrad", "mztrain_conv_wgrad",
           "mztrain_conv_reference_pack", "mztrain_conv_reference_forward", "mztrain_conv_reference_dgrad",
           "mztrain_conv_reference_wgrad"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals(native, lib, entry):
    """Decided on the arguments alone: the pointers are never followed (they point nowhere) and no device is touched."""
    reference = "reference" in entry
    kind = entry.rsplit("_", 1)[1]

    def check(args, text, why):
        function = getattr(lib, entry)
        pointer = ctypes.byref(args) if args is not None else None
        rc = function(pointer) if reference else function(pointer, None)
        message = (lib.mzmcts_last_error(None) or b"").decode()
        assert rc == native.ERR_INVALID and text in message and message.startswith(entry + ":"), (why, rc, message)

    check(None, "null args", "null args")
    required = {"pack": ("weight", "packed", "affine"),
                "forward": ("x", "y", "weight") if reference else ("x", "y", "packed", "affine"),
                "dgrad": ("dy", "dx", "weight") if reference else ("dy", "dx", "packed_dx", "affine"),
                "wgrad": ("x", "dy", "dw")}[kind]
    for member in required:
        check(good(native, entry, **{member: None}), "null", member)
    if kind == "pack":
        check(good(native, entry, packed_dx=None), "needs packed_dx", "packed_dx with dx_planes")
        for cin, cout in ((0, 16), (81, 16), (17, 32), (17, 0)):
            check(good(native, entry, cin=cin, cout=cout), "cin must lie in [1, 80] and cout must be 16 or 64", (cin, cout))
        for planes in (-16, 1, 17, 32, 64):
            check(good(native, entry, dx_planes=planes), "dx_planes must be 0, 16 or 64 and at most cin", planes)
        return
    for over in (dict(cin=0), dict(cin=81), dict(cin=49), dict(cout=32), dict(height=11, width=11), dict(height=7, width=6)):
        check(good(native, entry, **over), "unsupported shape", over)
    most = lib.mztrain_conv_max_batch(17, 16, 3, 3)
    for batch in (0, -3, most + 1):
        check(good(native, entry, batch=batch), "batch must be positive", batch)
    if kind == "dgrad":
        for planes in (0, -16, 1, 17, 32, 64):
            check(good(native, entry, dx_planes=planes), "dx_planes must be 16 or 64 and at most cin", planes)
        check(good(native, entry, dx=0x1000), "dx must not be dy", "aliased")
        check(good(native, entry, cin=65, cout=64, dx_planes=16), "unsupported shape of the data gradient", "64 -> 16 on 3 x 3")
    if kind == "forward":
        check(good(native, entry, y=0x1000), "y must not be x", "aliased")
    if kind in ("forward", "dgrad") and not reference:
        for member in ("x", "y", "packed") if kind == "forward" else ("dy", "dx", "packed_dx"):
            check(good(native, entry, **{member: 0x1004}), "16-byte aligned", member)


@pytest.mark.parametrize("name,mirror_name,count", [("mztrain_conv_pack_args", "MzTrainConvPackArgs", 7),
                                                    ("mztrain_conv_forward_args", "MzTrainConvForwardArgs", 10),
                                                    ("mztrain_conv_dgrad_args", "MzTrainConvDgradArgs", 11),
                                                    ("mztrain_conv_wgrad_args", "MzTrainConvWgradArgs", 8)])
def test_argument_structs_match_their_ctypes_mirrors(native, tmp_path, name, mirror_name, count):
    fields = c_fields("mztrain.h", name)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mztrain.h"', "int main(void) {",
             f'    printf("%zu", sizeof({name}));']
    lines += [f'    printf(" %zu", offsetof({name}, {f}));' for f in fields]
    lines += ['    printf(" %d %d", MZTRAIN_CONV_SLICE, MZTRAIN_CONV_AFFINE);', "    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, *offsets, slice_length, affine = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    mirror = getattr(native, mirror_name)
    assert [n for n, *_ in mirror._fields_] == fields and len(fields) == count
    assert ctypes.sizeof(mirror) == size
    assert [getattr(mirror, f).offset for f in fields] == offsets
    assert slice_length == native.CONV_SLICE and affine == native.CONV_AFFINE


# ---- the header under the sanitizers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("conv_train") / "conv_train_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "conv_train_check.cpp")],
                   check=True)
    return exe


SANITIZED = [s for s in ref.SHAPES if s[0] * s[1] * s[2] * s[3] * s[4] <= 60000]


@pytest.mark.parametrize("shape", SANITIZED, ids=["B{}-{}to{}-{}x{}-dx{}".format(*s) for s in SANITIZED])
def test_the_header_under_the_sanitizers(native, lib, program, tmp_path, shape):
    """The stand-alone program gives the host entries' bits on random data: outputs, both packings and the plan."""
    b, cin, cout, h, w, dx_planes = shape
    x, weight, dy = ref.normal_case(shape, seed=13)
    source, result = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(source, "wb") as f:
        f.write(struct.pack("<q5i", b, cin, cout, h, w, dx_planes))
        for a in (x, weight, dy):
            f.write(a.tobytes())
    done = subprocess.run([program, str(source), str(result)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    raw = np.fromfile(result, dtype=np.float32)
    packed, packed_dx, _ = ref.host_pack(native, lib, weight, dx_planes)
    want = [ref.host_forward(native, lib, x, weight)]
    if dx_planes:
        want.append(ref.host_dgrad(native, lib, dy, weight, dx_planes))
    want += [ref.host_wgrad(native, lib, x, dy), packed] + ([packed_dx] if dx_planes else [])
    rc, numbers = plan(lib, b, cin, cout, h, w)
    want.append(np.array(numbers, dtype=np.float32))
    want = np.concatenate([a.reshape(-1) for a in want])
    assert rc == 0 and raw.size == want.size
    assert np.array_equal(raw.view(np.uint32), want.view(np.uint32))
    exact = ref.wgrad_exact(x, dy).reshape(-1)                   # and the rule is a sound float32 sum: a few ulps of sum|a b|
    at = b * cout * h * w + b * dx_planes * h * w
    assert np.abs(raw[at: at + exact.size] - exact).max() <= 1e-6 * max(1e-30, np.abs(exact).max())


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def checkpoint(game):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    return {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}, config


def test_trainer_refuses_a_fully_connected_network(pkg):
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    ckpt, config = checkpoint("cartpole")
    with pytest.raises(NotImplementedError, match="native_conv=True.*residual networks"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_conv=True)


def test_trainer_refuses_a_model_off_the_gpu(pkg):
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    ckpt, config = checkpoint("tictactoe")
    with pytest.raises(NotImplementedError, match="native_conv=True.*must be on the GPU"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_conv=True)


def test_trainer_refuses_a_network_without_a_covered_convolution(pkg):
    """Gomoku's layers have 128 channels: nothing to switch is a refusal, not a silent no-op."""
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    ckpt, config = checkpoint("gomoku")
    with pytest.raises(NotImplementedError, match=r"native_conv=True\) found no 3 x 3 convolution"):
        trainer_mod.Trainer(ckpt, config, device="cpu", native_conv=True)
    model = models.MuZeroNetwork(config)
    assert not any(m.training_covered() for m in model.modules() if isinstance(m, models.BoardConv2d))


def test_the_switch_left_off_keeps_the_torch_path(pkg):
    """Off, or on for weights that are not on the GPU: no module is switched, every module reports the torch path and the
    convolution is torch's, bit for bit, with autograd."""
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    torch.manual_seed(2)
    model = models.MuZeroNetwork(config)
    convs = [m for m in model.modules() if isinstance(m, models.BoardConv2d)]
    assert len(convs) >= 5
    for on in (False, True):
        assert model.native_training_conv(on) == 0
        for conv in convs:
            x = torch.randn(4, conv.in_channels, 3, 3, requires_grad=True)
            assert not conv.takes_training_path(x) and not conv.takes_training_path(x[:, :-1], extra_plane=True)
        conv = convs[1].train()
        x = torch.randn(4, conv.in_channels, 3, 3, requires_grad=True)
        got = conv(x)
        assert got.grad_fn is not None and torch.equal(got, torch.nn.functional.conv2d(x, conv.weight, padding=1))
    dyn = model.dynamics_network.module.conv
    assert dyn.training_dx_planes() == dyn.in_channels - 1 == 16 and convs[0].training_dx_planes() == 0
