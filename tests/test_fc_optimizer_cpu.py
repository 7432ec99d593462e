"""The flat-buffer optimizer (csrc/fc_optimizer.h, include/mztrain.h mztrain_opt_*) without a GPU, through
mztrain_opt_reference on host arrays.

The yardstick (tests/fc_optimizer_reference.py, float64 numpy from the formulas) is first held to torch.optim in float64
(1e-12 relative).  The float32 entry is then held to it by the project's rule for a training step: native
error <= 4 max(library error, 4 * 2^-24 max|x64|), the library being torch.optim in float32 on the CPU; for the weights and
every moment tensor.  Three deliberate defects of the rule are shown to push a named tensor past that bound.  The per-step
scalars are Python's own expressions bit for bit.  Every refusal, the struct against its ctypes mirror, and the header under
the address and undefined-behaviour sanitizers (tests/fc_optimizer_check.cpp, a stand-alone program built with g++)."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import fc_optimizer_reference as ref
from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
CASES = [(label, decay) for label in ref.KINDS for decay in ref.DECAYS]


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def tensors_of(kind):
    return ("weights", "moment1", "moment2") if kind == "Adam" else ("weights", "moment1")


@pytest.mark.parametrize("label,decay", CASES, ids=[f"{l}-wd{d:g}" for l, d in CASES])
def test_the_float64_yardstick_is_torch_in_float64(label, decay):
    how = ref.KINDS[label]
    lrs = ref.learning_rates()
    for n in (5, 1748):
        weights, grads = ref.make_case(n)
        mine = ref.run64(how["kind"], weights, grads, lrs, weight_decay=decay, momentum=how.get("momentum", 0.0))
        theirs = ref.run_torch(how["kind"], weights, grads, lrs, torch.float64, weight_decay=decay,
                               momentum=how.get("momentum", 0.0))
        for key in tensors_of(how["kind"]):
            scale = np.abs(theirs[key]).max()
            assert np.abs(mine[key] - theirs[key]).max() <= 1e-12 * scale, (key, n)


@pytest.mark.parametrize("n", ref.SIZES)
@pytest.mark.parametrize("label,decay", CASES, ids=[f"{l}-wd{d:g}" for l, d in CASES])
def test_the_host_entry_meets_the_training_step_rule(native, label, decay, n):
    how = ref.KINDS[label]
    kind, momentum = how["kind"], how.get("momentum", 0.0)
    lrs = ref.learning_rates()
    weights, grads = ref.make_case(n)
    exact = ref.run64(kind, weights, grads, lrs, weight_decay=decay, momentum=momentum)
    library = ref.run_torch(kind, weights, grads, lrs, torch.float32, weight_decay=decay, momentum=momentum)
    got = ref.run_host_entry(native, kind, weights, grads, lrs, weight_decay=decay, momentum=momentum)
    assert got["steps_done"] == ref.STEPS
    worst = {}
    for key in tensors_of(kind):
        worst[key], _ = ref.ratio(got[key], library[key], exact[key])
    top = max(worst, key=worst.get)
    print(f"\n{label} wd {decay:g} n {n}: worst native error / allowed {worst[top]:.3f} ({top})")
    assert worst[top] <= 1.0, (top, worst)
    if kind == "SGD" and momentum == 0.0:
        assert not got["moment1"].any()


@pytest.mark.parametrize("defect,tensor", [("no_weight_decay", "moment1"), ("no_weight_decay", "weights"),
                                           ("t_off_by_one", "weights"), ("bc2s_left_out", "weights")])
def test_a_defect_pushes_its_tensor_past_the_bound(defect, tensor):
    """An implementation with the defect (the yardstick itself, in float64, stands in for it) fails the rule the host
    entry meets.  Five steps: Adam's first step hides the weight decay in the weights."""
    lrs = ref.learning_rates()
    weights, grads = ref.make_case(1748)
    exact = ref.run64("Adam", weights, grads, lrs, weight_decay=1e-4)
    library = ref.run_torch("Adam", weights, grads, lrs, torch.float32, weight_decay=1e-4)
    broken = ref.run64("Adam", weights, grads, lrs, weight_decay=1e-4, defect=defect)
    value, entry = ref.ratio(broken[tensor], library[tensor], exact[tensor])
    print(f"\n{defect}: {tensor} at {value:.1f} times the allowed error")
    assert value > 1.0, entry


def test_sgd_defect_no_weight_decay_pushes_the_momentum_buffer_past_the_bound():
    lrs = ref.learning_rates()
    weights, grads = ref.make_case(1748)
    exact = ref.run64("SGD", weights, grads, lrs, weight_decay=1e-4, momentum=0.9)
    library = ref.run_torch("SGD", weights, grads, lrs, torch.float32, weight_decay=1e-4, momentum=0.9)
    broken = ref.run64("SGD", weights, grads, lrs, weight_decay=1e-4, momentum=0.9, defect="no_weight_decay")
    value, entry = ref.ratio(broken["moment1"], library["moment1"], exact["moment1"])
    assert value > 1.0, entry


def bits(x):
    return struct.pack("<d", x)


def test_the_scalars_are_pythons_own_expressions_bit_for_bit(native):
    lib = native.load()
    out = (ctypes.c_double * 4)()
    lr = 0.02 * 0.8 ** (3 / 7)
    for beta1, beta2 in ((0.9, 0.999), (0.999, 0.9), (0.5, 0.0), (0.0, 0.5)):
        for t in range(1, 20001):
            assert lib.mztrain_opt_scalars(lr, beta1, beta2, t, out) == 0
            bc1 = 1 - beta1 ** t
            bc2 = 1 - beta2 ** t
            want = (bc1, bc2, lr / bc1, bc2 ** 0.5)
            if tuple(out) != want or any(bits(a) != bits(b) for a, b in zip(out, want)):
                raise AssertionError((beta1, beta2, t, tuple(out), want))
    assert lib.mztrain_opt_scalars(lr, 1.0, 0.5, 1, out) == native.ERR_INVALID
    assert lib.mztrain_opt_scalars(lr, 0.9, 0.5, 0, out) == native.ERR_INVALID
    assert lib.mztrain_opt_scalars(lr, 0.9, 0.5, 1, None) == native.ERR_INVALID


def test_first_sgd_step_on_a_zero_buffer_is_torchs_clone(native):
    """buf = fmaf(momentum, 0, g1) is g1: the first step's buffer equals torch's clone of the gradient, bit for bit."""
    weights, grads = ref.make_case(257, steps=1)
    got = ref.run_host_entry(native, "SGD", weights, grads, [0.02], momentum=0.9)
    library = ref.run_torch("SGD", weights, grads, [0.02], torch.float32, momentum=0.9)
    assert np.array_equal(got["moment1"].astype(np.float64), library["moment1"])


# ---- refusals -------------------------------------------------------------------------------------------------------------
def good_args(native, kind="Adam", **over):
    fields = dict(n=8, weights=0x1000, grads=0x2000, moment1=0x3000, moment2=0x4000, lr=0x5000, steps_done=0x6000)
    hyper = dict(weight_decay=1e-4, momentum=0.9 if kind == "SGD" else 0.0)
    for key in list(over):
        if key in hyper or key in ("beta1", "beta2", "eps"):
            hyper[key] = over.pop(key)
    fields.update(over)
    return ref.opt_args(native, kind, fields["n"], fields["weights"], fields["grads"], fields["moment1"], fields["moment2"],
                        fields["lr"], fields["steps_done"], **hyper)


@pytest.mark.parametrize("entry", ["mztrain_opt_step", "mztrain_opt_reference"])
def test_refusals(native, entry):
    """Decided on the arguments alone: the pointers are never followed (they point nowhere)."""
    lib = native.load()

    def refused(args):
        function = getattr(lib, entry)
        pointer = ctypes.byref(args) if args is not None else None
        rc = function(pointer, None) if entry == "mztrain_opt_step" else function(pointer)
        return rc, (lib.mzmcts_last_error(None) or b"").decode()

    def check(args, text, why):
        rc, message = refused(args)
        assert rc == native.ERR_INVALID and text in message and message.startswith(entry + ":"), (why, rc, message)

    check(None, "null args", "null args")
    for member in ("weights", "grads", "lr", "steps_done"):
        for kind in ("Adam", "SGD"):
            check(good_args(native, kind, **{member: None}), "null pointer in args", (kind, member))
    for member in ("moment1", "moment2"):
        check(good_args(native, "Adam", **{member: None}), "Adam needs moment1 and moment2", member)
    check(good_args(native, "SGD", moment1=None), "SGD with momentum needs moment1", "sgd moment1")
    for n in (0, -5):
        check(good_args(native, n=n), "n must be positive", n)
    for kind in (2, -1, 7):
        args = good_args(native)
        args.kind = kind
        check(args, "unknown kind", kind)
    for name in ("beta1", "beta2"):
        for value in (1.0, -0.1, 1.5, float("nan")):
            check(good_args(native, **{name: value}), "beta1 and beta2 must lie in [0, 1)", (name, value))
    for value in (0.0, -1e-8, float("nan")):
        check(good_args(native, eps=value), "eps must be positive", value)
    for kind in ("Adam", "SGD"):
        for value in (-1e-4, float("inf"), float("nan")):
            check(good_args(native, kind, weight_decay=value), "weight_decay must be finite and not negative", (kind, value))
            check(good_args(native, kind, momentum=value), "momentum must be finite and not negative", (kind, value))


def test_sgd_without_momentum_takes_null_moments(native):
    weights, grads = ref.make_case(5, steps=2)
    got = ref.run_host_entry(native, "SGD", weights, grads, [0.1, 0.05], momentum=0.0)       # moment1 = moment2 = NULL
    w = weights.astype(np.float64)
    for g, lr in zip(grads, (0.1, 0.05)):
        w = w - lr * g.astype(np.float64)
    assert np.abs(got["weights"] - w).max() <= 4 * ref.U * np.abs(w).max() and got["steps_done"] == 2


def test_argument_struct_matches_its_ctypes_mirror(native, tmp_path):
    fields = c_fields("mztrain.h", "mztrain_opt_args")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mztrain.h"', "int main(void) {",
             '    printf("%zu", sizeof(mztrain_opt_args));']
    lines += [f'    printf(" %zu", offsetof(mztrain_opt_args, {f}));' for f in fields]
    lines += ['    printf(" %d %d", MZTRAIN_OPT_ADAM, MZTRAIN_OPT_SGD);', "    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, *rest = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    offsets, kinds = rest[:-2], rest[-2:]
    mirror = native.MzTrainOptArgs
    assert [name for name, *_ in mirror._fields_] == fields and len(fields) == 13
    assert ctypes.sizeof(mirror) == size
    assert [getattr(mirror, f).offset for f in fields] == offsets
    assert kinds == [native.OPT_ADAM, native.OPT_SGD]


# ---- the header under the sanitizers -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("fc_optimizer") / "fc_optimizer_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "fc_optimizer_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("label,decay", CASES, ids=[f"{l}-wd{d:g}" for l, d in CASES])
def test_the_header_under_the_sanitizers_gives_the_entrys_bits(native, program, tmp_path, label, decay):
    how = ref.KINDS[label]
    kind, momentum = how["kind"], how.get("momentum", 0.0)
    lrs = ref.learning_rates()
    for n in (1, 5, 257):
        weights, grads = ref.make_case(n)
        source, result = tmp_path / f"case{n}.bin", tmp_path / f"out{n}.bin"
        with open(source, "wb") as f:
            f.write(struct.pack("<iiqq5d", native.OPT_ADAM if kind == "Adam" else native.OPT_SGD, len(grads), n, 0,
                                ref.BETA1, ref.BETA2, ref.EPS, decay, momentum))
            f.write(np.asarray(lrs, dtype=np.float64).tobytes())
            f.write(weights.tobytes())
            for g in grads:
                f.write(g.tobytes())
        done = subprocess.run([program, str(source), str(result)], capture_output=True, text=True)
        assert done.returncode == 0, done.stderr
        raw = np.fromfile(result, dtype=np.uint8)
        arrays = raw[:12 * n].view(np.float32).reshape(3, n)
        want = ref.run_host_entry(native, kind, weights, grads, lrs, weight_decay=decay, momentum=momentum)
        for index, key in enumerate(("weights", "moment1", "moment2")):
            if key in want:
                assert np.array_equal(arrays[index].view(np.uint32), want[key].view(np.uint32)), (key, n)
            else:
                assert not arrays[index].any()
        if kind == "Adam":
            t = len(grads)
            bc1, bc2 = 1 - ref.BETA1 ** t, 1 - ref.BETA2 ** t
            assert raw[12 * n:].view(np.float64).tolist() == [bc1, bc2, lrs[-1] / bc1, bc2 ** 0.5]
