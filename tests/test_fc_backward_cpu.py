"""csrc/fc_backward.h on the CPU: tests/fc_backward_check.cpp, a stand-alone program built by g++ with the address and
undefined-behaviour sanitizers, runs the backward rule and the weight-gradient sum in float32 on the float64 yardstick's
activations and logit gradients (rounded to float32) and is held to the yardstick's gradients.

The bound.  Every value the rule produces is a sum of products of its inputs; the yardstick carries, beside each, the sum
of the absolute values of those terms (M) and the number n of float32 operations on the longest path that leads to it
(fc_train_reference._Tracked).  The roundings of the inputs are counted in n where they occur: a delta at the logits
has n = 3 (the logit gradient rounded to float32, 1 / B rounded, their product), a Linear adds its `out` accumulations and
one for the rounded weight, an ELU slope three (the saved activation rounded, y + 1, the product).  Rounding each of these
once moves the result by at most gamma(n) M.  Allowed: 4 n 2^-24 M per entry, for the deltas and for the weight gradients
(whose float64 accumulation adds one rounding, counted in n).  An entry whose M is zero must be exactly zero."""
import os
import shutil
import subprocess

import importlib
import numpy as np
import pytest

import fc_train_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
CASES = [(name, B, K1) for name, sh in ref.SHAPES.items() for B, K1 in sh["cases"]]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("fc_backward") / "fc_backward_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "fc_backward_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def models(pkg):
    return importlib.import_module("muzero-hypermodel_amd.models")


def net_words(sh):
    """fcb::Net for the yardstick's record layout and the flat (unpadded) weight buffer, as int32 words; the plan rows."""
    off, places, R = ref.record_layout(sh)
    table, widths, n_weights = ref.flat_offsets(sh)
    F = 2 * sh["support"] + 1
    width = max(max(w) for w in widths)
    words = [sh["obs"], sh["enc"], sh["A"], F, off["raw"], off["norm"], off["stats"], R, (width + 3) // 4 * 4]
    steps = [0, 1, 1, 2, 2]
    plan = []
    for m in range(5):
        n = len(widths[m]) - 1
        words.append(n)
        for l in range(4):
            if l < n:
                fan_in, fan_out = widths[m][l], widths[m][l + 1]
                w_off, b_off = table[m][l]
                x_off, y_off = places[m][l]
                words += [fan_in, fan_out, fan_in, w_off, b_off, x_off, y_off]
                plan.append([fan_in, fan_out, x_off, y_off, w_off, b_off, steps[m]])
            else:
                words += [0] * 7
    assert len(words) == 9 + 5 * 29
    return np.array(words, dtype=np.int32), np.array(plan, dtype=np.int32), R, n_weights


def run(program, tmp_path, sh, state, out, B, K1):
    words, plan, R, n_weights = net_words(sh)
    weights = ref.flatten(state)
    assert weights.size == n_weights
    loss = out["loss"]
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([B, K1, n_weights, len(plan)], dtype=np.int32).tobytes())
        f.write(words.tobytes())
        f.write(plan.tobytes())
        for a in (weights, out["act"], loss["grad_value"], loss["grad_reward"], loss["grad_policy"]):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    proc = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    got = np.fromfile(dst, dtype=np.float32)
    assert got.size == B * K1 * R + n_weights
    return got[:B * K1 * R].reshape(B, K1, R).astype(np.float64), got[B * K1 * R:].astype(np.float64)


@pytest.mark.parametrize("name,B,K1", CASES, ids=[f"{n}-B{b}-K{k}" for n, b, k in CASES])
def test_rule_in_float32_vs_the_yardstick(program, models, tmp_path, name, B, K1):
    sh = ref.SHAPES[name]
    model = ref.make_model(models, sh, ref.SEEDS[name])
    state = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    batch = ref.make_batch(sh, B, K1, seed=B * 100 + K1, weights="per" if B % 2 else "none", bad_actions=(name == "S5"))
    out = ref.unroll64(state, batch, sh)
    deltas, grads = run(program, tmp_path, sh, state, out, B, K1)
    allowed = 4.0 * out["del_chain"] * ref.U * out["del_mag"]
    error = np.abs(deltas - out["del"])
    worst = float((error / np.maximum(allowed, 1e-300)).max())
    print(f"\n{name} B{B} K{K1}: deltas worst error / allowed {worst:.3f}")
    assert (error <= allowed).all(), worst
    table, widths, _ = ref.flat_offsets(sh)
    for key, g64 in out["grads"].items():
        m, l = ref.MLPS.index(key.split(".")[0]), int(key.split(".")[2]) // 2
        at = table[m][l][0 if key.endswith("weight") else 1]
        got = grads[at:at + g64.size].reshape(g64.shape)
        allowed = 4.0 * out["grad_chains"][key] * ref.U * out["grad_mags"][key]
        error = np.abs(got - g64)
        assert (error <= allowed).all(), (key, float((error / np.maximum(allowed, 1e-300)).max()))
        if K1 == 1 and m in (1, 2):
            assert (got == 0).all() and not np.signbit(got).any(), key
    assert not (grads == -12345.0).any(), "an entry of the gradient buffer was not written"
