"""mztrain_fc_* without a GPU: the argument struct against its ctypes mirror, and every refusal that is decided before
anything touches a device (the one refusal that needs a live handle, a batch above the created maxima, is in
tests/test_gpu_fc_train.py)."""
import ctypes
import importlib
import os
import subprocess

import pytest

from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def test_argument_struct_matches_its_ctypes_mirror(native, tmp_path):
    fields = c_fields("mztrain.h", "mztrain_fc_args")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mztrain.h"', "int main(void) {",
             '    printf("%zu", sizeof(mztrain_fc_args));']
    lines += [f'    printf(" %zu", offsetof(mztrain_fc_args, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, *offsets = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    mirror = native.MzTrainFcArgs
    assert [name for name, *_ in mirror._fields_] == fields and len(fields) == 14
    assert ctypes.sizeof(mirror) == size
    assert [getattr(mirror, f).offset for f in fields] == offsets


def cartpole_desc(native, hidden=16, layers=1, obs=4, enc=8):
    desc = native.MzFcDesc()
    desc.observation_floats, desc.encoding_size = obs, enc
    for i in range(5):
        desc.n_hidden[i] = layers
        for k in range(min(layers, 3)):
            desc.hidden[i][k] = hidden
    return desc


CARTPOLE_WEIGHTS = (4 * 16 + 16 + 16 * 8 + 8) + (10 * 16 + 16 + 16 * 8 + 8) + 2 * (8 * 16 + 16 + 16 * 21 + 21) + (8 * 16 + 16 + 16 * 2 + 2)


def create(native, desc=None, actions=2, support=10, weights=0x1000, n_weights=CARTPOLE_WEIGHTS, grads=0x2000, max_batch=8,
           max_steps=3, out=True):
    lib = native.load()
    handle = ctypes.c_void_p()
    rc = lib.mztrain_fc_create(ctypes.byref(desc) if desc is not None else None, actions, support, weights, n_weights, grads,
                               max_batch, max_steps, 0, ctypes.byref(handle) if out else None)
    return rc, handle, (lib.mzmcts_last_error(None) or b"").decode()


def test_create_refusals(native):
    good = cartpole_desc(native)
    for how in (dict(desc=None), dict(desc=good, weights=None), dict(desc=good, grads=None), dict(desc=good, out=False)):
        rc, handle, message = create(native, **how)
        assert rc == native.ERR_INVALID and not handle.value and "null argument" in message, how
    for how in (dict(actions=0), dict(max_batch=0), dict(max_steps=-1)):
        rc, handle, message = create(native, desc=good, **how)
        assert rc == native.ERR_INVALID and not handle.value and "must be positive" in message, how
    sizes = "layer sizes outside the supported range (<= 3 hidden layers per MLP, widths <= 256)"
    for how in (dict(desc=cartpole_desc(native, hidden=257)), dict(desc=cartpole_desc(native, layers=4)),
                dict(desc=cartpole_desc(native, obs=0)), dict(desc=good, support=0), dict(desc=good, support=128)):
        rc, handle, message = create(native, **how)
        assert rc == native.ERR_INVALID and not handle.value and sizes in message, (how, message)
    rc, handle, message = create(native, desc=good, n_weights=CARTPOLE_WEIGHTS - 1)
    assert rc == native.ERR_INVALID and not handle.value and "n_weights does not match the layer description" in message
    # admitted by build_fc_net, too large for a workgroup's LDS: 256-wide layers throughout
    wide = cartpole_desc(native, hidden=256, layers=3, obs=256, enc=128)

    def count(*widths):
        return sum(a * b + b for a, b in zip(widths[:-1], widths[1:]))

    n = (count(256, 256, 256, 256, 128) + count(129, 256, 256, 256, 128) + 2 * count(128, 256, 256, 256, 21)
         + count(128, 256, 256, 256, 1))
    rc, handle, message = create(native, desc=wide, actions=1, n_weights=n)
    assert rc == native.ERR_INVALID and not handle.value and "160 KB of LDS" in message, message
    # positions b * K1 + k are counted in int32
    rc, handle, message = create(native, desc=good, max_batch=1 << 16, max_steps=1 << 15)
    assert rc == native.ERR_INVALID and not handle.value and "does not fit int32" in message, message


def test_the_cartpole_weight_count_is_accepted_up_to_the_device(native):
    """The same call with everything in order gets past every argument check: without a GPU it ends at the device."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("checks where a GPU-less machine stops")
    rc, handle, message = create(native, desc=cartpole_desc(native))
    assert rc == native.ERR_HIP and not handle.value, message


def step_args(native, **over):
    fields = dict(observations=0x100, actions=0x200, target_value=0x300, target_reward=0x400, target_policy=0x500,
                  gradient_scale=0x600, weight=None, batch=4, steps=3, value_loss_weight=0.25, per_alpha=0.5,
                  sample_loss=0x700, head_sums=0x800, priorities=0x900)
    fields.update(over)
    return native.MzTrainFcArgs(**fields)


def test_step_refusals(native):
    lib = native.load()

    def refused(handle, args):
        rc = lib.mztrain_fc_step(handle, ctypes.byref(args) if args is not None else None, None)
        return rc, (lib.mzmcts_last_error(None) or b"").decode()

    rc, message = refused(None, step_args(native))
    assert rc == native.ERR_INVALID and "null handle" in message
    rc, message = refused(None, None)
    assert rc == native.ERR_INVALID and "null args" in message
    for member in ("observations", "actions", "target_value", "target_reward", "target_policy", "gradient_scale", "sample_loss",
                   "head_sums", "priorities"):
        rc, message = refused(None, step_args(native, **{member: None}))
        assert rc == native.ERR_INVALID and "null pointer in args" in message, member
    for how in (dict(batch=0), dict(steps=0), dict(batch=-3)):
        rc, message = refused(None, step_args(native, **how))
        assert rc == native.ERR_INVALID and "must be positive" in message, how
    assert lib.mztrain_fc_workspace_bytes(None) == -1
    pointers = [ctypes.c_void_p() for _ in range(3)]
    assert lib.mztrain_fc_logits(None, *(ctypes.byref(p) for p in pointers)) == native.ERR_INVALID
    lib.mztrain_fc_destroy(None)
