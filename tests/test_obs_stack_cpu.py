"""The device frame stack, the parts that need no GPU: csrc/obs_stack.h built for the host (tests/obs_stack_check.cpp)
against fixture G9 (recorded from the reference's GameHistory.get_stacked_observations) and against the scripts of
obs_stack_cases.py, the coverage those scripts must have, and the argument checks of mzenv_stack_*.  Frames are copied
and an action becomes float(action): every comparison is exact."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import obs_stack_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


@pytest.fixture(scope="module")
def stack_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("obs_stack") / "obs_stack_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "obs_stack_check.cpp")], check=True)

    def bits(frame):
        return " ".join(map(str, np.ascontiguousarray(frame, dtype=np.float32).view(np.uint32).reshape(-1).tolist()))

    def run(shape, n, first, commands):
        """commands: ("P", action, done, frame) | ("R", mask, frame); returns f32 [1 + len(commands), stacked planes, H, W]."""
        c, h, w = shape
        lines = [f"{c} {h * w} {n}", "F " + bits(first)]
        for cmd in commands:
            lines.append(" ".join([cmd[0]] + [str(int(v)) for v in cmd[1:-1]] + [bits(cmd[-1])]))
        proc = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert proc.returncode == 0, (proc.returncode, proc.stderr)
        out = np.array([line.split() for line in proc.stdout.splitlines()], dtype=np.uint64).astype(np.uint32)
        assert out.shape == (1 + len(commands), (c + n * (c + 1)) * h * w)
        return out.view(np.float32).reshape(1 + len(commands), c + n * (c + 1), h, w)
    return run


def test_rule_header_replays_g9(golden, stack_check):
    """Fixture G9: six frames and their actions pushed one by one; at indices 0, 1, 3 and 5 the stacked observation
    equals the reference's for n = 2 and n = 4, index -1 is index 5, and n = 0 yields the frame itself."""
    fx = golden("g9_stacked_observations")
    obs, actions = fx["observations"], fx["actions"]
    assert obs.shape == (6, 3, 3, 3) and actions.shape == (6,)
    # frame i is played from with action_history[i + 1]; the search after it sees frame i + 1
    commands = [("P", actions[i + 1], 0, obs[i + 1]) for i in range(5)]
    for n in (0, 2, 4):
        got = stack_check((3, 3, 3), n, obs[0], commands)
        for idx in (0, 1, 3, 5):
            want = fx[f"stack{n}_idx{idx}"]
            assert got[idx].dtype == want.dtype and np.array_equal(got[idx].view(np.uint32), want.view(np.uint32)), (n, idx)
        assert np.array_equal(got[5], fx[f"stack{n}_idx-1"])
        if n == 0:
            assert np.array_equal(got, obs)


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("n", cases.DEPTHS)
def test_scripts_cover_what_the_gpu_test_relies_on(pkg, shape, n):
    """So that tests/test_gpu_obs_stack.py cannot pass vacuously: for every (shape, n) some env has a game longer than n
    (the ring wraps), a game over before n frames (zeros remain), a done followed by an observation that must not hold
    the old game's frames, an untouched ply between two played ones, and a done on the first ply of a game; the
    mid-script reset clears some envs in mid-game and spares others that hold frames."""
    assert cases.E == 70 and cases.E > 64 and cases.E % 64
    cover = cases.coverage(shape, n)
    assert cover == dict(ring_wraps=True, zeros_remain=True, done_after_frames=True, untouched_between_played=True,
                         done_on_first_ply=True), cover
    sc = cases.script(shape, n)
    want, held = cases.model(shape, n)
    assert (sc["actions"] < 0).any() and sc["actions"].max() == cases.NUM_ACTIONS - 1
    at = cases.RESET_AT
    masked, spared = sc["mask"] != 0, sc["mask"] == 0
    assert (held[at][masked] > 0).any() and (held[at][spared] > 0).any()
    assert (held[at + 1][masked] == 0).all() and np.array_equal(held[at + 1][spared], held[at][spared])
    c = shape[0]
    assert want.shape == (cases.PLIES + 1, cases.E, c + n * (c + 1)) + tuple(shape[1:])
    # the model is the reference rule: the current frame first, then zeros exactly where the game has no frame yet
    assert np.array_equal(want[:, :, :c], sc["frames"])
    for k in range(n):
        planes = want[:, :, c + k * (c + 1): c + (k + 1) * (c + 1)]
        assert not planes[held <= k].any() and planes[held > k].any()


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("n", cases.DEPTHS)
def test_rule_header_plays_the_scripts(pkg, stack_check, shape, n):
    """csrc/obs_stack.h on a host ring, pushed frame written before the output is gathered: the stacked observation
    after the first reset, after every ply and after the masked reset equals GameHistory.get_stacked_observations."""
    sc = cases.script(shape, n)
    want, _ = cases.model(shape, n)
    for e in list(range(6)) + [63, 64, cases.E - 1]:
        commands = []
        for t in range(cases.PLIES):
            if t == cases.RESET_AT:
                commands.append(("R", sc["mask"][e], sc["frames"][t + 1, e]))
            else:
                commands.append(("P", sc["actions"][t, e], sc["done"][t, e], sc["frames"][t + 1, e]))
        got = stack_check(shape, n, sc["frames"][0, e], commands)
        assert np.array_equal(got.view(np.uint32), want[:, e].view(np.uint32)), (e, np.flatnonzero((got != want[:, e]).any(axis=(1, 2, 3)))[:5])


def test_stack_entries_check_their_arguments_without_a_device(pkg):
    """mzenv_stack_create refuses null pointers, n <= 0, a non-positive shape or env count and a stacked width whose float
    count leaves int32 before any device work; mzenv_stack_push / _reset refuse null pointers before they look at the
    handle.  Without a GPU a good create gets as far as the device and says so (ERR_HIP)."""
    import torch
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    handle = ctypes.c_void_p()

    def create(E=4, c=3, h=3, w=3, n=2, device=0, out=ctypes.byref(handle)):
        return lib.mzenv_stack_create(E, c, h, w, n, device, out)

    for bad in (dict(out=None), dict(n=0), dict(n=-1), dict(E=0), dict(E=-3), dict(c=0), dict(h=0), dict(w=-1),
                dict(c=1, h=1, w=4, n=2 ** 31 - 1),                 # 4 + n * 8 floats
                dict(c=3, h=2 ** 15, w=2 ** 15, n=1),               # C * H * W alone
                dict(c=1, h=2 ** 16, w=2 ** 16, n=1),               # H * W alone
                dict(c=2 ** 31 - 1, h=1, w=1, n=1),
                dict(c=1, h=1, w=4, n=2 ** 28)):                    # 4 + 8 n = 2^31 + 4: the first n that leaves int32
        assert create(**bad) == native.ERR_INVALID and not handle.value, bad
        assert b"mzenv_stack_create" in lib.mzenv_stack_last_error(None)
    assert create(n=2 ** 31 - 1, c=1, h=1, w=1) == native.ERR_INVALID
    assert b"int32" in lib.mzenv_stack_last_error(None)
    ptr = 0x10000                                   # never dereferenced: every refused call returns before a launch
    good = dict(obs_before=ptr, actions=ptr, done=ptr, obs_next=ptr, out=ptr)
    for name in good:
        a = {**good, name: None}
        assert lib.mzenv_stack_push(None, a["obs_before"], a["actions"], a["done"], a["obs_next"], a["out"], None) \
            == native.ERR_INVALID, name
        assert b"null argument" in lib.mzenv_stack_last_error(None)
    assert lib.mzenv_stack_push(None, ptr, ptr, ptr, ptr, ptr, None) == native.ERR_INVALID
    assert b"null handle" in lib.mzenv_stack_last_error(None)
    assert lib.mzenv_stack_reset(None, None, None, ptr, None) == native.ERR_INVALID
    assert lib.mzenv_stack_reset(None, None, ptr, None, None) == native.ERR_INVALID
    assert lib.mzenv_stack_reset(None, None, ptr, ptr, None) == native.ERR_INVALID
    assert lib.mzenv_stack_floats(None) == -1
    lib.mzenv_stack_destroy(None)
    rc = create(E=1, c=1, h=1, w=1, n=1)
    if not torch.cuda.is_available():
        assert rc == native.ERR_HIP and not handle.value
        assert b"no HIP device" in lib.mzenv_stack_last_error(None)
        # the largest width that is still an int32 (2^31 - 4 floats) passes the argument check
        assert create(E=1, c=1, h=1, w=4, n=2 ** 28 - 1) == native.ERR_HIP
        device = importlib.import_module("muzero-hypermodel_amd.games.device")
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            device.DeviceFrameStack(4, (3, 3, 3), 2)
    else:
        assert rc == 0 and lib.mzenv_stack_floats(handle) == 3
        lib.mzenv_stack_destroy(handle)
