"""The device frame stack on the GPU (include/mzenv.h mzenv_stack_reset / mzenv_stack_push, csrc/obs_stack.hip) against the
numpy model of obs_stack_cases.py, which is GameHistory.get_stacked_observations.  Frames are copied and an action becomes
float(action): every comparison is exact (bit patterns)."""
import importlib

import numpy as np
import pytest
import torch

import obs_stack_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_mod(pkg):
    return importlib.import_module("muzero-hypermodel_amd.games.device")


def _upload(sc):
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in sc.items()}


def _ply(stack, dev, t, out):
    """Ply t of a script: the masked reset at RESET_AT, a push everywhere else."""
    if t == cases.RESET_AT:
        return stack.reset(dev["frames"][t + 1], out, mask=dev["mask"])
    return stack.push(dev["frames"][t], dev["actions"][t], dev["done"][t], dev["frames"][t + 1], out)


def _same(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("n", cases.DEPTHS)
def test_stack_plays_the_scripts(device_mod, shape, n):
    """70 envs (a full 64-env group and a partial one): after the first reset, after every ply -- pushes, untouched envs,
    games that end -- and after the masked reset in mid-script, stacked_out equals the model for every env.  The output
    buffer starts out as NaN, so a float the kernel does not write shows."""
    sc = cases.script(shape, n)
    want, _ = cases.model(shape, n)
    dev = _upload(sc)
    stack = device_mod.DeviceFrameStack(cases.E, shape, n)
    assert stack.stacked_shape == want.shape[2:]
    out = stack.new_output().fill_(float("nan"))
    stack.reset(dev["frames"][0], out)
    assert _same(out, want[0])
    for t in range(cases.PLIES):
        out.fill_(float("nan"))
        assert _ply(stack, dev, t, out) is out
        assert _same(out, want[t + 1]), t
    stack.close()


def test_two_stacks_on_two_streams_do_not_mix(device_mod):
    """A second stack of another depth plays another script on a second stream, ply by ply in turn with the first: each
    keeps its own frames, heads and counts."""
    a_case, b_case = ((3, 3, 3), 2), ((3, 3, 3), 5)
    runs = []
    for shape, n in (a_case, b_case):
        stack = device_mod.DeviceFrameStack(cases.E, shape, n)
        stream = torch.cuda.Stream()
        dev = _upload(cases.script(shape, n))
        outs = stack.new_output(cases.PLIES + 1)
        runs.append((stack, stream, dev, outs, cases.model(shape, n)[0]))
    torch.cuda.synchronize()
    for stack, stream, dev, outs, _ in runs:
        with torch.cuda.stream(stream):
            stack.reset(dev["frames"][0], outs[0])
    for t in range(cases.PLIES):
        for stack, stream, dev, outs, _ in runs:
            with torch.cuda.stream(stream):
                _ply(stack, dev, t, outs[t + 1])
    for stack, stream, dev, outs, want in runs:
        stream.synchronize()
        assert _same(outs, want)
        stack.close()


def test_binding_refuses_what_is_not_resident_or_not_its_shape(device_mod):
    stack = device_mod.DeviceFrameStack(4, (1, 1, 4), 1)
    obs = torch.zeros((4, 1, 1, 4), device="cuda")
    out = stack.new_output()
    assert out.shape == (4, 3, 1, 4)
    acts = torch.zeros(4, dtype=torch.int32, device="cuda")
    done = torch.zeros(4, dtype=torch.uint8, device="cuda")
    for bad in (dict(obs_before=obs.cpu()), dict(actions=acts.long()), dict(done=done[:3]), dict(obs_next=obs[:, :, :, :3]),
                dict(out=obs)):
        with pytest.raises(ValueError):
            stack.push(**{**dict(obs_before=obs, actions=acts, done=done, obs_next=obs, out=out), **bad})
    with pytest.raises(RuntimeError, match="n = 0 needs none"):
        device_mod.DeviceFrameStack(4, (1, 1, 4), 0)
    stack.close()
