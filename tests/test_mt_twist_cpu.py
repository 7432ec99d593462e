"""The phase form of the MT19937 regeneration (csrc/np_legacy_rng.h mt_twist_*) that the narrow whole-move kernel runs
with the 16 lanes of a tree's row (narrow_device.h mt_regenerate_row), built for the host with g++ and run as 16
emulated lanes, one phase at a time, every lane's loads before any lane's store (tests/mt_twist_check.cpp).

The phase boundaries are the one place the split can go wrong: an element reads its neighbour key[k + 1] as the OLD word,
and the neighbour belongs to another lane (to the next phase when k is a phase's last element).  Whatever order the lanes
run in -- ascending, descending, a seeded shuffle -- the block must be the one the serial mt_regenerate leaves, and the one
numpy's own RandomState holds after its generator crossed a block."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
INPUTS, BLOCKS = 34, 3          # seeds 0..31, the all-zero block, the all-ones block; three successive blocks each


@pytest.fixture(scope="module")
def twisted(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build tests/mt_twist_check.cpp"
    tmp = tmp_path_factory.mktemp("mt_twist")
    exe, out = str(tmp / "mt_twist_check"), str(tmp / "blocks.u32")
    subprocess.run([gxx, "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "mt_twist_check.cpp")],
                   check=True)
    proc = subprocess.run([exe, out], capture_output=True, text=True)
    report = json.loads(proc.stdout.strip().splitlines()[-1])
    blocks = np.fromfile(out, dtype=np.uint32).reshape(INPUTS, BLOCKS, 624)
    return proc.returncode, report, blocks


def test_lane_orders_equal_serial_regeneration(twisted):
    """ascending, descending and shuffled lane order against mt_regenerate, on every input and block"""
    returncode, report, _ = twisted
    assert report["tiling"], "the phases do not tile [0, 624) in order"
    assert report["blocks"] == INPUTS * BLOCKS * 3
    assert report["mismatches"] == 0 and returncode == 0, report


def _numpy_blocks(state):
    rs = np.random.RandomState()
    rs.set_state(state)
    out = []
    for _ in range(BLOCKS):
        rs.bytes(4)                      # the first word of a new block: numpy regenerates
        kind, key, pos = rs.get_state()[:3]
        assert kind == "MT19937" and pos == 1
        out.append(key.copy())
        rs.bytes(4 * 623)                # the rest of the block
        assert rs.get_state()[2] == 624
    return np.stack(out)


@pytest.mark.parametrize("seed", range(32))
def test_blocks_equal_numpy_state_after_crossing(twisted, seed):
    state = np.random.RandomState(seed).get_state()
    assert state[2] == 624
    assert np.array_equal(twisted[2][seed], _numpy_blocks(state))


@pytest.mark.parametrize("index,fill", [(32, 0x00000000), (33, 0xFFFFFFFF)])
def test_degenerate_blocks_equal_numpy(twisted, index, fill):
    state = ("MT19937", np.full(624, fill, dtype=np.uint32), 624, 0, 0.0)
    assert np.array_equal(twisted[2][index], _numpy_blocks(state))
