"""np_legacy_rng.h DeviceStream WITH a staged window -- the form root_noise_kernel and move_inputs_kernel draw the
exploration noise through -- built for the host with g++ (tests/device_stream_check.cpp, mode `windows`) and held to the
window-less form, to HostStream and to numpy.random.RandomState itself, bit for bit: rows, position, word count and
the key block after the draw.  One stream state per start position 0..624 (tests/noise_stream_cases.py), plus a state
constructed so that the draw ends at 624 exactly; windows of every length 0..96 for the short rows, of lengths 0, 1, 95
and 96 for 121 and 256 actions.  The window array is allocated at exactly its length and the program is built once more
with -fsanitize=address,undefined and run directly on the positions around the block's end."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import noise_stream_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "device_stream_check.cpp")

ALL_LENGTHS = list(range(cases.WINDOW + 1))
FEW_LENGTHS = [0, 1, cases.WINDOW - 1, cases.WINDOW]
# under the sanitizers: both ends of the block, the last position with a full window and its neighbours, and every
# position of the last 64, where the window is clipped
SAN_POSITIONS = sorted({0, 1, 300, 527, 528, 529} | set(range(cases.BLOCK - 64, cases.BLOCK + 1)))


def lengths_of(k):
    return ALL_LENGTHS if k <= 9 else FEW_LENGTHS


def build(gxx, out, flags):
    built = subprocess.run([gxx] + flags + ["-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", out, SOURCE, "-lm"],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return out


@pytest.fixture(scope="module")
def gxx():
    found = shutil.which("g++")
    if found is None:
        pytest.skip("no g++")
    return found


def fma_flags():
    return ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []     # (without it __builtin_fma calls libm's fma)


@pytest.fixture(scope="module")
def exe(gxx, tmp_path_factory):
    return build(gxx, str(tmp_path_factory.mktemp("device_stream") / "device_stream_check"), ["-O2", "-Wall", "-Werror"] + fma_flags())


def states_of(alpha, k, positions):
    """the sweep's states at `positions`, and for the short rows the constructed exact end"""
    states = [cases.sweep_state(e) for e in positions]
    if k <= 9:
        states.append(cases.exact_end_state(alpha, k))
    return states


def run_windows(exe, alpha, k, lengths, states):
    lines = ["%r %d %d %s\n" % (alpha, k, len(lengths), " ".join(str(v) for v in lengths))]
    lines += ["%d %s\n" % (s[2], " ".join("%x" % w for w in s[1].tolist())) for s in states]
    proc = subprocess.run([exe, "windows"], input="".join(lines), capture_output=True, text=True, timeout=600)
    out = proc.stdout.strip().splitlines()
    assert proc.returncode == 0, proc.stderr + (out[-1] if out else "")
    report = json.loads(out[-1])
    assert report == {"states": len(states), "window_draws": len(states) * len(lengths), "window_mismatches": 0,
                      "host_mismatches": 0}
    assert len(out) == len(states) + 1
    return out[:-1]


def assert_equals_numpy(lines, alpha, k, states):
    """what the program drew through the widest window against RandomState from the same state"""
    categories = []
    for line, state in zip(lines, states):
        fields = line.split()
        want = cases.draw(state, alpha, k)
        assert (int(fields[0]), int(fields[1])) == (want.after[2], want.words), (alpha, k, state[2])
        row = np.array([int(v, 16) for v in fields[2:2 + k]], dtype=np.uint64)
        assert np.array_equal(row, want.row.view(np.uint64)), (alpha, k, state[2], want.category)
        key = np.array([int(v, 16) for v in fields[2 + k:]], dtype=np.uint32)
        assert np.array_equal(key, want.after[1]), (alpha, k, state[2], want.category)
        categories.append(want.category)
    return categories


@pytest.mark.parametrize("alpha,k", cases.SHAPES)
def test_windowed_draws_equal_windowless_host_and_numpy(exe, alpha, k):
    states = states_of(alpha, k, range(cases.E))
    lines = run_windows(exe, alpha, k, lengths_of(k), states)
    categories = assert_equals_numpy(lines, alpha, k, states)
    # coverage, from numpy's word accounting of these very states
    assert categories[:cases.E] == [d.category for d in cases.sweep(alpha, k)]
    cases.assert_coverage({(alpha, k): cases.counts(cases.sweep(alpha, k))},
                          {(alpha, k): cases.block_end_subcases(cases.sweep(alpha, k))})
    if k <= 9:
        assert categories[-1] == "exact_end"


def test_sweep_meets_every_category():
    """the classification of the whole sweep: every category is met by the shape that is there for it"""
    counts = {shape: cases.counts(cases.sweep(*shape)) for shape in cases.SHAPES}
    for shape, c in counts.items():
        assert sum(c.values()) == cases.E, shape
    cases.assert_coverage(counts, {shape: cases.block_end_subcases(cases.sweep(*shape)) for shape in cases.SHAPES})
    assert counts[(0.3, 121)]["inside"] == 0 and counts[(0.3, 256)]["window_out"] == 0      # (draws longer than the window / the block)
    for alpha, k in cases.SHAPES:
        if k <= 9:
            d = cases.draw(cases.exact_end_state(alpha, k), alpha, k)
            assert d.category == "exact_end" and d.p + d.words == cases.BLOCK and d.after[2] == cases.BLOCK
            assert np.array_equal(d.after[1], cases.exact_end_state(alpha, k)[1])            # the key is not regenerated


def test_check_program_is_clean_under_asan_and_ubsan(gxx, tmp_path):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtimes here")             # (a trivial program does not link: nothing of ours)
    san = build(gxx, str(tmp_path / "device_stream_check_san"), flags + fma_flags())
    for alpha, k in cases.SHAPES:
        states = states_of(alpha, k, SAN_POSITIONS)
        assert_equals_numpy(run_windows(san, alpha, k, lengths_of(k), states), alpha, k, states)


def test_noise_rows_entry_refuses_null_arguments_without_a_device(pkg):
    """mzmcts_noise_rows (the read-only address of the rows the GPU drew, for tests/test_gpu_noise_stream_edges.py)
    judges its arguments first: no engine, no answer."""
    import ctypes
    import importlib
    lib = importlib.import_module("muzero-hypermodel_amd._native").load()
    rows = ctypes.c_void_p(1)
    assert lib.mzmcts_noise_rows(None, ctypes.byref(rows)) != 0 and lib.mzmcts_noise_rows(None, None) != 0
    assert rows.value == 1
