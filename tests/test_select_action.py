"""csrc/select_action.h -- SelfPlay.select_action at any softmax temperature, the sampler the GPU runs behind the searches
of a move batch (visit_count ** (1 / T) by glibc's pow restated, csrc/glibc_libm.h) -- built for the host with g++:

* against HostStream::select_action (this machine's libm): same slot, word count and stream state over the ten visit sets
  of fixture G8 and generated rows of 2 ... 256 children, general temperatures and the unchanged paths, 200 seeds each;
  the restated pow against libm's for every visit count up to 32767 at those exponents;
* against fixture G8 itself (recorded from the reference), T = 0.7 included;
* the two C-ABI entries of the feature: exported, declared, bound; bad arguments are refused without a device.

The device build of the same header is checked on the GPU by tests/test_gpu_temperatures.py."""
import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("select_action") / "select_action_check")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC]
    if "fma" in open("/proc/cpuinfo").read():
        flags.append("-mfma")          # (without it __builtin_fma calls libm's fma: same values, slower)
    subprocess.run([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "select_action_check.cpp"), "-lm"], check=True)
    return exe


@pytest.fixture(scope="module")
def native(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native")


def test_shared_sampler_equals_host_sampler_on_cpu(check_exe, golden):
    fx = golden("g8_select_action")
    rows = [fx[f"set{i}_visits"] for i in range(int(fx["n_sets"]))]
    text = "".join(f"{len(v)} " + " ".join(str(int(x)) for x in v) + "\n" for v in rows)
    proc = subprocess.run([check_exe, "sweep"], input=text, capture_output=True, text=True)
    report = json.loads(proc.stdout.strip().splitlines()[-1])
    assert proc.returncode == 0 and report["mismatches"] == 0 and report["pow_mismatches"] == 0, proc.stdout
    assert report["given_rows"] == 10 and report["rows"] == 10 + 6 * 4 * 3
    assert report["general_cases"] > 100000 and report["cases"] > report["general_cases"]
    assert report["powers"] == 11 * 32768
    assert report["routed"] and report["refused"]


def test_shared_sampler_reproduces_g8(check_exe, golden):
    fx = golden("g8_select_action")
    lines, want = [], []
    for i in range(int(fx["n_sets"])):
        visits, actions = fx[f"set{i}_visits"], fx[f"set{i}_actions"]
        for T in (0, 0.25, 0.5, 1.0, 0.7, float("inf")):
            lines.append(f"{100 + i} {T!r} 12 {len(visits)} " + " ".join(str(int(v)) for v in visits))
            want.append((i, T, actions, fx[f"set{i}_T{T}"].tolist()))
    proc = subprocess.run([check_exe, "rows"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = proc.stdout.strip().splitlines()
    assert len(out) == len(want)
    for line, (i, T, actions, picks) in zip(out, want):
        nums = [int(x) for x in line.split()]
        assert [int(actions[s]) for s in nums[:12]] == picks, (i, T)
        if T == 0:
            assert nums[12] == 0
        elif T != float("inf"):
            assert nums[12] == 24, (i, T)                 # two words per sample, general temperature or not


def _header_arguments(name):
    text = open(os.path.join(ROOT, "include", "mzmcts.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/mzmcts.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_entries_are_exported_declared_and_bound(native):
    lib = native.load()
    kinds = {"mzmcts_engine *": ctypes.c_void_p, "int32_t": ctypes.c_int32, "const uint32_t *": native.c_u32_p,
             "const int32_t *": native.c_i32_p, "const double *": native.c_f64_p, "int32_t *": native.c_i32_p,
             "uint32_t *": native.c_u32_p}
    for name in ("mzmcts_set_device_temperatures", "mzmcts_device_select_action"):
        assert hasattr(lib, name)
        restype, argtypes = native.PROTOTYPES[name]
        declared = [a[:a.rindex("*") + 1] if "*" in a else a.rsplit(" ", 1)[0] for a in _header_arguments(name)]
        assert restype is ctypes.c_int and [kinds[d] for d in declared] == list(argtypes), (name, declared)
    assert lib.mzmcts_abi_version() == native.ABI_VERSION == 2          # an additive change


def test_new_entries_refuse_bad_arguments_without_a_device(native):
    lib = native.load()
    assert lib.mzmcts_set_device_temperatures(None, 1) == native.ERR_INVALID
    seeds = np.arange(3, dtype=np.uint32)
    visits = np.array([[0, 50], [1, 49], [25, 25]], dtype=np.int32)
    slots, words = np.zeros((3, 2), dtype=np.int32), np.zeros(3, dtype=np.uint32)

    def call(seeds_=seeds, n_streams=3, visits_=visits, n=2, temps=(0.7, 0.7, 0.7), draws=2, slots_=slots, words_=words):
        t = np.array(temps, dtype=np.float64)
        return lib.mzmcts_device_select_action(
            None if seeds_ is None else native.ptr(seeds_, native.c_u32_p), n_streams,
            None if visits_ is None else native.ptr(visits_, native.c_i32_p), n,
            None if temps is None else native.ptr(t, native.c_f64_p), draws,
            None if slots_ is None else native.ptr(slots_, native.c_i32_p),
            None if words_ is None else native.ptr(words_, native.c_u32_p))

    for bad in (dict(seeds_=None), dict(visits_=None), dict(temps=None), dict(slots_=None), dict(words_=None),
                dict(n_streams=0), dict(n=0), dict(draws=0), dict(n_streams=-3),
                dict(temps=(0.7, float("nan"), 0.7)), dict(temps=(-1.0, 0.7, 0.7)), dict(temps=(0.7, 0.7, 1e-4)),
                dict(visits_=np.array([[0, 50], [-1, 49], [25, 25]], dtype=np.int32)),
                dict(visits_=np.array([[0, 50], [0, 0], [25, 25]], dtype=np.int32))):     # no visit: 0 / 0 at T = 0.7
        assert call(**bad) == native.ERR_INVALID, bad
    with pytest.raises(RuntimeError):
        native.device_select_action(seeds, visits, float("nan"))
