"""What a finished game reports (csrc/game_outcomes.h, include/mzreplay.h mzreplay_outcomes_reference) without a GPU.

The library's host entry is held, bit for bit, to tests/game_outcomes_reference.py: Python's built-in sum() over the
reward list (the reference's expressions) and numpy.mean / numpy.sum over the list of non-zero root values, at every
length and count of counted values on either side of numpy's 8 and 128, with NaN, -0.0 and all-zero values, for one
player, two alternating players and a player who moves twice in a row, with integer and non-integer rewards.  Two directed
cases show that the order of the additions is visible in the last bit; five deliberate defects of the restatement are each
told from the rule by a named case.  The header is built as a stand-alone program under the address and undefined-behaviour
sanitizers and must give the entry's bits.  The refusals that are decided on the arguments alone, the struct against its
ctypes mirror and numpy record, and FiledGames' three fields.

Refusals that need a store (n < 0 with a live store, a slot outside it, enabling after begin) are in
tests/test_gpu_game_outcomes.py: a store cannot be created without a device."""
import ctypes
import importlib
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import game_outcomes_reference as ref
from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
CASES = ref.make_cases()
DIRECTED = ref.directed_cases()
BY_NAME = {case.name: case for case in CASES + DIRECTED}


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def entry(native, case):
    return native.outcomes_reference(case.rewards, case.to_play, case.root_values)


def test_the_cases_cover_what_the_issue_lists():
    assert sorted({case.n for case in CASES}) == sorted(ref.LENGTHS)
    counted = {(case.n, int(np.count_nonzero(case.root_values))) for case in CASES}
    for n in ref.LENGTHS:
        for c in ref.EDGES:
            if c < n:
                assert (n, c) in counted
    names = " ".join(BY_NAME)
    for word in ref.PLAYERS + ref.REWARDS + ref.SPECIALS:
        assert word in names
    assert any(np.isnan(case.root_values).any() for case in CASES)
    assert any(np.signbit(case.root_values[case.root_values == 0]).any() for case in CASES)


def test_the_written_out_tree_is_numpys_sum():
    """ref.pairwise (used for the split defect) is numpy.sum, bit for bit, on every case's counted values."""
    rng = np.random.default_rng(5)
    lists = [[float(v) for v in case.root_values if v] for case in CASES]
    lists += [rng.standard_normal(n).tolist() for n in (130, 200, 300, 511, 777, 1025)]
    for values in lists:
        if values:
            assert ref.same_bits(ref.pairwise(values), float(np.sum(values))), len(values)


@pytest.mark.parametrize("n", ref.LENGTHS)
def test_the_host_entry_is_pythons_sum_and_numpys_mean(native, n):
    seen = 0
    for case in CASES:
        if case.n == n:
            assert ref.record_matches(entry(native, case), ref.restate(case)), case.name
            seen += 1
    assert seen >= 3 * 2 + len(ref.SPECIALS)


def test_the_directed_cases(native):
    """The order of the additions shows in the last bit: the entry follows numpy's tree and the ascending reward order."""
    case = BY_NAME["pairwise_last_bit"]
    got, want = entry(native, case), ref.restate(case)
    assert ref.record_matches(got, want)
    assert not ref.same_bits(got["value_sum"], sum(float(v) for v in case.root_values))
    case = BY_NAME["reverse_order"]
    got = entry(native, case)
    assert ref.record_matches(got, ref.restate(case))
    assert ref.bits(got["total_reward"]) == ref.bits(sum(case.rewards.tolist()))
    assert ref.bits(got["total_reward"]) != ref.bits(sum(reversed(case.rewards.tolist())))


def test_special_values(native):
    got = entry(native, BY_NAME["n9-nan"])
    assert got["value_count"] == 9 and math.isnan(got["value_sum"])              # `if value` is true for a NaN
    case = BY_NAME["n9-negative_zero"]
    got = entry(native, case)
    assert got["value_count"] == int(np.count_nonzero(case.root_values)) < 9       # -0.0 does not count
    got = entry(native, BY_NAME["n500-all_zero"])
    assert got["value_count"] == 0 and ref.bits(got["value_sum"]) == 0
    one = entry(native, BY_NAME["n129-c129-one-integer"])
    assert ref.bits(one["reward_of_player"][1]) == 0                               # one player: [1] stays +0.0
    assert ref.bits(one["reward_of_player"][0]) == ref.bits(one["total_reward"])


# the case that tells each defect from the rule, and the field it shows in
SEEN_ON = {"sequential": ("pairwise_last_bit", "value_sum"), "zeros_counted": ("n9-c8-one-integer", "value_count"),
           "to_play_i": ("n9-c9-alternating-fraction", "reward_of_player"), "float32": ("n129-c129-one-fraction", "value_sum"),
           # (136 counted values: the halves are 64 + 72, not 68 + 68)
           "split_unrounded": ("n136-c136-one-fraction", "value_sum")}


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_each_defect_is_seen_on_its_named_case(native, defect):
    name, field = SEEN_ON[defect]
    case = BY_NAME[name]
    got = entry(native, case)
    assert ref.record_matches(got, ref.restate(case))
    broken = ref.restate(case, defect=defect)
    assert not ref.record_matches(got, broken), (defect, name)
    if field == "reward_of_player":
        assert any(ref.bits(got[field][p]) != ref.bits(broken[field][p]) for p in (0, 1))
    elif field == "value_count":
        assert int(got[field]) != broken[field]
    else:
        assert ref.bits(got[field]) != ref.bits(broken[field])


# ---- the header under the sanitizers --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("game_outcomes") / "game_outcomes_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "game_outcomes_check.cpp")],
                   check=True)
    return exe


def test_the_header_under_the_sanitizers_gives_the_entrys_bits(native, program, tmp_path):
    cases = CASES + DIRECTED
    source, result = tmp_path / "cases.bin", tmp_path / "out.bin"
    source.write_bytes(ref.pack_cases(cases))
    done = subprocess.run([program, str(source), str(result)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    records = np.fromfile(result, dtype=native.GAME_OUTCOME_DTYPE)
    assert len(records) == len(cases)
    for case, record in zip(cases, records):
        want = entry(native, case)
        assert record.tobytes() == want.tobytes() or (math.isnan(want["value_sum"]) and math.isnan(record["value_sum"])
                                                      and record["value_count"] == want["value_count"]), case.name


# ---- refusals decided on the arguments alone ----------------------------------------------------------------------------------
def test_refusals(native, pkg):
    lib = native.load()
    f64, i8 = native.c_f64_p, ctypes.POINTER(ctypes.c_int8)
    rewards, to_play, values = np.zeros(3), np.zeros(3, dtype=np.int8), np.ones(2)
    out = np.zeros(1, dtype=native.GAME_OUTCOME_DTYPE)
    good = (native.ptr(rewards, f64), native.ptr(to_play, i8), native.ptr(values, f64), out.ctypes.data)
    assert lib.mzreplay_outcomes_reference(2, *good) == 0
    for hole in range(4):
        args = list(good)
        args[hole] = None
        assert lib.mzreplay_outcomes_reference(2, *args) == -1
        assert b"null argument" in lib.mzreplay_last_error(None)
    for n in (0, -1):
        assert lib.mzreplay_outcomes_reference(n, *good) == -1
        assert b"at least one move" in lib.mzreplay_last_error(None)
    with pytest.raises(ValueError, match="one entry more"):
        native.outcomes_reference(np.zeros(2), np.zeros(3), np.zeros(2))
    slots = np.zeros(1, dtype=np.int32)
    assert lib.mzreplay_game_outcomes(None, -1, native.ptr(slots, native.c_i32_p), out.ctypes.data, None) == -1
    assert b"must not be negative" in lib.mzreplay_last_error(None)
    assert lib.mzreplay_game_outcomes(None, 1, native.ptr(slots, native.c_i32_p), out.ctypes.data, None) == -1
    assert b"null argument" in lib.mzreplay_last_error(None)
    assert lib.mzreplay_filer_enable_outcomes(None, 1) == -1
    n_out, out_p = ctypes.c_int32(), ctypes.c_void_p()
    assert lib.mzreplay_filer_sync_outcomes(None, ctypes.byref(n_out), ctypes.byref(out_p)) == -1
    # taking outcomes with the switch off says how to turn it on
    rb = importlib.import_module("muzero-hypermodel_amd.replay_buffer")
    with pytest.raises(RuntimeError, match=r"file_to\(replay_buffer, outcomes=True\)"):
        rb.DeviceFiler(None, None, 4).take_outcomes()


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def test_the_struct_its_ctypes_mirror_and_the_numpy_record(native, tmp_path):
    fields = c_fields("mzreplay.h", "mzreplay_game_outcome")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    prints = "".join(f'    printf(" %zu", offsetof(mzreplay_game_outcome, {f}));\n' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mzreplay.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(mzreplay_game_outcome));\n' + prints + '    printf("\\n");\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, *offsets = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    mirror = native.MzReplayGameOutcome
    assert [name for name, *_ in mirror._fields_] == fields and len(fields) == 5
    assert ctypes.sizeof(mirror) == size == 40 == native.GAME_OUTCOME_DTYPE.itemsize
    assert [getattr(mirror, f).offset for f in fields] == offsets
    assert [native.GAME_OUTCOME_DTYPE.fields[f][1] for f in fields] == offsets
    assert list(native.GAME_OUTCOME_DTYPE.names) == fields


def test_the_named_tuples(pkg):
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    native = importlib.import_module("muzero-hypermodel_amd._native")
    assert sp.FiledGames._fields == ("env_index", "length", "game_id")
    assert sp.GameOutcomes._fields == ("env_index", "length", "game_id", "total_reward", "reward_of_player", "value_sum",
                                       "value_count")
    records = np.zeros(3, dtype=native.GAME_OUTCOME_DTYPE)
    records["value_sum"], records["value_count"] = [1.5, 0.0, -3.0], [2, 0, 3]
    got = sp.GameOutcomes.from_records([0, 1, 2], [4, 5, 6], [7, 8, 9], records)
    assert len(got) == 3 and got.reward_of_player.shape == (3, 2) and got.value_count.dtype == np.int32
    assert got.mean_value[0] == 0.75 and math.isnan(got.mean_value[1]) and got.mean_value[2] == -1.0
    both = sp.GameOutcomes.concatenate([got, got])
    assert len(both) == 6 and both.game_id.tolist() == [7, 8, 9, 7, 8, 9]
    assert len(sp.GameOutcomes.concatenate([])) == 0
