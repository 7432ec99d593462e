"""Paired moves (include/mzenv.h mzenv_advance_paired), the part that needs no GPU: the slot rule the environment kernels
compile (csrc/paired_moves.h), built for the host and replayed against three single-ply calls per move."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")


def test_paired_slot_rule_equals_three_single_plies_on_cpu(tmp_path):
    """Tic-tac-toe and connect four x expert and random x MuZero first and second x move limits 0, 2, 3 and 5, twelve
    seeded streams each, 60 moves after the settle call: board, side to move, ply counter and stream equal after every
    move, every slot equals the corresponding single-ply call, MuZero is to move after every paired move, the settle call
    plays exactly the opening (slot 1) when MuZero is second and nothing otherwise.  Slot 2 must have been exercised."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "paired_moves_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "paired_moves_check.cpp")], check=True)
    proc = subprocess.run([exe], capture_output=True, text=True)
    report = json.loads(proc.stdout.strip().splitlines()[-1])
    assert proc.returncode == 0, proc.stdout
    assert report["moves"] == 2 * 2 * 2 * 4 * 12 * 60
    assert report["state_mismatches"] == report["slot_mismatches"] == report["invariant_breaks"] == 0, proc.stdout
    assert report["slot2_plies"] > 0 and report["skipped"] > 0 and report["games"] > report["moves"] // 10, proc.stdout
