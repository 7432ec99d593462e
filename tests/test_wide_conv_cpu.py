"""csrc/wide_conv.h (geometry, packed-weight index rule and range rule of the 128-channel layer on 11 x 11 boards) and
plan_wide_conv of csrc/launch_plan.h, built for the host with g++ (tests/wide_conv_check.cpp) and held to a restatement
written here from the layout the kernel's documentation gives."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "wide_conv_check.cpp")

H = W = 11
PW, PP = 12, 157


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    work = tmp_path_factory.mktemp("wide_conv")
    exe = str(work / "wide_conv_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, SOURCE], check=True)

    def run(mode, *args, rows=None, fields=1):
        argv = [exe, mode]
        if rows is not None:
            rows = np.ascontiguousarray(np.asarray(rows).astype(np.int32).reshape(-1, fields))
            path = str(work / f"{mode}.bin")
            with open(path, "wb") as f:
                f.write(np.int32(len(rows)).tobytes())
                f.write(rows.tobytes())
            argv.append(path)
        proc = subprocess.run(argv + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0, proc.stderr
        return json.loads(proc.stdout.strip().splitlines()[-1])
    run.work = work
    return run


def test_geometry_names_the_right_neighbour_or_a_cell_the_fill_never_writes(check):
    g = check("geometry")
    assert (g["P"], g["PW"], g["PP"], g["padded_plane"]) == (121, PW, PP, PP)
    assert (g["cout"], g["max_cin"], g["threads"], g["row_tiles"]) == (128, 160, 512, 8)
    plane_pos, row_pos, tap_offset = g["plane_pos"], g["row_pos"], g["tap_offset"]
    assert tap_offset == [(tap // 3 - 1) * 12 + (tap % 3 - 1) for tap in range(9)]
    written = {}                                        # padded position -> the board cell the fill stores there
    for p in range(121):
        assert plane_pos[p] == (p // W + 1) * PW + p % W + 1
        written[plane_pos[p]] = (p // W, p % W)
    assert len(written) == 121
    assert len(row_pos) == 128 and row_pos[:121] == plane_pos
    for p, tap in itertools.product(range(121), range(9)):
        y, x = p // W + tap // 3 - 1, p % W + tap % 3 - 1
        at = row_pos[p] + tap_offset[tap]
        assert 0 <= at < PP
        if 0 <= y < H and 0 <= x < W:
            assert written[at] == (y, x)               # the right neighbour
        else:
            assert at not in written                    # the zero border
    for m in range(121, 128):                           # padding rows of the last tile: a zero cell, all reads inside
        assert row_pos[m] == g["zero_pos"] and row_pos[m] not in written
        for tap in range(9):
            assert 0 <= row_pos[m] + tap_offset[tap] < PP
    # the staging tile [128][ldm] of the epilogue holds every position and lies inside its bytes
    assert g["stage_ldm"] >= 121 and g["stage_bytes"] == 4 * 128 * g["stage_ldm"]
    assert g["lds_bytes"] == [max(PP * 2 * (32 * -(-cin // 32) + 8) * 2, g["stage_bytes"]) for cin in range(1, 161)]


def test_range_predicate(check):
    f32 = lambda values: np.asarray(values, dtype=np.float32).view(np.int32)
    below = np.nextafter(np.float32(8188.0), np.float32(0.0))
    cases = [(8188.0, 0), (below, 1), (-8188.0, 0), (-below, 1), (np.inf, 0), (-np.inf, 0), (np.nan, 0), (0.0, 1), (-0.0, 1),
             (1e-45, 1), (-1e-45, 1), (1.1754942e-38, 1), (3e7, 0), (8187.9, 1), (1.0, 1), (3.4e38, 0)]
    bits = f32([c[0] for c in cases]).tolist() + [0x7fc00001, -1]      # two more NaN patterns (-1 = 0xffffffff)
    got = check("range", rows=bits)
    assert got == [c[1] for c in cases] + [0, 0]


def plan_restated(batch, cin, cout, h, w, stage_bytes):
    """rc, groups, cph, grid, block, lds, supported"""
    supported = int(h == 11 and w == 11 and cout == 128 and 1 <= cin <= 160)
    if not supported or batch < 0 or batch > 0x3fffffff:
        return [-1, 0, 0, 0, 0, 0, supported]
    groups = -(-cin // 32)
    cph = 32 * groups + 8
    lds = max(157 * 2 * cph * 2, stage_bytes)
    if batch == 0:
        return [0, groups, cph, 0, 512, lds, supported]
    assert lds <= 160 * 1024
    return [0, groups, cph, batch, 512, lds, supported]


def test_plan_equals_its_restatement(check):
    stage = check("geometry")["stage_bytes"]
    rows = [[batch, cin, cout, h, w] for cin in range(0, 162) for cout in (16, 64, 128)
            for h, w in ((3, 3), (6, 7), (11, 11), (11, 12)) for batch in (-1, 0, 1, 257, 0x3fffffff, 0x40000000)]
    said = check("plan", rows=rows, fields=5)
    assert said == {"rows": len(rows), "fields": 7}
    got = np.fromfile(str(check.work / "plan.bin.out"), dtype=np.int64).reshape(len(rows), 7)
    want = np.array([plan_restated(*row, stage) for row in rows], dtype=np.int64)
    differ = np.flatnonzero(np.any(got != want, axis=1))
    assert differ.size == 0, (rows[differ[0]], got[differ[0]].tolist(), want[differ[0]].tolist())
    launched = (got[:, 0] == 0) & (np.array(rows)[:, 0] > 0)
    assert launched.sum() == 160 * 3 and np.all(got[launched, 3] == np.array(rows)[launched, 0]) and np.all(got[launched, 4] == 512)

    # LDS bytes by hand: 157 positions x 2 halves x (32 groups + 8) channels x 2 bytes, or the [128][124] float staging tile
    def lds(cin):
        check("plan", rows=[[5, cin, 128, 11, 11]], fields=5)
        return int(np.fromfile(str(check.work / "plan.bin.out"), dtype=np.int64)[5])
    assert stage == 63488
    assert lds(3) == 63488                              # one group: 157 x 2 x 40 x 2 = 25120 < the staging tile
    assert lds(128) == 85408                            # four groups: 157 x 2 x 136 x 2
    assert lds(129) == 105504 and lds(160) == 105504    # five groups: 157 x 2 x 168 x 2 -- 105 KB of 160


@pytest.mark.parametrize("cin", [1, 3, 32, 33, 129, 160])
def test_pack_index_is_a_bijection_with_zeros_exactly_in_the_padding(check, cin):
    cout = 128
    path = str(check.work / f"pack{cin}.bin")
    said = check("pack", cin, cout, path)
    groups = -(-cin // 32)
    assert said["halfs"] == said["split_halfs"] == (9 * groups + 2) * 2 * 4 * cout * 8
    rows = np.fromfile(path, dtype=np.int32).reshape(said["halfs"], 5)
    n, ci, tap, q, zero = rows.T
    # the layout [9 groups + 2 spare][2 q][4 kk][cout][8 j], restated
    i = np.arange(said["halfs"])
    j, nn, kk, qq, tg = i % 8, i // 8 % cout, i // 8 // cout % 4, i // 8 // cout // 4 % 2, i // 8 // cout // 8
    assert np.array_equal(n, nn) and np.array_equal(q, qq) and np.array_equal(tap, tg // groups)
    assert np.array_equal(ci, (tg % groups) * 32 + 8 * kk + j)
    assert np.array_equal(zero.astype(bool), (tap >= 9) | (ci >= cin))
    live = rows[zero == 0][:, :4]
    assert len(live) == cout * cin * 9 * 2                                         # every half of every weight ...
    key = ((live[:, 0] * cin + live[:, 1]) * 9 + live[:, 2]) * 2 + live[:, 3]
    assert np.array_equal(np.sort(key), np.arange(cout * cin * 9 * 2))             # ... exactly once
