"""csrc/launch_plan.h -- the one place a board-network launch is decided (which kernel a tower, a convolution or a set of
heads gets, samples per workgroup, LDS bytes, grid) -- built for the host with g++ (tests/launch_plan_check.cpp) and held
to restatements that were written from the launchers the header replaced:

* heads: tests/net_head_cases.py (dispatch, mfma_form, mfma_total, wave_total, wave_split, samples_per_round) on every
  entry of HEAD_CASES and over EVERY ordered launch of one, two and three heads out of the product of shapes at the
  kernels' limits (19 million launches, enumerated by the check program and compared as arrays);
* towers and the per-layer convolution: tests/board_tower_cases.py (tower_plan, conv_plan) over the full product of
  shapes, switches and batches, and every id of FP32_FORMS, SPLIT_FORMS and MANY -- the names the GPU tests carry -- against
  the kernel and template arguments the header gives it at every cin0 and batch tests/test_gpu_board_towers.py runs;
* the gate invariant: the split launch's workgroup, the fp32 launch's gate_samples and mzmcts_board_tower_blocks are one
  number, so the gate buffer Python sizes is the buffer both kernels index;
* LDS figures worked out by hand from the kernels' layouts.

The check program is built once more with -fsanitize=address,undefined and driven through every mode."""
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import board_tower_cases as towers
import net_head_cases as heads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "launch_plan_check.cpp")

TOWER_IN = ("batch", "cin0", "channels", "h", "w", "n_layers", "split", "const_plane", "gated", "n_heads", "cols_on", "aligned",
            "split_boards", "layer1_skip", "bad_layer")
TOWER_OUT = ("rc", "kernel", "nt", "sb", "waves", "samples", "cp0", "cp1", "grid", "block", "lds", "gate_samples")
CONV_OUT = ("rc", "nt", "sb", "grid", "block", "lds")
HEADS_KERNELS = ("none", "cols", "mfma", "wave")                       # HeadsKernel, in the header's order
BOARDS = ((3, 3), (6, 6), (6, 7))


def _runner(work, exe):
    def run(mode, rows, fields=1):
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, fields))
        path = str(work / f"{mode}.bin")
        with open(path, "wb") as f:
            f.write(np.int32(len(rows)).tobytes())
            f.write(rows.tobytes())
        proc = subprocess.run([exe, mode, path], capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0, proc.stderr
        said = json.loads(proc.stdout.strip().splitlines()[-1])
        if mode == "sizes":
            return said
        if mode == "heads_product":
            return np.fromfile(path + ".out", dtype=np.int32).reshape(said["rows"], said["fields"])
        assert said["rows"] == len(rows)
        return np.fromfile(path + ".out", dtype=np.int64).reshape(len(rows), said["fields"])
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    work = tmp_path_factory.mktemp("launch_plan")
    exe = str(work / "launch_plan_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, SOURCE], check=True)
    return _runner(work, exe)


def tower_rows(**columns):
    """Broadcasts the named inputs (defaults: one fp32 layer, nothing switched) to int32 rows in TOWER_IN's order."""
    defaults = dict(n_layers=1, split=0, const_plane=0, gated=0, n_heads=0, cols_on=1, aligned=1, split_boards=2, layer1_skip=0,
                    bad_layer=-1)
    defaults.update(columns)
    arrays = np.broadcast_arrays(*[np.asarray(defaults[k], dtype=np.int64).ravel() for k in TOWER_IN])
    return np.stack(arrays, axis=1)


def tower_header(check, rows):
    out = check("tower", rows, len(TOWER_IN))
    return {k: out[:, i] for i, k in enumerate(TOWER_OUT)}


def tower_restated(rows):
    named = {k: rows[:, i] for i, k in enumerate(TOWER_IN)}
    named.pop("bad_layer")
    return towers.tower_plan(**named)


def assert_same_plans(got, want, rows, names):
    for k in names:
        differ = np.flatnonzero(got[k] != want[k])
        assert differ.size == 0, (k, len(differ), rows[differ[0]].tolist(), int(got[k][differ[0]]), int(want[k][differ[0]]))


# ---- towers: the ids of the GPU tests ------------------------------------------------------------------------------------------
def named_launch(form_id):
    """The kernel and template arguments a GPU test id names: (kernel, {field: value})."""
    m = re.match(r"launch_board_tower(_split|_cols|_patch66)?(?:<([\d,]+)>)?(<heads>)?", form_id)
    kind, nums = m.group(1), tuple(int(v) for v in m.group(2).split(",")) if m.group(2) else ()
    if kind == "_split":
        return "split", dict(h=nums[0], w=nums[1], sb=nums[2], waves=nums[3] if len(nums) > 3 else 8, samples=nums[2])
    if kind == "_cols":
        return ("cols+heads" if m.group(3) else "cols"), dict(samples=64)
    if kind == "_patch66":
        return "patch", dict(samples=16)
    return "row", dict(nt=nums[0], h=nums[1], w=nums[2], sb=nums[3], samples=nums[3])


def around(*units):
    """The batches exercise() of tests/test_gpu_board_towers.py runs a form with: 1 and k S - 1, k S, k S + 1 around its units."""
    out = {1}
    for s in units:
        if s:
            out |= {s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1}
    return sorted(b for b in out if b >= 1)


GPU_LAYERS = (1, 2, 3, 5, 16)                # standard_cases and deep_case
FEW_OF = {(1, 6, 7, 6): (1, 6, 7, 4), (1, 6, 6, 3): (1, 6, 6, 4), (1, 3, 3, 14): (1, 3, 3, 16)}


def assert_named(plan, form_id, h, w, what):
    kernel, fields = named_launch(form_id)
    fields.setdefault("h", h)
    fields.setdefault("w", w)
    assert np.all(plan["rc"] == 0), (form_id, what)
    assert {towers.KERNELS[k] for k in plan["kernel"]} == {kernel}, (form_id, what)
    for k, v in fields.items():
        got = plan[k] if k in plan else np.full(1, fields[k])
        assert np.all(got == v), (form_id, what, k, v, np.unique(got))


@pytest.mark.parametrize("form", towers.FP32_FORMS, ids=[f[0] for f in towers.FP32_FORMS])
def test_fp32_form_ids_name_the_kernel_the_plan_gives(check, form):
    name, channels, h, w, cols, S, wide, cin0s = form
    cin0, batch, n_layers = (a.ravel() for a in np.meshgrid(cin0s, around(S, wide), GPU_LAYERS, indexing="ij"))
    rows = tower_rows(batch=batch, cin0=cin0, channels=channels, h=h, w=w, n_layers=n_layers, cols_on=int(cols != "off"))
    plan = tower_header(check, rows)
    plan["h"], plan["w"] = rows[:, 3], rows[:, 4]
    assert_named(plan, name, h, w, "every cin0, batch and depth")
    assert np.all(plan["samples"] == (wide or S))
    assert np.all(plan["grid"] == -(-batch // plan["samples"]))


@pytest.mark.parametrize("form", towers.SPLIT_FORMS, ids=[f[0] for f in towers.SPLIT_FORMS])
def test_split_form_ids_name_the_kernel_the_plan_gives(check, form):
    name, h, w, S, cin0s = form
    for const_plane in (0, 1):
        cin0, batch, n_layers = (a.ravel() for a in np.meshgrid(cin0s, around(S), GPU_LAYERS, indexing="ij"))
        rows = tower_rows(batch=batch, cin0=cin0, channels=64, h=h, w=w, n_layers=n_layers, split=1, const_plane=const_plane)
        plan = tower_header(check, rows)
        plan["h"], plan["w"] = rows[:, 3], rows[:, 4]
        assert_named(plan, name, h, w, f"const_plane {const_plane}")
        assert np.all(plan["samples"] == S) and np.all(plan["block"] == 64 * plan["waves"])


@pytest.mark.parametrize("form", towers.MANY, ids=[f[0] for f in towers.MANY])
def test_many_form_ids_name_the_kernel_on_both_sides_of_the_switch(check, form):
    name, h, w, cols, cin0 = form
    for batch in (16383, 16384, 16385):
        rows = tower_rows(batch=batch, cin0=cin0, channels=16, h=h, w=w, n_layers=(2, 3, 5), cols_on=int(cols != "off"))
        plan = tower_header(check, rows)
        plan["h"], plan["w"] = rows[:, 3], rows[:, 4]
        kernel, fields = named_launch(name)
        if batch < 16384 and kernel == "row":
            few = FEW_OF[(fields["nt"], fields["h"], fields["w"], fields["sb"])]
            assert_named(plan, "launch_board_tower<%d,%d,%d,%d>" % few, h, w, batch)
        else:
            assert_named(plan, name, h, w, batch)


def test_heads_inside_a_tower_launch_are_the_cols_kernel_only(check):
    rows = tower_rows(batch=(1, 17, 65), cin0=17, channels=16, h=3, w=3, n_layers=5, n_heads=3)
    plan = tower_header(check, rows)
    assert_named(plan, "launch_board_tower_cols<heads>", 3, 3, "three heads")
    assert np.all(plan["lds"] == 69312)
    refused = tower_rows(batch=5, cin0=(17, 17, 17, 20, 65), channels=(16, 16, 16, 16, 64), h=(3, 6, 6, 3, 6), w=(3, 6, 7, 3, 7),
                         n_heads=1, cols_on=(0, 1, 1, 1, 1))
    assert np.all(tower_header(check, refused)["rc"] == -1)           # MZ_TOWER_COLS=off, 6 x 6, 6 x 7, cin0 = 20, 64 channels


def test_split_boards_one_and_four(check):
    """MZ_SPLIT_BOARDS = 1 and 4: board_tower_split_kernel<6,7,1,2> and <6,7,4,8>, which no GPU test reaches; anything else
    is the default of 2 boards on 4 wavefronts; 6 x 6 boards do not listen to it."""
    for boards, (sb, waves) in {1: (1, 2), 4: (4, 8), 2: (2, 4), 3: (2, 4), 0: (2, 4), 8: (2, 4)}.items():
        plan = tower_header(check, tower_rows(batch=(1, 9), cin0=65, channels=64, h=6, w=7, n_layers=5, split=1, const_plane=1,
                                              split_boards=boards))
        assert np.all(plan["rc"] == 0) and np.all(plan["kernel"] == towers.KERNELS.index("split"))
        assert np.all(plan["sb"] == sb) and np.all(plan["waves"] == waves) and np.all(plan["block"] == 64 * waves)
        assert np.all(plan["gate_samples"] == sb) and plan["grid"].tolist() == [1, -(-9 // sb)]
        other = tower_header(check, tower_rows(batch=9, cin0=65, channels=64, h=6, w=6, split=1, split_boards=boards))
        assert (other["sb"][0], other["waves"][0]) == (4, 8)


# ---- towers and convolutions: restatement == header over the full product -----------------------------------------------------
def test_tower_plan_equals_its_restatement_over_the_full_product(check):
    axes = dict(channels=(16, 64), board=range(3), cin0=range(1, 81), n_layers=(1, 2, 5, 16), split=(0, 1), const_plane=(0, 1),
                gated=(0, 1), n_heads=range(4), cols_on=(0, 1), batch=range(10))
    grid = dict(zip(axes, (a.ravel() for a in np.meshgrid(*axes.values(), indexing="ij"))))
    h, w = np.array(BOARDS)[grid.pop("board")].T
    which = grid.pop("batch")
    shape = dict(grid, h=h, w=w)
    S = towers.tower_plan(batch=1, **shape)["samples"]                # (0 where the arguments are refused: batch -1 follows)
    batch = np.choose(which, [0 * S, 0 * S + 1, S - 1, S, S + 1, 0 * S + 16383, 0 * S + 16384, 0 * S + 16385,
                              0 * S + 0x3fffffff, 0 * S + 0x40000000])
    rows = tower_rows(batch=batch, **shape)
    assert len(rows) == 2 * 3 * 80 * 4 * 2 * 2 * 2 * 4 * 2 * 10
    got, want = tower_header(check, rows), tower_restated(rows)
    assert_same_plans(got, want, rows, TOWER_OUT)
    launched = (got["rc"] == 0) & (batch > 0)
    assert launched.sum() > 100000 and np.all(got["lds"][launched] <= 160 * 1024)
    whole = launched & ((rows[:, 8] == 0) | (rows[:, 6] == 1))         # (a gated fp32 launch is a fixed grid of at most 256)
    assert np.all(got["grid"][whole] * got["samples"][whole] >= batch[whole])


def test_tower_plan_switches_outside_the_product(check):
    """Unaligned packed weights (the patch kernel falls back to the row tile), a layer-1 skip over the constant plane, a
    layer whose descriptor states another cin, depths outside 1..16, a negative batch: header == restatement, and the
    return codes by name."""
    axes = dict(channels=(16, 64), board=range(3), cin0=(1, 2, 16, 17, 20, 64, 65, 80), n_layers=(0, 1, 2, 3, 16, 17), split=(0, 1),
                const_plane=(0, 1), aligned=(0, 1), layer1_skip=(0, 1), batch=(-1, 0, 5, 16384))
    grid = dict(zip(axes, (a.ravel() for a in np.meshgrid(*axes.values(), indexing="ij"))))
    h, w = np.array(BOARDS)[grid.pop("board")].T
    rows = tower_rows(h=h, w=w, **grid)
    got, want = tower_header(check, rows), tower_restated(rows)
    assert_same_plans(got, want, rows, TOWER_OUT)

    def rc(**kw):
        return int(tower_header(check, tower_rows(**kw))["rc"][0])
    patch = tower_header(check, tower_rows(batch=(5, 5, 16384), cin0=16, channels=16, h=6, w=6, aligned=(1, 0, 0)))
    assert [towers.KERNELS[k] for k in patch["kernel"]] == ["patch", "row", "row"] and patch["sb"].tolist() == [0, 4, 3]
    assert rc(batch=5, cin0=64, channels=64, h=6, w=7, n_layers=3, split=1, const_plane=1, layer1_skip=1) == -1
    assert rc(batch=5, cin0=65, channels=64, h=6, w=7, n_layers=3, split=1, const_plane=1, layer1_skip=1) == 0
    assert rc(batch=5, cin0=64, channels=64, h=6, w=7, n_layers=3, split=1, const_plane=0, layer1_skip=1) == 0
    assert rc(batch=5, cin0=1, channels=64, h=6, w=7, split=1, const_plane=1) == -1
    for bad_layer in (0, 1, 4):
        assert rc(batch=5, cin0=17, channels=16, h=3, w=3, n_layers=5, bad_layer=bad_layer) == -1
        assert rc(batch=5, cin0=65, channels=64, h=6, w=7, n_layers=5, split=1, bad_layer=bad_layer) == -1
    assert rc(batch=5, cin0=17, channels=16, h=3, w=3, n_layers=5, bad_layer=5) == 0
    assert rc(batch=5, cin0=17, channels=16, h=3, w=3, gated=1) == -1            # (a gate: the 64-channel pair only)
    assert rc(batch=5, cin0=65, channels=16, h=6, w=7, split=1) == -1
    for split in (0, 1):                                                         # 64 channels on 3 x 3: refused, but for an empty batch
        assert rc(batch=5, cin0=65, channels=64, h=3, w=3, split=split) == -1
        assert rc(batch=0, cin0=65, channels=64, h=3, w=3, split=split) == 0
    assert rc(batch=5, cin0=80, channels=64, h=6, w=7, split=1, split_boards=4) == -1    # 183088 bytes
    assert rc(batch=0, cin0=80, channels=64, h=6, w=7, split=1, split_boards=4) == 0     # (an empty batch: before any size check)
    assert rc(batch=5, cin0=80, channels=64, h=6, w=7, split=1) == 0
    assert rc(batch=5, cin0=81, channels=64, h=6, w=7) == -1 and rc(batch=5, cin0=17, channels=32, h=3, w=3) == -1
    assert rc(batch=5, cin0=17, channels=16, h=6, w=5) == -1


def test_conv_plan_equals_its_restatement_and_names_six_forms(check):
    axes = dict(cout=(16, 64), board=range(3), cin=range(0, 82), batch=(-1, 0, 1, 3, 4, 5, 31, 32, 33, 16384, 0x3fffffff, 0x40000000))
    grid = dict(zip(axes, (a.ravel() for a in np.meshgrid(*axes.values(), indexing="ij"))))
    h, w = np.array(BOARDS)[grid.pop("board")].T
    rows = np.stack([grid["batch"], grid["cin"], grid["cout"], h, w], axis=1)
    out = check("conv", rows, 5)
    got = {k: out[:, i] for i, k in enumerate(CONV_OUT)}
    want = towers.conv_plan(grid["batch"], grid["cin"], grid["cout"], h, w)
    assert_same_plans(got, want, rows, CONV_OUT)
    ok = got["rc"] == 0
    forms = {(int(n), int(a), int(b), int(s)) for n, a, b, s in zip(got["nt"][ok], h[ok], w[ok], got["sb"][ok])}
    assert forms == {(4, 6, 7, 4), (1, 6, 7, 8), (4, 6, 6, 4), (1, 6, 6, 16), (4, 3, 3, 16), (1, 3, 3, 32)}
    assert np.all(got["rc"][(grid["cin"] < 1) | (grid["cin"] > 80) | (grid["batch"] < 0) | (grid["batch"] > 0x3fffffff)] == -1)
    # launch_board_conv's max(planes, stage): with one group of input channels the 64-channel staging tile is the larger
    narrow = check("conv", [[5, 16, 64, 6, 7], [5, 32, 64, 6, 7], [5, 33, 64, 6, 7]], 5)[:, 5].tolist()
    stage = 4 * (64 * (4 * 42 + 1) + 128)
    assert narrow == [stage, stage, 4 * 4 * 65 * 52] and 4 * 4 * 65 * 36 < stage < narrow[2]
    assert np.all(got["lds"][ok & (grid["batch"] > 0)] <= 160 * 1024) and ok.sum() > 2 * 3 * 80 * 8


# ---- the gate invariant ----------------------------------------------------------------------------------------------------------
def parent_block_samples(batch, channels, h, w, split_boards):
    """tower_block_samples as mzmcts_board_tower_blocks had it before the plan: 0 = no answer."""
    many = batch >= 16384
    if (h, w) == (6, 7):
        return (split_boards if split_boards in (4, 2, 1) else 2) if channels == 64 else 0
    if (h, w) == (6, 6):
        return 4 if channels == 64 else (3 if many else 4)
    return 16 if channels == 64 else (14 if many else 16)


def test_blocks_gate_samples_and_the_split_grid_are_one_number(check):
    """Every 64-channel shape that admits a gate (6 x 6 and 6 x 7 boards; cin0 1..80, 1 / 2 / 5 / 16 layers, with and without
    a constant plane, every MZ_SPLIT_BOARDS): gate_samples of the fp32 plan is the split plan's samples per workgroup,
    mzmcts_board_tower_blocks x that number covers the batch, and blocks is the split launch's grid."""
    batches = (1, 2, 3, 4, 5, 7, 8, 9, 1029, 16383, 16384, 16385, 0x3fffffff)
    axes = dict(board=(1, 2), split_boards=(1, 2, 4, 3), cin0=range(1, 81), n_layers=(1, 2, 5, 16), const_plane=(0, 1), batch=batches)
    grid = dict(zip(axes, (a.ravel() for a in np.meshgrid(*axes.values(), indexing="ij"))))
    h, w = np.array(BOARDS)[grid.pop("board")].T
    const_plane, batch, boards, cin0 = grid.pop("const_plane"), grid["batch"], grid["split_boards"], grid["cin0"]
    common = dict(grid, channels=64, h=h, w=w)
    split = tower_header(check, tower_rows(split=1, const_plane=const_plane, gated=1, **common))
    fp32 = tower_header(check, tower_rows(gated=1, **common))
    ungated = tower_header(check, tower_rows(**common))
    blocks = check("blocks", np.stack([batch, 0 * batch + 64, h, w, boards], axis=1), 5)[:, 0]
    admitted = ~((const_plane == 1) & (cin0 < 2))                     # (a constant plane needs a second one to convolve)
    launched = split["rc"] == 0
    # over 160 KB in the split form: 6 x 7 at 4 boards with more than 64 convolved input channels
    too_large = (w == 7) & (boards == 4) & (cin0 - const_plane > 64)
    assert np.array_equal(launched, admitted & ~too_large) and np.all(fp32["rc"] == 0)
    assert np.all(fp32["gate_samples"][admitted] == split["samples"][admitted])
    assert np.all(split["gate_samples"][admitted] == split["samples"][admitted]) and np.all(split["samples"][admitted] > 0)
    assert np.all(blocks * fp32["gate_samples"] >= batch) and np.all((blocks - 1) * fp32["gate_samples"] < batch)
    assert np.all(blocks[launched] == split["grid"][launched])
    assert np.all(fp32["grid"] == np.minimum(-(-batch // 4), 256)) and np.all(ungated["grid"] == -(-batch // 4))


def test_blocks_answers_as_before(check):
    rows = [[b, c, h, w, boards] for b in (-1, 0, 1, 15, 16, 17, 16383, 16384, 16385, 0x40000000) for c in (16, 64, 32)
            for h, w in BOARDS + ((6, 5),) for boards in (1, 2, 4, 7)]
    got = check("blocks", rows, 5)[:, 0]
    for (b, c, h, w, boards), blocks in zip(rows, got):
        sb = parent_block_samples(b, c, h, w, boards) if (c in (16, 64) and (h, w) in BOARDS) else 0
        assert blocks == (-1 if (b < 0 or sb <= 0) else -(-b // sb)), (b, c, h, w, boards)
    assert check("blocks", [[100, 16, 6, 7, 2]], 5)[0, 0] == -1                 # 16-channel 6 x 7: no answer, as ever


# ---- LDS figures worked out by hand ------------------------------------------------------------------------------------------------
def test_lds_anchor_rows(check):
    def lds(**kw):
        plan = tower_header(check, tower_rows(**kw))
        return int(plan["lds"][0]), int(plan["rc"][0]), plan

    def row(nt_h_w_sb, cin0, batch=5, **kw):
        nt, h, w, sb = nt_h_w_sb
        size, rc, plan = lds(batch=batch, cin0=cin0, channels=16 * nt, h=h, w=w, n_layers=5, cols_on=0, **kw)
        assert (towers.KERNELS[plan["kernel"][0]], plan["nt"][0], plan["sb"][0]) == ("row", nt, sb)
        return size, rc, (int(plan["cp0"][0]), int(plan["cp1"][0]))

    assert row((4, 6, 7, 4), 65) == row((4, 6, 7, 4), 80) == (158128, 0, (84, 68))
    assert row((4, 6, 6, 4), 65)[:2] == (138672, 0)
    assert row((1, 3, 3, 16), 17)[:2] == (75456, 0) and row((1, 3, 3, 14), 17, batch=16384)[:2] == (66024, 0)
    assert row((1, 6, 6, 4), 17)[:2] == (51120, 0) and row((1, 6, 6, 3), 17, batch=16384)[:2] == (38340, 0)
    assert row((1, 6, 7, 4), 17)[:2] == (58288, 0) and row((1, 6, 7, 6), 17, batch=16384)[:2] == (87432, 0)
    assert row((1, 6, 7, 6), 80, batch=16384)[:2] == (162312, 0)                # fits: 160 KB = 163840

    split = dict(batch=5, channels=64, n_layers=5, split=1)
    assert lds(cin0=65, h=6, w=7, const_plane=1, **split)[:2] == (74904, 0)
    assert lds(cin0=65, h=6, w=7, const_plane=0, **split)[:2] == (91544, 0)
    assert lds(cin0=65, h=6, w=7, const_plane=1, split_boards=1, **split)[:2] == (37452, 0)
    assert lds(cin0=65, h=6, w=6, const_plane=1, **split)[:2] == (131376, 0)
    assert lds(cin0=80, h=6, w=6, const_plane=0, **split)[:2] == (160560, 0)    # fits
    assert lds(cin0=80, h=6, w=7, const_plane=0, split_boards=4, **split)[:2] == (183088, -1)

    sizes = check("sizes", [])
    assert sizes["row_tile_4_3_3_16"] == 182976 and sizes["split_3_3_16"] == 193728     # why 64 channels on 3 x 3 have no tower
    assert lds(batch=5, cin0=17, channels=16, h=3, w=3)[:2] == (41472, 0)
    assert lds(batch=5, cin0=17, channels=16, h=3, w=3, n_heads=2)[:2] == (69312, 0)
    assert lds(batch=5, cin0=17, channels=16, h=6, w=6)[:2] == (77056, 0) and sizes["patch_boards"] == 16
    assert 4 * (4 * sizes["col_wave_floats"] + sizes["col_head_w1_floats"]) == 50752

    def head_launch(shape, cols_on=1, use_mfma=1, batch=100):
        out = check("heads", [[1, batch, cols_on, use_mfma] + list(shape) + [0] * 10], 19)[0]
        return HEADS_KERNELS[out[1]], int(out[2]), int(out[3])
    assert head_launch((16, 9, 16, 8, 21)) == ("cols", 50752, 1)
    assert head_launch((64, 42, 2, 64, 21)) == ("mfma", 68864, 2)
    assert head_launch((4, 42, 6, 48, 7)) == ("mfma", 129280, 1)
    assert head_launch((64, 42, 2, 64, 21), use_mfma=0)[:2] == ("wave", 74144)


# ---- heads ------------------------------------------------------------------------------------------------------------------------
def heads_rows(launches):
    """[(shapes, batch, cols_off, use_mfma)] -> int32 rows of the check program."""
    rows = []
    for shapes, batch, cols_off, use_mfma in launches:
        flat = [v for s in shapes for v in s] + [0] * (5 * (3 - len(shapes)))
        rows.append([len(shapes), batch, int(not cols_off), int(use_mfma)] + flat)
    return rows


def assert_heads(check, launches):
    """Kernel, per-head forms and layouts, LDS bytes, samples per round and grid of every launch against net_head_cases."""
    out = check("heads", heads_rows(launches), 19)
    for (shapes, batch, cols_off, use_mfma), got in zip(launches, out):
        what = (shapes, batch, cols_off, use_mfma)
        rc, kernel, lds, per_cu, grid_x, grid_y, block = (int(v) for v in got[:7])
        want = heads.dispatch(shapes, cols_off=cols_off)
        if not use_mfma and want == "mfma":                            # MZ_HEADS_WAVE_PER_SAMPLE: the matrix-core kernel is skipped
            want = "wave" if 4 * max(heads.wave_total(s) for s in shapes) <= heads.LDS_LIMIT else "none"
        assert HEADS_KERNELS[kernel] == want and rc == (-1 if want == "none" else 0), (what, HEADS_KERNELS[kernel], want)
        for h, s in enumerate(shapes):
            form, mfma_total, wave_total, split = tuple(got[7 + 7 * h:11 + 7 * h]), got[11 + 7 * h], got[12 + 7 * h], got[13 + 7 * h]
            assert (mfma_total, wave_total, split) == (heads.mfma_total(s), heads.wave_total(s), heads.wave_split(s[3])), what
            assert form == (heads.mfma_form(s) if want == "mfma" else (0, 0, 0, 0)), what
        if want == "none":
            continue
        assert grid_y == len(shapes) and block == 256
        if want == "cols":
            assert (lds, grid_x) == (50752, -(-batch // 64)), what
            continue
        total = heads.mfma_total if want == "mfma" else heads.wave_total
        per_workgroup = heads.K_HEAD_WAVES * (heads.TILE if want == "mfma" else 1)
        assert lds == 4 * max(total(s) for s in shapes), what
        assert 256 * per_cu * per_workgroup == heads.samples_per_round(shapes, want), what
        assert grid_x == min(-(-batch // per_workgroup), 256 * per_cu), what


def test_every_head_case_reaches_the_kernel_and_form_it_names(check):
    launches = [(case["shapes"], batch, case["cols_off"], True) for case in heads.HEAD_CASES.values() for batch in (0,) + tuple(case["batches"])]
    assert_heads(check, launches)
    out = check("heads", heads_rows(launches), 19)
    at = 0
    for case in heads.HEAD_CASES.values():
        for _ in (0,) + tuple(case["batches"]):
            assert HEADS_KERNELS[out[at, 1]] == case["kernel"], case
            at += 1
    reached = {tuple(out[i, 7 + 7 * h:11 + 7 * h]) for i, launch in enumerate(launches) if HEADS_KERNELS[out[i, 1]] == "mfma"
               for h in range(len(launch[0]))}
    assert reached == heads.ALL_MFMA_FORMS


HEAD_AXES = dict(C=(1, 3, 4, 16, 17, 63, 64, 65), P=(1, 9, 36, 42), R=(1, 16, 17), Hd=(1, 16, 17, 32, 33, 64, 65), O=(1, 32, 33, 65))


def test_heads_plan_over_the_product_of_shapes(check):
    """Every single head of the product with the board-column form on and off, with and without the matrix-core kernel; then
    launches of two and three heads of mixed shapes: every shape of the product leads a pair and a triple whose other heads
    are drawn (seeded) from the shapes sharing its board, C and P."""
    shapes = list(itertools.product(*HEAD_AXES.values()))
    assert len(shapes) == 8 * 4 * 3 * 7 * 4
    launches = [([s], batch, cols_off, use_mfma) for s in shapes for cols_off in (False, True) for use_mfma in (True, False)
                for batch in ((0, 1, 65, 40000) if use_mfma else (65,))]
    rs = np.random.RandomState(11)
    tails = list(itertools.product(HEAD_AXES["R"], HEAD_AXES["Hd"], HEAD_AXES["O"]))
    for s in shapes:
        for n in (2, 3):
            others = [s[:2] + tails[i] for i in rs.randint(0, len(tails), size=n - 1)]
            order = rs.permutation(n)
            launches.append(([([s] + others)[i] for i in order], int(rs.choice([1, 17, 5000, 70000])), bool(rs.randint(2)), True))
    # the board-column heads among themselves (the product holds few of them)
    cols = [(16, 9, r, hd, o) for r in (1, 16) for hd in (1, 16) for o in (1, 32)]
    launches += [(list(c), 130, cols_off, True) for c in itertools.product(cols, cols[::3], cols[1::4]) for cols_off in (False, True)]
    assert_heads(check, launches)
    kernels = {heads.dispatch(s, cols_off=c) for s, _, c, _ in launches}
    assert kernels == {"cols", "mfma", "wave", "none"}


@pytest.mark.parametrize("C", HEAD_AXES["C"])
def test_heads_plan_over_every_launch_of_one_to_three_heads(check, C):
    """EVERY ordered launch of one, two and three heads out of the product (heads of a launch share C and P: 32 boards x
    84 + 84^2 + 84^3 launches), with the board-column form on and off; the one- and two-head launches also without the
    matrix-core kernel.  The per-head ingredients are net_head_cases' own (cols_ok, mfma_head_ok, mfma_total, wave_total,
    mfma_form, wave_split); a launch combines them as net_head_cases.dispatch and samples_per_round do -- every head must pass
    a form's test, the widest layout counts -- and that combination, written for arrays here, is held to those two
    functions on a seeded sample of the same launches."""
    tails = list(itertools.product(HEAD_AXES["R"], HEAD_AXES["Hd"], HEAD_AXES["O"]))
    T = len(tails)
    rs = np.random.RandomState(5 + C)
    form_code = lambda s: 1 + (heads.mfma_form(s)[0] == 4) + 2 * (heads.mfma_form(s)[1] == 2) + 4 * (heads.mfma_form(s)[2] == 16)
    seen = set()
    for P in HEAD_AXES["P"]:
        shapes = [(C, P) + t for t in tails]
        cols_ok = np.array([heads.cols_ok(s) for s in shapes])
        mfma_ok = np.array([heads.mfma_head_ok(s) for s in shapes])
        mfma_lds = 4 * np.array([heads.mfma_total(s) for s in shapes])
        wave_lds = 4 * np.array([heads.wave_total(s) for s in shapes])
        forms = np.array([form_code(s) for s in shapes])
        log_split = np.array([int(np.log2(heads.wave_split(s[3]))) for s in shapes])
        for n, cols_on, use_mfma in [(n, c, m) for n in (1, 2, 3) for c in (1, 0) for m in ((1, 0) if n < 3 else (1,))]:
            batch = (1, 65, 40000, 70001)[(n + cols_on + C + P) % 4]
            got = check("heads_product", [C, P, n, cols_on, use_mfma, batch, T] + [v for t in tails for v in t])
            assert got.shape == (T ** n, 3)                           # launch i: head h is shapes[unravel(i)[h]], the last fastest
            of_head = lambda a, h: np.broadcast_to(a.reshape([T if k == h else 1 for k in range(n)]), (T,) * n).ravel()
            every = lambda a: np.logical_and.reduce([of_head(a, h) for h in range(n)])
            widest = lambda a: np.maximum.reduce([of_head(a, h) for h in range(n)])
            cols = every(cols_ok) & bool(cols_on)
            mfma = ~cols & every(mfma_ok) & bool(use_mfma) & (widest(mfma_lds) <= heads.LDS_LIMIT)
            wave = ~cols & ~mfma & (widest(wave_lds) <= heads.LDS_LIMIT)
            kernel = np.select([cols, mfma, wave], [1, 2, 3], 0)
            lds = np.select([cols, mfma, wave], [50752, widest(mfma_lds), widest(wave_lds)], 0)
            per_cu = np.select([cols, mfma, wave], [1, np.clip(heads.LDS_LIMIT // np.maximum(lds, 1), 1, 4),
                                                    np.clip(heads.LDS_LIMIT // np.maximum(lds, 1), 1, 8)], 0)
            per_workgroup = np.select([cols, mfma, wave], [64, 64, 4], 1)
            grid = np.where(kernel == 0, 0, np.where(cols, -(-batch // 64), np.minimum(-(-batch // per_workgroup), 256 * per_cu)))
            per_head = sum((np.where(mfma, of_head(forms, h), 0) | np.where(wave, of_head(log_split, h), 0) << 4) << (7 * h) for h in range(n))
            want = np.stack([kernel | per_cu << 2 | (kernel == 0).astype(np.int64) << 6 | lds << 7, per_head, grid], axis=1)
            differ = np.flatnonzero(np.any(got != want, axis=1))
            assert differ.size == 0, (C, P, n, cols_on, use_mfma, [shapes[j] for j in np.unravel_index(differ[0], (T,) * n)], got[differ[0]], want[differ[0]])
            seen |= set(np.unique(kernel).tolist())
            if use_mfma:                                               # the combination above against the yardstick's own
                for i in rs.randint(0, T ** n, size=12):
                    launch = [shapes[j] for j in np.unravel_index(i, (T,) * n)]
                    name = heads.dispatch(launch, cols_off=not cols_on)
                    assert HEADS_KERNELS[kernel[i]] == name, (launch, cols_on)
                    if name in ("mfma", "wave"):
                        assert 256 * per_cu[i] * per_workgroup[i] == heads.samples_per_round(launch, name), (launch, name)
    assert seen == ({0, 1, 2, 3} if C == 16 else {0, 2, 3} if C <= 64 else {0, 3})


def test_heads_plan_refusals(check):
    ok = (16, 9, 4, 8, 21)

    def rc_kernel(shapes, n=None, batch=5, cols_on=1):
        flat = [v for s in shapes for v in s] + [0] * (5 * (3 - len(shapes)))
        out = check("heads", [[len(shapes) if n is None else n, batch, cols_on, 1] + flat], 19)[0]
        return int(out[0]), HEADS_KERNELS[out[1]]
    assert rc_kernel([ok]) == (0, "cols") and rc_kernel([ok], batch=0) == (0, "cols")
    assert rc_kernel([ok], batch=0x40000000) == (0, "mfma")                     # past the board-column form's batch limit
    assert rc_kernel([ok], n=0)[0] == -1 and rc_kernel([ok, ok, ok], n=4)[0] == -1 and rc_kernel([ok], batch=-1)[0] == -1
    for field in range(5):
        for bad in (0, -1):
            shape = list(ok)
            shape[field] = bad
            assert rc_kernel([ok, tuple(shape)])[0] == -1 and rc_kernel([tuple(shape)])[0] == -1
    assert rc_kernel([ok, (17, 9, 4, 8, 21)])[0] == -1 and rc_kernel([ok, (16, 36, 4, 8, 21)])[0] == -1   # one board, one C per launch
    assert rc_kernel([(64, 42, 16, 64, 21)], batch=0) == (-1, "none")           # over 160 KB in both forms: also for an empty batch


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------
def test_check_program_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtimes here")             # (a trivial program does not link: nothing of ours)
    exe = str(tmp_path / "launch_plan_check_san")
    built = subprocess.run([gxx] + flags + ["-I", CSRC, "-o", exe, SOURCE], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = _runner(tmp_path, exe)
    axes = dict(channels=(16, 64), board=range(3), cin0=(1, 16, 17, 65, 80), n_layers=(0, 1, 2, 16, 17), split=(0, 1), const_plane=(0, 1),
                n_heads=(-1, 0, 3, 4), batch=(-1, 0, 1, 16384, 0x40000000))
    grid = dict(zip(axes, (a.ravel() for a in np.meshgrid(*axes.values(), indexing="ij"))))
    h, w = np.array(BOARDS)[grid.pop("board")].T
    rows = tower_rows(h=h, w=w, **grid)
    assert_same_plans(tower_header(run, rows), tower_restated(rows), rows, TOWER_OUT)
    run("conv", [[b, cin, cout, h, w] for b in (-1, 0, 5) for cin in (0, 1, 80, 81) for cout in (16, 64, 5) for h, w in BOARDS], 5)
    run("blocks", [[b, c, h, w, 2] for b in (-1, 0, 5, 0x40000000) for c in (16, 64) for h, w in BOARDS], 5)
    assert_heads(run, [(case["shapes"], batch, case["cols_off"], True) for case in heads.HEAD_CASES.values() for batch in case["batches"]])
    run("heads", [[n, 5, 1, 1] + [16, 9, 4, 8, 21] * 3 for n in (-1, 0, 4)], 19)
    for n in (1, 2, 3):
        assert len(run("heads_product", [64, 42, n, 1, 1, 70001, 3, 16, 64, 21, 17, 65, 65, 2, 1, 1])) == 3 ** n
    assert run("sizes", [])["patch_boards"] == 16
