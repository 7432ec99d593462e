"""csrc/staging_layout.h -- the one place the search engine's five staging blocks are laid out (per-move upload, per-tree
download, move-batch control block, output ring, inputs ring) -- built for the host with g++ (tests/staging_layout_check.cpp)
and held, shape by shape, to tests/staging_layout_cases.py: the offset chains as mzmcts_create, ensure_batch_capacity and
ensure_inputs_capacity had them before the header.  Beyond equality: no field overlaps another or leaves its block, each is
aligned to its element, the move-batch blocks step by 256 bytes, and the orderings the copies rely on hold.  The check
program also writes a distinct value through every typed pointer of every block and reads them all back; it is built once
more with -fsanitize=address,undefined and run directly."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

import staging_layout_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "staging_layout_check.cpp")

ES = (1, 2, 3, 63, 64, 65, 83, 512)
AS = (1, 2, 3, 9, 64, 65, 121, 256)
MS = (1, 2, 3, 12, 4096)
SHAPES = list(itertools.product(ES, AS, MS))
ROUNDTRIPS = ((3, 2, 3), (5, 9, 2))
SIZE_KEYS = {"upload": ("bytes", "bytes_no_noise"), "download": ("bytes",), "control": ("bytes",), "output": ("stride",), "inputs": ("stride",)}


def restated(E, A, M):
    return dict(upload=cases.upload(E, A), download=cases.download(E), control=cases.move_control(E, A, M),
                output=cases.move_output(E, A), inputs=cases.move_inputs(E, A))


def parse(line):
    """One line of `staging_layout_check offsets` -> (shape, {block: ({field: offset}, {size key: value})}), read in the
    program's order: each block's fields, then its sizes."""
    numbers = [int(v) for v in line.split()]
    shape, at, out = tuple(numbers[:3]), 3, {}
    for block, want in restated(*shape).items():
        names = [f[0] for f in want["fields"]]
        keys = SIZE_KEYS[block]
        out[block] = (dict(zip(names, numbers[at:at + len(names)])), dict(zip(keys, numbers[at + len(names):at + len(names) + len(keys)])))
        at += len(names) + len(keys)
    assert at == len(numbers), line
    return shape, out


def run_offsets(exe, shapes):
    text = "".join("%d %d %d\n" % s for s in shapes)
    proc = subprocess.run([exe, "offsets"], input=text, capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr
    parsed = [parse(line) for line in proc.stdout.strip().splitlines()]
    assert [p[0] for p in parsed] == list(shapes)
    return parsed


def assert_equal_to_restatement(parsed):
    for shape, blocks in parsed:
        for block, want in restated(*shape).items():
            got_offsets, got_sizes = blocks[block]
            assert got_offsets == cases.offsets(want), (shape, block)
            assert got_sizes == {k: want[k] for k in SIZE_KEYS[block]}, (shape, block)


def build(gxx, out, flags):
    built = subprocess.run([gxx] + flags + ["-std=c++17", "-I", CSRC, "-o", out, SOURCE], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return out


@pytest.fixture(scope="module")
def gxx():
    found = shutil.which("g++")
    if found is None:
        pytest.skip("no g++")
    return found


@pytest.fixture(scope="module")
def exe(gxx, tmp_path_factory):
    return build(gxx, str(tmp_path_factory.mktemp("staging_layout") / "staging_layout_check"), ["-O2", "-Wall", "-Werror"])


@pytest.fixture(scope="module")
def header(exe):
    """Every offset, size and stride the header gives, over the product of shapes."""
    assert len(SHAPES) == 8 * 8 * 5
    return run_offsets(exe, SHAPES)


def test_header_includes_no_device_or_engine_header():
    text = open(os.path.join(CSRC, "staging_layout.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>"]


def test_every_offset_size_and_stride_equals_the_restatement(header):
    assert_equal_to_restatement(header)


def test_fields_lie_inside_their_block_apart_and_aligned(header):
    for shape, blocks in header:
        for block, want in restated(*shape).items():
            got, sizes = blocks[block]
            end = sizes.get("bytes", sizes.get("stride"))
            spans = sorted((got[name], got[name] + size * count, size, name) for name, _, size, count in want["fields"])
            for (lo, hi, size, name), (next_lo, _, _, _) in zip(spans, spans[1:] + [(end, 0, 0, "")]):
                assert 0 <= lo < hi <= next_lo, (shape, block, name)
                assert lo % min(size, 8) == 0, (shape, block, name)    # (mz::MinMax, 16 bytes: two doubles, aligned as one)
            assert spans[-1][1] <= end


def test_move_batch_blocks_step_by_256_bytes(header):
    for shape, blocks in header:
        for block in ("control", "output", "inputs"):
            got, sizes = blocks[block]
            assert all(v % 256 == 0 for v in got.values()) and all(v % 256 == 0 for v in sizes.values()), (shape, block)


def test_orderings_the_copies_rely_on(header):
    for (E, A, M), blocks in header:
        control, sizes = blocks["control"]
        # the noise rows first; behind them ONE range up to the block's end: each field starts on the 256-byte step its
        # predecessor ends in (mzmcts_moves_prepare_device uploads [rng_skip, bytes) in one copy)
        assert control["noise"] == 0 and min(v for k, v in control.items() if k != "noise") == control["rng_skip"]
        assert control["rng_skip"] == cases.align256(8 * M * E * A)
        rest = [("rng_skip", 4 * M * E), ("temperature", 8 * E), ("move_limit", 4 * E), ("expected_ties", 4 * E)]
        for (name, nbytes), following in zip(rest, [control[n] for n, _ in rest[1:]] + [sizes["bytes"]]):
            assert following == cases.align256(control[name] + nbytes), ((E, A, M), name)
        upload, upload_sizes = blocks["upload"]
        assert upload_sizes["bytes_no_noise"] == upload["noise"] == max(upload.values())
        assert upload_sizes["bytes"] == upload["noise"] + 8 * E * A


@pytest.mark.parametrize("shape", ROUNDTRIPS, ids=lambda s: "E%d-A%d-M%d" % s)
def test_values_written_through_every_typed_pointer_read_back(exe, shape):
    proc = subprocess.run([exe, "roundtrip"] + [str(v) for v in shape], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert json.loads(proc.stdout.strip().splitlines()[-1]) == {"fields": 18 + 12 * shape[2], "bad": 0}


def test_check_program_is_clean_under_asan_and_ubsan(gxx, tmp_path):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([gxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtimes here")             # (a trivial program does not link: nothing of ours)
    san = build(gxx, str(tmp_path / "staging_layout_check_san"), flags)
    assert_equal_to_restatement(run_offsets(san, SHAPES))
    for shape in ROUNDTRIPS:
        proc = subprocess.run([san, "roundtrip"] + [str(v) for v in shape], capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        assert json.loads(proc.stdout.strip().splitlines()[-1])["bad"] == 0
