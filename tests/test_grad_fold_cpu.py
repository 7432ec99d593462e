"""Weight gradients folded and the optimizer applied (csrc/grad_fold.h, include/mztrain.h mztrain_fold_*) without a GPU.

The host entry mztrain_fold_reference against the numpy restatement of tests/grad_fold_reference.py -- sequential float32
additions in ascending slot order, then mztrain_opt_reference on the folded gradient -- bit for bit: segment counts either
side of the vector width and of a chunk, uses 1, 2 and 21, offsets that are and are not 16-byte aligned, Adam and SGD with
momentum 0 and 0.9, weight decay 0 and 1e-4, three steps under a changing rate.  Sentinels between the segments and NaN in
every slot at `uses` or above show what must not be touched or read.  Directed cases, five named defects each seen on a named
case, the launch plan against a restatement, every refusal, the struct layouts, the header as a stand-alone program under the
address and undefined-behaviour sanitizers (tests/grad_fold_check.cpp), the Trainer's refusals that need no GPU, and the
autograd graph with no sink installed."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import grad_fold_reference as ref
from test_struct_layout import c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "muzero-hypermodel_amd", "csrc")
OPT_CASES = [(label, decay) for label in ref.KINDS for decay in ref.DECAYS]
OPT_IDS = [f"{l}-wd{d:g}" for l, d in OPT_CASES]
LAYOUTS = ref.the_case_list()


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def how(label):
    return ref.KINDS[label]["kind"], ref.KINDS[label].get("momentum", 0.0)


def assert_untouched(layout, state, kind, momentum, what):
    """Sentinels in the gaps of every flat buffer, and no NaN anywhere a step writes."""
    gaps = ~layout.inside()
    for key in ("weights", "grads", "moment1", "moment2"):
        assert (state[key][gaps] == ref.SENTINEL).all(), (what, key, "a float outside every segment was written")
    for key in ref.tensors_of(kind, momentum):
        assert not np.isnan(state[key]).any(), (what, key, "a slot at uses or above was read")


# ---- the host entry against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", LAYOUTS, ids=[name for name, _ in LAYOUTS])
@pytest.mark.parametrize("label,decay", OPT_CASES, ids=OPT_IDS)
def test_the_host_entry_is_the_restatement_bit_for_bit(native, label, decay, name, layout):
    kind, momentum = how(label)
    weights, stagings = layout.make_case()
    lrs = ref.learning_rates()
    assert len(set(lrs)) == ref.STEPS == 3
    want = ref.run_restatement(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
    got = ref.run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
    assert got["steps_done"] == want["steps_done"] == 3
    for key in ("weights", "grads", "moment1", "moment2"):       # (all four: a buffer the kind does not use stays as it was)
        assert ref.same_bits(got[key], want[key]), (name, key)
    assert_untouched(layout, got, kind, momentum, name)
    moved = [k for k, uses in enumerate(layout.uses) if uses]
    for k in moved:
        at, count = layout.offsets[k], layout.counts[k]
        assert not ref.same_bits(got["weights"][at:at + count], weights[at:at + count]), (name, k, "a used segment stood still")


def test_the_case_list_covers_what_it_should():
    counts = {c for _, layout in LAYOUTS for c in layout.counts}
    assert {1, 3, 4, 5, 255, 256, 257, 1025} <= counts
    assert {1, 2, 21, 0} <= {u for _, layout in LAYOUTS for u in layout.uses}
    for _, layout in LAYOUTS:
        assert all((at % 4 == 0) == layout.aligned for at in layout.offsets)
        assert all((base % 4 == 0) == layout.aligned for base in layout.slot_bases)
        assert all(stride % 128 == 0 and stride >= count for stride, count in zip(layout.strides, layout.counts))


# ---- directed cases -----------------------------------------------------------------------------------------------------------------
def one_segment(native, slots, capacity=None, kind="SGD", lr=1.0):
    """A one-element segment with the given slots under SGD without momentum or decay: (w = 0 - lr * g, the folded g)."""
    layout = ref.Layout([1], [len(slots)], capacity=capacity or len(slots))
    weights = np.full(layout.n, ref.SENTINEL, dtype=np.float32)
    weights[layout.offsets[0]] = 0.0
    staging = np.full(layout.staging_floats, np.nan, dtype=np.float32)
    for s, value in enumerate(slots):
        layout.slot(staging, 0, s)[0] = value
    return layout, weights, staging


def test_the_fold_is_sequential_float32_in_ascending_order(native):
    slots = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]
    layout, weights, staging = one_segment(native, slots)
    got = ref.run_host_entry(native, layout, "SGD", weights, [staging], [1.0])
    at = layout.offsets[0]
    assert got["grads"][at] == 0.0 and got["weights"][at] == 0.0
    assert float(ref.fold32([np.float32([v]) for v in slots])[0]) == 0.0
    assert float(ref.fold32([np.float32([v]) for v in slots[::-1]])[0]) == 2.0
    assert float(np.float32(np.sum(np.array(slots, dtype=np.float64)))) == 2.0


def test_an_unused_segment_is_untouched_while_its_neighbours_move(native):
    layout = ref.Layout([5, 257, 4], [2, 0, 3])
    weights, stagings = layout.make_case()
    for label, decay in OPT_CASES:
        kind, momentum = how(label)
        got = ref.run_host_entry(native, layout, kind, weights, stagings, ref.learning_rates(), weight_decay=decay,
                                 momentum=momentum)
        at, count = layout.offsets[1], layout.counts[1]
        assert ref.same_bits(got["weights"][at:at + count], weights[at:at + count]), label
        assert (got["grads"][at:at + count] == ref.SENTINEL).all(), label
        assert not got["moment1"][at:at + count].any() and not got["moment2"][at:at + count].any(), label
        for k in (0, 2):
            a, c = layout.offsets[k], layout.counts[k]
            assert not ref.same_bits(got["weights"][a:a + c], weights[a:a + c]), (label, k)


DEFECT_CASES = {
    # defect: (layout, optimizer label, weight decay, what shows it)
    "reverse_order": (ref.Layout([257], [21]), "sgd-m0", 0.0, "grads"),
    "float64_fold": (ref.Layout([1025], [21]), "sgd-m0", 0.0, "grads"),
    "decay_reaches_gap": (ref.Layout([5, 4], [2, 1]), "adam", 1e-4, "gap"),
    "one_slot_too_many": (ref.Layout([5, 256], [2, 1]), "adam", 0.0, "nan"),
    "unused_segment_updated": (ref.Layout([5, 257, 4], [2, 0, 3]), "adam", 1e-4, "unused"),
}


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_a_defect_is_seen_on_its_case(native, defect):
    """The restatement with the defect built in stands in for an implementation that has it: on the named case it differs
    from the host entry in the named way, and the host entry equals the restatement without the defect."""
    layout, label, decay, shows = DEFECT_CASES[defect]
    kind, momentum = how(label)
    weights, stagings = layout.make_case()
    lrs = ref.learning_rates()
    good = ref.run_restatement(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
    got = ref.run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
    broken = ref.run_restatement(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum,
                                 defect=defect)
    for key in ("weights", "grads", "moment1", "moment2"):
        assert ref.same_bits(got[key], good[key]), key
    gaps = ~layout.inside()
    if shows == "grads":
        assert not ref.same_bits(broken["grads"], got["grads"]) and not ref.same_bits(broken["weights"], got["weights"])
    elif shows == "gap":
        assert (got["weights"][gaps] == ref.SENTINEL).all() and not (broken["weights"][gaps] == ref.SENTINEL).all()
    elif shows == "nan":
        assert np.isnan(broken["grads"]).any() and np.isnan(broken["weights"]).any()
        assert not np.isnan(got["grads"]).any() and not np.isnan(got["weights"]).any()
    else:
        at, count = layout.offsets[1], layout.counts[1]
        assert (got["grads"][at:at + count] == ref.SENTINEL).all() and not (broken["grads"][at:at + count] == ref.SENTINEL).all()
        assert ref.same_bits(got["weights"][at:at + count], weights[at:at + count])
        assert not ref.same_bits(broken["weights"][at:at + count], weights[at:at + count])


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
PLAN_COUNTS = [(1,), (1024,), (1025,), (1, 3, 4, 5, 255, 256, 257, 1025), (2049, 16, 1023), (1024 * 1024,),
               (1024 * 1023 + 1, 1), (1024 * 1024, 1), (4096,) * 300]


@pytest.mark.parametrize("counts", PLAN_COUNTS, ids=[f"{len(c)}x{max(c)}" + ("" if i < 6 else f"-{i}") for i, c in
                                                    enumerate(PLAN_COUNTS)])
def test_the_plan_at_its_edges(native, counts):
    lib = native.load()
    for aligned in (True, False):
        layout = ref.Layout(counts, [1] * len(counts), aligned=aligned, capacity=1)
        want, grid = ref.plan_restated(counts)
        out = (ctypes.c_int64 * 4)()
        assert lib.mztrain_fold_plan(layout.segments(native), len(counts), layout.n, layout.staging_floats, out, None, 0) == 0
        assert list(out) == [len(want), grid, ref.THREADS, ref.CHUNK] and 1 <= out[1] <= ref.MAX_BLOCKS
        table = (ctypes.c_int64 * (4 * len(want)))()
        assert lib.mztrain_fold_plan(layout.segments(native), len(counts), layout.n, layout.staging_floats, out, table,
                                     len(want)) == 0
        got = np.array(table, dtype=np.int64).reshape(-1, 4)
        assert [tuple(row[:3]) for row in got.tolist()] == want
        assert (got[:, 3] == (1 if aligned else 0)).all()
        # every element in exactly one chunk, no chunk across a segment
        for k, count in enumerate(counts):
            rows = got[got[:, 0] == k]
            assert (rows[:, 1] + rows[:, 2] <= count).all() and (rows[:, 2] >= 1).all() and (rows[:, 2] <= ref.CHUNK).all()
            covered = np.zeros(count, dtype=np.int32)
            for _, first, n, _ in rows.tolist():
                covered[first:first + n] += 1
            assert (covered == 1).all(), k
        if len(want) > 1:
            assert lib.mztrain_fold_plan(layout.segments(native), len(counts), layout.n, layout.staging_floats, out, table,
                                         len(want) - 1) == native.ERR_INVALID
    assert max(len(ref.plan_restated(c)[0]) for c in PLAN_COUNTS) > ref.MAX_BLOCKS      # the cap is met


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def segment(native, **over):
    fields = dict(offset=8, count=5, slot_base=0, slot_stride=128, capacity=3)
    fields.update(over)
    return native.MzTrainFoldSegment(**fields)


def good_fold_args(native, kind="Adam", n=64, staging_floats=1024, **over):
    fields = dict(weights=0x1000, grads=0x2000, moment1=0x3000, moment2=0x4000, lr=0x5000, steps_done=0x6000, staging=0x7000)
    hyper = dict(weight_decay=1e-4, momentum=0.9 if kind == "SGD" else 0.0)
    for key in list(over):
        if key in hyper or key in ("beta1", "beta2", "eps"):
            hyper[key] = over.pop(key)
    fields.update(over)
    return ref.fold_args(native, kind, n, fields["weights"], fields["grads"], fields["moment1"], fields["moment2"],
                         fields["lr"], fields["steps_done"], fields["staging"], staging_floats, **hyper)


def test_refusals_decided_on_the_segments(native):
    """Create, plan and the host entry share them; nothing is dereferenced (the pointers point nowhere) and no device is
    touched: create refuses before it selects one."""
    lib = native.load()

    def entries(array, count, n=64, staging_floats=1024):
        handle = ctypes.c_void_p()
        out = (ctypes.c_int64 * 4)()
        uses = ref.uses_array([1] * max(count, 1))
        args = good_fold_args(native, n=n, staging_floats=staging_floats)
        yield "mztrain_fold_create", lib.mztrain_fold_create(array, count, n, staging_floats, 0, ctypes.byref(handle))
        assert handle.value is None
        yield "mztrain_fold_plan", lib.mztrain_fold_plan(array, count, n, staging_floats, out, None, 0)
        assert list(out) == [0, 0, 0, 0]
        yield "mztrain_fold_reference", lib.mztrain_fold_reference(array, uses, count, ctypes.byref(args))

    def check(segments, text, count=None, **sizes):
        array = (native.MzTrainFoldSegment * len(segments))(*segments) if segments is not None else None
        count = (len(segments) if segments is not None else 1) if count is None else count
        for entry, rc in entries(array, count, **sizes):
            message = (lib.mzmcts_last_error(None) or b"").decode()
            assert rc == native.ERR_INVALID and text in message and message.startswith(entry + ":"), (entry, text, rc, message)

    check(None, "null segments")
    for count in (0, -3):
        check([segment(native)], "n_segments must be positive", count=count)
    check([segment(native)], "n and staging_floats must be positive", n=0)
    check([segment(native)], "n and staging_floats must be positive", staging_floats=0)
    check([segment(native, count=0)], "count must be positive")
    for over in (dict(offset=-1), dict(offset=60), dict(offset=64, count=1), dict(offset=0, count=65)):
        check([segment(native, **over)], "outside the flat buffer")
    check([segment(native, offset=0, count=130, slot_stride=128)], "slot_stride below count", n=256)
    for stride in (5, 6, 7, 129):
        check([segment(native, slot_stride=stride)], "slot_stride must be a multiple of 4")
    check([segment(native, capacity=0)], "capacity must be positive")
    for over in (dict(slot_base=-4), dict(slot_base=1024), dict(capacity=9), dict(slot_base=768), dict(slot_base=1020, capacity=1)):
        check([segment(native, **over)], "outside the staging buffer")
    check([segment(native), segment(native, offset=12, slot_base=512)], "overlaps another")
    check([segment(native, offset=10, slot_base=512), segment(native)], "overlaps another")
    check([segment(native, offset=0, count=40, slot_base=512), segment(native)], "overlaps another")     # one inside the other


def test_adjacent_segments_and_a_last_slot_that_just_fits_are_taken(native):
    lib = native.load()
    array = (native.MzTrainFoldSegment * 2)(segment(native, offset=8, count=5), segment(native, offset=13, count=51,
                                                                                        slot_base=384, slot_stride=52, capacity=13))
    out = (ctypes.c_int64 * 4)()
    assert 384 + 12 * 52 + 51 == 1059
    assert lib.mztrain_fold_plan(array, 2, 64, 1059, out, None, 0) == 0 and list(out)[:2] == [2, 2]
    assert lib.mztrain_fold_plan(array, 2, 64, 1058, out, None, 0) == native.ERR_INVALID


def test_refusals_of_the_uses_and_the_arguments(native):
    lib = native.load()
    array = (native.MzTrainFoldSegment * 2)(segment(native), segment(native, offset=20, slot_base=384))
    entry = "mztrain_fold_reference"

    def check(uses, args, text, count=2):
        rc = lib.mztrain_fold_reference(array, ref.uses_array(uses) if uses is not None else None, count,
                                        ctypes.byref(args) if args is not None else None)
        message = (lib.mzmcts_last_error(None) or b"").decode()
        assert rc == native.ERR_INVALID and text in message and message.startswith(entry + ":"), (text, rc, message)

    good = good_fold_args(native, staging_floats=768)
    check([1, 1], None, "null args")
    check(None, good, "null uses")
    check([1, 4], good, "uses outside [0, capacity] (segment 1)")
    check([-1, 1], good, "uses outside [0, capacity] (segment 0)")
    check([1, 1], good_fold_args(native, staging_floats=768, staging=None), "null pointer in args (staging)")
    # the optimizer's own refusals, through the same check as mztrain_opt_step
    for member in ("weights", "grads", "lr", "steps_done"):
        check([1, 1], good_fold_args(native, staging_floats=768, **{member: None}), "null pointer in args")
    check([1, 1], good_fold_args(native, staging_floats=768, moment2=None), "Adam needs moment1 and moment2")
    check([1, 1], good_fold_args(native, "SGD", staging_floats=768, moment1=None), "SGD with momentum needs moment1")
    check([1, 1], good_fold_args(native, staging_floats=768, beta1=1.0), "beta1 and beta2 must lie in [0, 1)")
    check([1, 1], good_fold_args(native, staging_floats=768, eps=0.0), "eps must be positive")
    check([1, 1], good_fold_args(native, staging_floats=768, weight_decay=-1.0), "weight_decay must be finite")
    bad = good_fold_args(native, staging_floats=768)
    bad.opt.kind = 5
    check([1, 1], bad, "unknown kind")
    # the handle's entries refuse a null handle before anything else
    for name, call in (("mztrain_fold_set_uses", lambda: lib.mztrain_fold_set_uses(None, ref.uses_array([1, 1]), 2)),
                       ("mztrain_fold_step", lambda: lib.mztrain_fold_step(None, ctypes.byref(good), None))):
        rc = call()
        message = (lib.mzmcts_last_error(None) or b"").decode()
        assert rc == native.ERR_INVALID and message == name + ": null handle"
    assert lib.mztrain_fold_create(array, 2, 64, 768, 0, None) == native.ERR_INVALID
    lib.mztrain_fold_destroy(None)


def test_structs_match_their_ctypes_mirrors(native, tmp_path):
    pairs = {"mztrain_fold_segment": native.MzTrainFoldSegment, "mztrain_fold_args": native.MzTrainFoldArgs}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mztrain.h"', "int main(void) {"]
    fields = {}
    for name in pairs:
        fields[name] = c_fields("mztrain.h", name)
        lines.append(f'    printf("%zu", sizeof({name}));')
        lines += [f'    printf(" %zu", offsetof({name}, {f}));' for f in fields[name]]
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rows = subprocess.check_output([str(exe)], text=True).splitlines()
    for (name, mirror), row in zip(pairs.items(), rows):
        size, *offsets = (int(v) for v in row.split())
        assert [f for f, *_ in mirror._fields_] == fields[name], name
        assert ctypes.sizeof(mirror) == size and [getattr(mirror, f).offset for f in fields[name]] == offsets, name
    assert fields["mztrain_fold_segment"] == ["offset", "count", "slot_base", "slot_stride", "capacity", "reserved"]
    assert fields["mztrain_fold_args"] == ["opt", "staging", "staging_floats"]
    assert ctypes.sizeof(native.MzTrainFoldSegment) == 40
    assert (native.FOLD_CHUNK, native.FOLD_MAX_BLOCKS) == (ref.CHUNK, ref.MAX_BLOCKS)


# ---- the header under the sanitizers ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "the check needs g++"
    exe = str(tmp_path_factory.mktemp("grad_fold") / "grad_fold_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "grad_fold_check.cpp")],
                   check=True)
    return exe


@pytest.mark.parametrize("label,decay", OPT_CASES, ids=OPT_IDS)
def test_the_header_under_the_sanitizers_gives_the_entrys_bits(native, program, tmp_path, label, decay):
    kind, momentum = how(label)
    lrs = ref.learning_rates()
    for name, layout in LAYOUTS:
        if "uses2-" in name:
            continue                                 # (uses 1 and 21 and the mixed list: the program is the slow part)
        weights, stagings = layout.make_case()
        start = ref.start_state(layout, weights)
        source, result = tmp_path / f"{name}.bin", tmp_path / f"{name}.out"
        with open(source, "wb") as f:
            f.write(struct.pack("<4i2q5d", native.OPT_ADAM if kind == "Adam" else native.OPT_SGD, len(stagings),
                                len(layout.counts), 0, layout.n, layout.staging_floats, ref.optref.BETA1, ref.optref.BETA2,
                                ref.optref.EPS, decay, momentum))
            f.write(np.asarray(lrs, dtype=np.float64).tobytes())
            f.write(bytes(layout.segments(native)))
            f.write(np.asarray(layout.uses, dtype=np.int32).tobytes())
            for key in ("weights", "grads", "moment1", "moment2"):
                f.write(start[key].tobytes())
            for staging in stagings:
                f.write(staging.tobytes())
        done = subprocess.run([program, str(source), str(result)], capture_output=True, text=True)
        assert done.returncode == 0, (name, done.stderr)
        arrays = np.fromfile(result, dtype=np.float32).reshape(4, layout.n)
        want = ref.run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=decay, momentum=momentum)
        for index, key in enumerate(("weights", "grads", "moment1", "moment2")):
            assert ref.same_bits(arrays[index], want[key]), (name, key)


# ---- the Trainer, as far as a machine without a GPU goes -----------------------------------------------------------------------------
THREE = dict(native_epilogue=True, native_conv=True, native_heads=True)


def test_the_trainers_refusals_come_in_order(pkg):
    """Missing flags first, then the network, then the device; fc_step and an uncovered parameter need a model on the GPU and
    are in tests/test_gpu_grad_fold.py."""
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    cartpole = importlib.import_module("muzero-hypermodel_amd.games.cartpole").MuZeroConfig()
    tictactoe = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    assert cartpole.network == "fullyconnected" and tictactoe.network == "resnet"

    def ckpt(config):
        return {"weights": models.MuZeroNetwork(config).get_weights(), "training_step": 0, "optimizer_state": None}

    for missing in THREE:
        flags = {k: v for k, v in THREE.items() if k != missing}
        with pytest.raises(NotImplementedError, match=rf"native_optimizer=True\).*pass {missing}=True as well"):
            trainer_mod.Trainer(ckpt(cartpole), cartpole, device="cpu", fc_step=True, native_optimizer=True, **flags)
    with pytest.raises(NotImplementedError, match="pass native_epilogue=True, native_conv=True, native_heads=True as well"):
        trainer_mod.Trainer(ckpt(cartpole), cartpole, device="cpu", native_optimizer=True, native_rescale=True)
    with pytest.raises(NotImplementedError, match=r"native_optimizer=True\) folds the gradients of residual networks"):
        trainer_mod.Trainer(ckpt(cartpole), cartpole, device="cpu", fc_step=True, native_optimizer=True, **THREE)
    with pytest.raises(NotImplementedError, match=r"native_optimizer=True\) runs HIP kernels: the model must be on the GPU"):
        trainer_mod.Trainer(ckpt(tictactoe), tictactoe, device="cpu", fc_step=True, native_optimizer=True, **THREE)
    # without the flag nothing of this is consulted
    trainer = trainer_mod.Trainer(ckpt(tictactoe), tictactoe, device="cpu")
    assert trainer._fold is None and not hasattr(trainer, "flat_weights")
    with pytest.raises(NotImplementedError, match="native_optimizer"):
        trainer.gradients()


def graph_of(tensor):
    """The autograd graph under `tensor` as a sorted list of (node name, names of its inputs' nodes)."""
    seen, out, todo = set(), [], [tensor.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        out.append((type(node).__name__, tuple(type(n).__name__ if n is not None else "None" for n, _ in node.next_functions)))
        todo.extend(n for n, _ in node.next_functions)
    return sorted(out)


def test_no_sink_leaves_the_autograd_graph_node_for_node(pkg):
    """Installing a sink and taking it away again leaves no trace: the same unroll builds the same graph, and on a model that
    never had one no parameter carries the attribute.  (On the CPU the Functions do not run; what the sink changes in their
    backward is in the GPU tests.)"""
    trainer_mod = importlib.import_module("muzero-hypermodel_amd.trainer")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module("muzero-hypermodel_amd.games.tictactoe").MuZeroConfig()
    config.num_unroll_steps = 2
    torch.manual_seed(1)
    model = models.MuZeroNetwork(config)
    model.train()
    assert all(models._sink_slot(p) is None for p in model.parameters()) and "_gradient_sink" not in model.__dict__
    observations = torch.rand((4,) + tuple(config.observation_shape))
    actions = torch.randint(0, 9, (4, 3, 1))

    def unroll():
        import types
        steps = trainer_mod.Trainer._unroll(types.SimpleNamespace(model=model), observations, actions)
        return graph_of(sum(t.sum() for step in steps for t in step))

    before = unroll()
    names = [name for name, _ in model.named_parameters()]
    views = [[torch.zeros_like(p)] for p in model.parameters()]
    sink = models.GradientSink(names, views)
    model.install_gradient_sink(sink)
    assert [models._sink_slot(p)[1] for p in model.parameters()] == list(range(len(names)))
    model.install_gradient_sink(None)
    assert all(models._sink_slot(p) is None for p in model.parameters())
    assert unroll() == before and len(before) > 50
    # the sink itself: slots in arrival order, one arrival too many raises and names the parameter
    assert sink.next_slot(3) is views[3][0] and sink.arrivals[3] == 1
    with pytest.raises(RuntimeError, match=names[3].replace(".", r"\.") + r" received gradient number 2"):
        sink.next_slot(3)
    sink.reset()
    assert sink.next_slot(3) is views[3][0]
