"""The fold-and-update step (csrc/grad_fold.h, include/mztrain.h mztrain_fold_*) restated in numpy: per segment the slots are
added one after the other in float32, ascending, the sum goes to the flat gradient buffer, and mztrain_opt_reference -- the
flat-buffer optimizer's own host entry -- is run on that segment's weights, moments and folded gradient.  Also the launch
plan restated, the case layouts the CPU and the GPU tests share, and `defect`: a named mistake, so that the tests can show
the case each one is seen on."""
import ctypes

import numpy as np

import fc_optimizer_reference as optref

COUNTS = (1, 3, 4, 5, 255, 256, 257, 1025)
USES = (1, 2, 21)
CAPACITY = 21
KINDS = optref.KINDS
DECAYS = optref.DECAYS
STEPS = 3
SENTINEL = np.float32(-12345.5)
DEFECTS = ("reverse_order", "float64_fold", "decay_reaches_gap", "one_slot_too_many", "unused_segment_updated")
CHUNK, MAX_BLOCKS, THREADS = 1024, 1024, 256


def learning_rates(steps=STEPS):
    return optref.learning_rates(steps)


class Layout:
    """Segments of `counts` floats in flat buffers of n floats, with gaps between them, and their slots in a staging buffer.
    aligned: every offset and slot_base a multiple of 4 floats; else each is one float past such a boundary."""

    def __init__(self, counts, uses, aligned=True, capacity=CAPACITY, gap=7):
        self.counts, self.uses, self.capacity, self.aligned = list(counts), list(uses), capacity, aligned
        assert len(self.counts) == len(self.uses)
        self.offsets, self.slot_bases, self.strides = [], [], []
        at, slot = gap, 0
        for count in self.counts:
            at = -(-at // 4) * 4 + (0 if aligned else 1)
            slot = -(-slot // 128) * 128 + (0 if aligned else 1)
            stride = -(-count // 128) * 128
            self.offsets.append(at)
            self.slot_bases.append(slot)
            self.strides.append(stride)
            at += count + gap
            slot += stride * capacity
        self.n, self.staging_floats = at, slot

    def segments(self, native):
        array = (native.MzTrainFoldSegment * len(self.counts))()
        for k in range(len(self.counts)):
            array[k] = native.MzTrainFoldSegment(offset=self.offsets[k], count=self.counts[k], slot_base=self.slot_bases[k],
                                                 slot_stride=self.strides[k], capacity=self.capacity)
        return array

    def inside(self):
        mask = np.zeros(self.n, dtype=bool)
        for at, count in zip(self.offsets, self.counts):
            mask[at:at + count] = True
        return mask

    def slot(self, staging, k, s):
        first = self.slot_bases[k] + s * self.strides[k]
        return staging[first:first + self.counts[k]]

    def make_case(self, steps=STEPS, seed=0):
        """(weights with sentinels in the gaps, per step a staging buffer: the slots in use hold gradients, all else NaN)."""
        rng = np.random.RandomState(seed + 31 * self.n)
        weights = np.full(self.n, SENTINEL, dtype=np.float32)
        weights[self.inside()] = (rng.standard_normal(int(self.inside().sum())) * 0.5).astype(np.float32)
        stagings = []
        for _ in range(steps):
            staging = np.full(self.staging_floats, np.nan, dtype=np.float32)
            for k, count in enumerate(self.counts):
                for s in range(self.uses[k]):
                    g = rng.standard_normal(count) * 10.0 ** rng.uniform(-6, 0, count)
                    g[rng.random_sample(count) < 0.1] = 0.0
                    self.slot(staging, k, s)[:] = g.astype(np.float32)
            stagings.append(staging)
        return weights, stagings


def fold32(slots):
    """Sequential float32 additions, ascending."""
    g = np.array(slots[0], dtype=np.float32, copy=True)
    for s in slots[1:]:
        g = g + np.asarray(s, dtype=np.float32)
        assert g.dtype == np.float32
    return g


def start_state(layout, weights):
    """{weights, grads, moment1, moment2} as a step finds them: sentinels wherever no launch may write."""
    return {"weights": weights.copy(), "grads": np.full(layout.n, SENTINEL, dtype=np.float32),
            "moment1": np.where(layout.inside(), np.float32(0), SENTINEL).astype(np.float32),
            "moment2": np.where(layout.inside(), np.float32(0), SENTINEL).astype(np.float32)}


def run_restatement(native, layout, kind, weights, stagings, lrs, weight_decay=0.0, momentum=0.0, defect=None):
    """The steps by numpy's fold and mztrain_opt_reference per segment."""
    lib = native.load()
    state = start_state(layout, weights)
    adam = kind == "Adam"
    with_buffer = adam or momentum != 0.0
    address = lambda a: a.ctypes.data if a is not None else None
    for index, (staging, rate) in enumerate(zip(stagings, lrs)):
        spans = list(zip(layout.offsets, layout.counts))
        if defect == "decay_reaches_gap":
            spans = [(0, layout.n)]
        for k, (at, count) in enumerate(spans):
            if defect == "decay_reaches_gap":
                g = np.zeros(layout.n, dtype=np.float32)
                for j in range(len(layout.counts)):
                    if layout.uses[j]:
                        g[layout.offsets[j]:layout.offsets[j] + layout.counts[j]] = fold32(
                            [layout.slot(staging, j, s) for s in range(layout.uses[j])])
            else:
                uses = layout.uses[k]
                if uses == 0 and defect != "unused_segment_updated":
                    continue
                if defect == "one_slot_too_many":
                    uses += 1
                slots = [layout.slot(staging, k, s) for s in range(uses)] or [np.zeros(count, dtype=np.float32)]
                if defect == "reverse_order":
                    slots = slots[::-1]
                if defect == "float64_fold":
                    g = np.sum(np.array(slots, dtype=np.float64), axis=0).astype(np.float32)
                else:
                    g = fold32(slots)
            state["grads"][at:at + count] = g
            w = state["weights"][at:at + count].copy()
            m = state["moment1"][at:at + count].copy() if with_buffer else None
            v = state["moment2"][at:at + count].copy() if adam else None
            lr = np.full(1, rate, dtype=np.float64)
            done = np.full(1, index, dtype=np.int64)
            args = optref.opt_args(native, kind, count, address(w), address(g), address(m), address(v), address(lr),
                                   address(done), weight_decay=weight_decay, momentum=momentum)
            rc = lib.mztrain_opt_reference(ctypes.byref(args))
            assert rc == 0, (rc, lib.mzmcts_last_error(None))
            state["weights"][at:at + count] = w
            if with_buffer:
                state["moment1"][at:at + count] = m
            if adam:
                state["moment2"][at:at + count] = v
    state["steps_done"] = len(stagings)
    return state


def fold_args(native, kind, n, weights, grads, moment1, moment2, lr, steps_done, staging, staging_floats, weight_decay=0.0,
              momentum=0.0, **hyper):
    """mztrain_fold_args from raw addresses (host or device; None stays a null pointer)."""
    opt = optref.opt_args(native, kind, n, weights, grads, moment1, moment2, lr, steps_done, weight_decay=weight_decay,
                          momentum=momentum, **hyper)
    return native.MzTrainFoldArgs(opt=opt, staging=staging, staging_floats=staging_floats)


def uses_array(uses):
    return (ctypes.c_int32 * len(uses))(*[int(u) for u in uses])


def run_host_entry(native, layout, kind, weights, stagings, lrs, weight_decay=0.0, momentum=0.0):
    """The steps through mztrain_fold_reference on host arrays; the staging arrays are checked to come back unchanged."""
    lib = native.load()
    state = start_state(layout, weights)
    adam = kind == "Adam"
    with_buffer = adam or momentum != 0.0
    lr = np.zeros(1, dtype=np.float64)
    done = np.zeros(1, dtype=np.int64)
    segments = layout.segments(native)
    for staging, rate in zip(stagings, lrs):
        kept = staging.copy()
        lr[0] = rate
        args = fold_args(native, kind, layout.n, state["weights"].ctypes.data, state["grads"].ctypes.data,
                         state["moment1"].ctypes.data if with_buffer else None,
                         state["moment2"].ctypes.data if adam else None, lr.ctypes.data, done.ctypes.data,
                         staging.ctypes.data, layout.staging_floats, weight_decay=weight_decay, momentum=momentum)
        rc = lib.mztrain_fold_reference(segments, uses_array(layout.uses), len(layout.counts), ctypes.byref(args))
        assert rc == 0, (rc, lib.mzmcts_last_error(None))
        assert np.array_equal(staging.view(np.uint32), kept.view(np.uint32)), "the staging buffer was written"
    state["steps_done"] = int(done[0])
    return state


def tensors_of(kind, momentum):
    if kind == "Adam":
        return ("weights", "grads", "moment1", "moment2")
    return ("weights", "grads", "moment1") if momentum != 0.0 else ("weights", "grads")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def the_case_list():
    """(label, Layout) the CPU and the GPU tests walk: every count with every uses, aligned and not; then all counts in one
    list with mixed uses (an unused segment among them) so that chunks of several segments share a launch."""
    cases = []
    for aligned in (True, False):
        tag = "aligned" if aligned else "offset-by-a-float"
        for uses in USES:
            cases.append((f"each-count-uses{uses}-{tag}", Layout(COUNTS, [uses] * len(COUNTS), aligned=aligned)))
        cases.append((f"mixed-uses-{tag}", Layout(COUNTS + (2049, 16), [1, 2, 21, 0, 3, 21, 2, 5, 4, 0], aligned=aligned)))
    return cases


def plan_restated(counts):
    """(chunks as (segment, first, count), grid)."""
    chunks = [(k, first, min(CHUNK, count - first)) for k, count in enumerate(counts) for first in range(0, count, CHUNK)]
    return chunks, min(len(chunks), MAX_BLOCKS)
