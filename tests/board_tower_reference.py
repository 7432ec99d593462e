"""The yardstick of the board-conv tower tests: include/mzmcts.h mzmcts_board_tower's layer semantics in numpy (the
convolution itself through torch's float64 CPU convolution, held to a written-out numpy one), nothing taken from the
kernels (tests/test_gpu_board_towers.py drives the kernels, tests/test_board_tower_reference.py holds this file to
account without a GPU).

A tower is `layers = [(weight[cout, cin, 3, 3], scale[cout], shift[cout], relu, skip, rescale)]`:

    out_l = act( conv3x3(in_l, weight; padding 1) * scale + shift  (+ in_{l-1}[:, :cout]) )

  * layer l reads the previous layer's output (layer 0: the tower's input);
  * `skip` adds the input of the layer BEFORE ahead of the ReLU -- for l == 1 the tower's input, first cout channels;
  * a `rescale` layer's unit-rescaled output replaces its output for every later layer and every later skip;
  * the rescale is (x - min) / span per (sample, channel) plane, span += 1e-5 when below 1e-5.

Two modes over the same function (tower_reference):

  exact    the input, the weights, scale and shift are integers (or integers / `denom`, a power of two: a gathered
           action plane action / A): float64 arithmetic on them is exact, and so is every fp32 product and partial sum of
           any kernel in any order as long as nothing reaches 2^24 -- which is ASSERTED here, per layer, on
           sum |a| |w| |scale| + |shift| + |skip| and on every activation, so that a case can never be silently inexact.
           Cases meant for the split form (two fp16 halves of 8 x, range 8188) also assert |activation| < 8188 and
           |input| < 8188 (the `loose` samples of the overflow case excepted: those are held below 2^24 only).
           A rescale ends the exact regime: its quotients are no integers; the layers behind it are computed in float64
           from the float32 quotients and reported as not exact (`exact_upto`).
  float64  any data; nothing is asserted; the rescale is done in float64.

judge_exports is the verdict both test files share: every layer of a tower run with export_raw on every layer (and
export_unit on the rescale layers) is judged ON THE RUN'S OWN EXPORTED INPUT, so errors do not compound and a rescale's
division by a small span never amplifies an earlier layer's rounding into a later layer's verdict.
"""
import numpy as np

from parity_helpers import tower_layer_rounding_bound

F32 = np.float32
TWO24 = float(2 ** 24)
SPLIT_RANGE = 8188.0          # include/mzmcts.h: |activation| must stay below 8188 in the split form


def conv3x3_numpy(x, w):
    """Cross-correlation of x[b, cin, h, w] with w[cout, cin, 3, 3], padding 1, in float64, written out in numpy:
    out[y, x] = sum w[ty, tx] in[y + ty - 1, x + tx - 1] (torch conv2d's convention)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    b, c, h, wd = x.shape
    o = w.shape[0]
    assert w.shape == (o, c, 3, 3), (w.shape, x.shape)
    padded = np.zeros((b, h + 2, wd + 2, c))
    padded[:, 1:-1, 1:-1] = x.transpose(0, 2, 3, 1)
    out = np.zeros((b * h * wd, o))
    for ty in range(3):
        for tx in range(3):
            out += np.ascontiguousarray(padded[:, ty:ty + h, tx:tx + wd]).reshape(-1, c) @ w[:, :, ty, tx].T
    return out.reshape(b, h, wd, o).transpose(0, 3, 1, 2)


def conv3x3_f64(x, w):
    """The same convolution through torch's float64 CPU convolution (ten times quicker on the large cases; the CPU test
    file holds the two to each other -- on integers they agree exactly, whatever order either sums in)."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    assert w.shape[1:] == (x.shape[1], 3, 3), (tuple(w.shape), tuple(x.shape))
    return torch.nn.functional.conv2d(x, w, padding=1).numpy()


def unit_rescale_f32(raw):
    """(x - min) / span per (sample, channel) plane in float32, span += 1e-5 below 1e-5: two correctly rounded float32
    operations per element, the expression the fp32 towers must reproduce bit for bit on their own raw export."""
    raw = np.asarray(raw, dtype=F32)
    low = raw.min(axis=(2, 3), keepdims=True)
    high = raw.max(axis=(2, 3), keepdims=True)
    span = (high - low).astype(F32)
    span = np.where(span < F32(1e-5), (span + F32(1e-5)).astype(F32), span)
    return ((raw - low).astype(F32) / span).astype(F32)


def unit_rescale_f64(raw):
    raw = np.asarray(raw, dtype=np.float64)
    low = raw.min(axis=(2, 3), keepdims=True)
    high = raw.max(axis=(2, 3), keepdims=True)
    span = high - low
    span = np.where(span < 1e-5, span + 1e-5, span)
    return (raw - low) / span


def split22(v):
    """What the split tower keeps of a float32 value: 8 v as two fp16 halves, h0 = fp16(8 v), h1 = fp16(8 v - h0), read
    back as (h0 + h1) / 8 (board_tower_split_kernel store_val / load_val; the sum and the scaling are exact in float32)."""
    with np.errstate(over="ignore", invalid="ignore"):
        vs = (np.asarray(v, dtype=F32) * F32(8.0)).astype(F32)
        h0 = vs.astype(np.float16)
        h1 = (vs - h0.astype(F32)).astype(F32).astype(np.float16)
        return ((h0.astype(F32) + h1.astype(F32)) * F32(0.125)).astype(F32)


def layer_f64(inp, layer, skip_src):
    """One layer in float64: (output, conv, sum |a| |w|) with `skip_src` the planes a skip adds (or None)."""
    weight, scale, shift, relu, skip, _ = layer
    cout = weight.shape[0]
    conv = conv3x3_f64(inp, weight)
    magnitude = conv3x3_f64(np.abs(inp), np.abs(np.asarray(weight, dtype=np.float64)))
    v = conv * np.asarray(scale, dtype=np.float64).reshape(1, cout, 1, 1) + np.asarray(shift, dtype=np.float64).reshape(1, cout, 1, 1)
    if skip:
        v = v + skip_src
    if relu:
        v = np.maximum(v, 0.0)
    return v, conv, magnitude


def _skip_source(l, x, outs, cout):
    """The input of layer l - 1: the tower's input (first cout channels) for l == 1, else what layer l - 2 left."""
    assert l >= 1, "layer 0 has no layer before it: a skip there is not defined"
    if l == 1:
        assert x.shape[1] >= cout, "a skip from the tower's input needs at least `channels` input planes"
        return x[:, :cout]
    return outs[l - 2]


def tower_reference(x, layers, exact=False, split=False, denom=1, loose=()):
    """Every layer's raw output and, for rescale layers, its unit-rescaled output (None elsewhere), chained as the header
    says.  Returns dict(raw, unit, magnitude = max sum |a| |w| per layer, max_activation, exact_upto = index of the last
    layer computed exactly (exact mode: the first rescale layer, or the last layer))."""
    x = np.asarray(x, dtype=np.float64)
    held = np.ones(x.shape[0], dtype=bool)
    held[list(loose)] = False

    def check(values, what, l):
        assert np.array_equal(values * denom, np.round(values * denom)), f"{what} of layer {l}: not a multiple of 1 / {denom}"
        assert float(np.abs(values).max(initial=0.0)) * denom < TWO24, f"{what} of layer {l} reaches 2^24"
        if split:
            assert float(np.abs(values[held]).max(initial=0.0)) < SPLIT_RANGE, f"{what} of layer {l} leaves the split range"

    if exact:
        check(x, "input", 0)
    raws, units, outs, magnitudes = [], [], [], []
    exact_upto, still_exact, top = len(layers) - 1, exact, float(np.abs(x).max(initial=0.0))
    for l, layer in enumerate(layers):
        weight, scale, shift, relu, skip, rescale = layer
        cout = weight.shape[0]
        inp = x if l == 0 else outs[l - 1]
        src = _skip_source(l, x, outs, cout) if skip else None
        v, conv, magnitude = layer_f64(inp, layer, src)
        if still_exact:
            for name, values in (("weight", weight), ("scale", scale), ("shift", shift)):
                assert np.array_equal(values, np.round(values)), f"{name} of layer {l}: not integers"
            partial = magnitude * np.abs(np.asarray(scale, dtype=np.float64)).reshape(1, cout, 1, 1) \
                + np.abs(np.asarray(shift, dtype=np.float64)).reshape(1, cout, 1, 1) + (np.abs(src) if skip else 0.0)
            assert float(partial.max()) * denom < TWO24, f"partial sums of layer {l} reach 2^24"
            check(v, "activation", l)
        raws.append(v)
        magnitudes.append(float(magnitude.max(initial=0.0)))
        top = max(top, float(np.abs(v).max(initial=0.0)))
        out = v
        if rescale:
            unit = unit_rescale_f32(v).astype(np.float64) if exact else unit_rescale_f64(v)
            if split and exact:
                unit = split22(unit).astype(np.float64)
            units.append(unit)
            out = unit
            if still_exact:
                exact_upto, still_exact = l, False
        else:
            units.append(None)
        outs.append(out)
    return dict(raw=raws, unit=units, magnitude=magnitudes, max_activation=top, exact_upto=exact_upto)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=F32)
    b = np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def judge_exports(x, layers, raws, units, split=False, reference=None, samples=None):
    """The verdict on one tower run whose every layer exported its raw output (float32 [b, cout, h, w]) and whose rescale
    layers exported their unit output.  `x` is the tower's input as float32 (a gathered input assembled: pool rows + the
    action plane).  Returns (failures, worst): failures = [(layer, what, detail)], worst = the largest error / bound met,
    as dict(all=..., ordinary=...): `ordinary` leaves out channels with |scale| < 1/4 (a tiny-span channel computes
    1 + 2^-22 conv, whose one rounding next to 1.0 IS the bound: its ratio says nothing about the accumulation).

      float64, layer by layer   raws[l] against act(conv64(got_{l-1}) * scale + shift (+ got_{l-2})) computed from the
                                run's OWN exports (the unit export where one was made), within
                                parity_helpers.tower_layer_rounding_bound;
      unit exports              bit for bit the numpy float32 expression on the run's own raw export -- for the split form
                                that expression's value as the form stores it (split22): board_tower_split_kernel rescales
                                the float32 values h0 + h1 (load_val) with the same two float32 operations, and writes
                                the quotient back as two fp16 halves before it exports it;
      exact (reference given)   raws[l] == the integers of tower_reference(..., exact=True) for every l <= exact_upto.
    `samples`: judge the split store rounding only on these (boolean mask; the overflow case: samples the fp32 tower
    re-ran carry none)."""
    x = np.asarray(x, dtype=F32)
    failures, worst = [], dict(all=0.0, ordinary=0.0)
    got = []          # what layer l left for the following layers, as float64
    stored = np.ones(x.shape[0], dtype=bool) if samples is None else np.asarray(samples, dtype=bool)
    for l, layer in enumerate(layers):
        weight, scale, shift, relu, skip, rescale = layer
        cout = weight.shape[0]
        raw = np.asarray(raws[l], dtype=F32)
        inp = x.astype(np.float64) if l == 0 else got[l - 1]
        src = _skip_source(l, x.astype(np.float64), got, cout) if skip else None
        want, conv, magnitude = layer_f64(inp, layer, src)
        bound = tower_layer_rounding_bound(magnitude, conv, scale, shift, src, split_store=False)
        if split:
            with_store = tower_layer_rounding_bound(magnitude, conv, scale, shift, src, split_store=True)
            bound = np.where(stored.reshape(-1, 1, 1, 1), with_store, bound)
        err = np.abs(raw.astype(np.float64) - want)
        if not np.all(err <= bound):
            bad = np.argwhere(~(err <= bound))[0]
            failures.append((l, "raw", f"at {tuple(int(i) for i in bad)}: got {raw[tuple(bad)]!r}, want {want[tuple(bad)]!r}, "
                                       f"bound {bound[tuple(bad)]:.3e}"))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        if np.all(np.isfinite(ratio)):
            worst["all"] = max(worst["all"], float(ratio.max(initial=0.0)))
            ordinary = np.abs(np.asarray(scale, dtype=np.float64)) >= 0.25
            worst["ordinary"] = max(worst["ordinary"], float(ratio[:, ordinary].max(initial=0.0)))
        if reference is not None and l <= reference["exact_upto"] and not np.array_equal(raw.astype(np.float64), reference["raw"][l]):
            bad = np.argwhere(raw.astype(np.float64) != reference["raw"][l])[0]
            failures.append((l, "exact", f"at {tuple(int(i) for i in bad)}: got {raw[tuple(bad)]!r}, "
                                         f"want {reference['raw'][l][tuple(bad)]!r}"))
        out = raw
        if rescale:
            unit = np.asarray(units[l], dtype=F32)
            want_unit = unit_rescale_f32(raw)
            if split:
                want_unit = np.where(stored.reshape(-1, 1, 1, 1), split22(want_unit), want_unit)
            if not same_bits(unit, want_unit):
                bad = np.argwhere(unit.view(np.uint32) != want_unit.view(np.uint32))[0]
                failures.append((l, "unit", f"at {tuple(int(i) for i in bad)}: got {unit[tuple(bad)]!r}, want {want_unit[tuple(bad)]!r}"))
            out = unit
        got.append(out.astype(np.float64))
    return failures, worst
