"""tests/board_tower_reference.py (the yardstick of tests/test_gpu_board_towers.py) and tests/board_tower_cases.py held
to account without a GPU:

  * the yardstick equals the module path (ResidualBlock stacks, conv_epilogue, _unit_rescale of models.py) in float64;
  * its exact mode and its float64 mode agree on integer towers, and every integer case passes the exact-mode assertions;
  * the float64-mode bound holds for a float32 k-ordered fmaf chain emulated in numpy;
  * DISCRIMINATING POWER: a CPU emulation of a tower with one deliberate defect at a time is rejected by the case set.
"""
import importlib

import numpy as np
import pytest
import torch

import board_tower_cases as cases
import board_tower_reference as ref
from parity_helpers import synthetic_model, tower_layer_rounding_bound

F32 = np.float32


# ---- a tower as the kernels compute it, in numpy: float32 epilogue operations on a correctly rounded convolution ----------
def emulate_tower(x, layers, split=False, defect=None):
    """Every layer's (raw, unit) exports of a float32 tower chained on its own outputs.  The convolution is float64 rounded
    once to float32 (exact on integer data, a tenth of the chain bar otherwise); the epilogue is board_conv.hip's: multiply,
    add, skip, ReLU, one float32 rounding each; the split form keeps split22 of every value.  `defect`: one deliberate
    mistake (see DEFECTS)."""
    keep = ref.split22 if split else (lambda v: np.asarray(v, dtype=F32))
    x = keep(x)
    outs, pre_rescale, raws, units = [], [], [], []
    for l, (weight, scale, shift, relu, skip, rescale) in enumerate(layers):
        cout = weight.shape[0]
        inp = x if l == 0 else outs[l - 1]
        if defect == "raw_planes_read" and l >= 1:
            inp = pre_rescale[l - 1]
        w = weight
        if defect == "taps_transposed":
            w = np.ascontiguousarray(weight.transpose(0, 1, 3, 2))
        if defect == "last_channel_dropped" and l == 0:
            inp = inp.copy()
            inp[:, -1] = 0
        if defect == "low_half_dropped":
            with np.errstate(over="ignore"):
                inp = ((inp * F32(8)).astype(np.float16).astype(F32) * F32(0.125)).astype(F32)
        acc = ref.conv3x3_f64(inp, w).astype(F32)
        v = (acc * scale.reshape(1, cout, 1, 1)).astype(F32)
        v = (v + shift.reshape(1, cout, 1, 1)).astype(F32)
        if defect == "relu_before_skip" and relu:
            v = np.maximum(v, F32(0))
        if skip:
            if l == 1:
                src = x[:, :cout]
            elif defect == "skip_pre_rescale":
                src = pre_rescale[l - 2]
            else:
                src = outs[l - 2]
            if defect == "skip_from_previous_layer":
                src = inp[:, :cout]
            v = (v + src).astype(F32)
        if relu:
            v = np.maximum(v, F32(0))
        v = keep(v)
        raw, unit, out = v, None, v
        if rescale:
            unit = keep(ref.unit_rescale_f32(v))
            out = unit
            if defect == "rescaled_raw_export":
                raw = unit
        raws.append(raw)
        units.append(unit)
        outs.append(out)
        pre_rescale.append(v)
    return raws, units


def _verdict(case, x, split=False, defect=None, denom=1, emulated_input=None):
    reference = ref.tower_reference(x, case["layers"], exact=True, split=split, denom=denom) if case["integer"] else None
    raws, units = emulate_tower(x if emulated_input is None else emulated_input, case["layers"], split=split, defect=defect)
    return ref.judge_exports(x, case["layers"], raws, units, split=split, reference=reference)


def _case_set():
    """(case, split) pairs at small shapes: what the GPU file runs, one board and channel count each."""
    out = []
    for h, w, cin0, channels, split in ((3, 3, 17, 16, False), (6, 7, 65, 64, False), (6, 7, 65, 64, True), (6, 6, 64, 64, True)):
        for case in cases.standard_cases(h, w, cin0, channels, split=split):
            out.append((case, split))
    out.append((cases.deep_case(3, 3, 17, 16), False))
    out.append((cases.deep_case(6, 7, 64, 64), True))
    return out


# ---- the yardstick against the modules ------------------------------------------------------------------------------
def _layers_of(block_layers):
    out = []
    for conv, bn, relu, skip in block_layers:
        scale, shift = bn.folded()
        out.append((conv.weight.detach().numpy(), scale.detach().numpy(), shift.detach().numpy(), relu, skip, 0))
    return out


@pytest.mark.parametrize("game", ["tictactoe", "connect4"])
def test_yardstick_equals_the_module_path_in_float64(game):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    config = importlib.import_module(f"muzero-hypermodel_amd.games.{game}").MuZeroConfig()
    model, _ = synthetic_model(models, config, "cpu")
    model = model.double()
    model.refresh_inference_constants()
    dyn, pred = model.dynamics_network.module, model.prediction_network.module
    c = dyn.conv.out_channels
    h, w = config.observation_shape[1], config.observation_shape[2]
    rs = np.random.RandomState(3)
    batch = 5
    with torch.no_grad():
        # dynamics + rescale + prediction: the layer list _recurrent_tower hands to the launch
        planes = torch.from_numpy(rs.standard_normal((batch, c + 1, h, w)))
        block_layers = [(dyn.conv, dyn.bn, 1, 0)] + model._block_layers(dyn.resblocks)
        last_dyn = len(block_layers) - 1
        block_layers += model._block_layers(pred.resblocks)
        layers = _layers_of(block_layers)
        layers[last_dyn] = layers[last_dyn][:5] + (1,)
        y = models.conv_epilogue(dyn.conv(planes), dyn.bn)
        for block in dyn.resblocks:
            y = block(y)
        raw = y
        shifted, span = models._unit_rescale(raw, (2, 3))
        state = shifted / span
        y = state
        for block in pred.resblocks:
            y = block(y)
        got = ref.tower_reference(planes.numpy(), layers)
        np.testing.assert_allclose(got["raw"][last_dyn], raw.numpy(), rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(got["unit"][last_dyn], state.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["raw"][-1], y.numpy(), rtol=1e-9, atol=1e-11)
        assert all(u is None for i, u in enumerate(got["unit"]) if i != last_dyn)

        # a root tower that starts with a residual block (the down-sampled representation): layer 1's skip is the input
        x = torch.from_numpy(rs.standard_normal((batch, c, h, w)))
        block_layers = model._block_layers(pred.resblocks)
        last_rep = len(block_layers) - 1
        block_layers += model._block_layers(dyn.resblocks)
        layers = _layers_of(block_layers)
        layers[last_rep] = layers[last_rep][:5] + (1,)
        assert layers[1][4] == 1
        y = x
        for block in pred.resblocks:
            y = block(y)
        shifted, span = models._unit_rescale(y, (2, 3))
        y = state = shifted / span
        for block in dyn.resblocks:
            y = block(y)
        got = ref.tower_reference(x.numpy(), layers)
        np.testing.assert_allclose(got["unit"][last_rep], state.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["raw"][-1], y.numpy(), rtol=1e-9, atol=1e-11)


def test_exact_mode_and_float64_mode_agree_and_every_integer_case_is_exact():
    """tower_reference(exact=True) asserts < 2^24 (and < 8188 for split cases) per layer; up to the first rescale the two
    modes return the same numbers, and the rescale differs by float32 rounding only."""
    seen = 0
    for case, split in _case_set():
        if not case["integer"]:
            continue
        x = cases.case_input(case, 9, 17, const_plane=split)
        exact = ref.tower_reference(x, case["layers"], exact=True, split=split)
        plain = ref.tower_reference(x, case["layers"])
        upto = exact["exact_upto"]
        for l in range(upto + 1):
            assert np.array_equal(exact["raw"][l], plain["raw"][l]), (case["name"], l)
        if case["layers"][upto][5]:
            np.testing.assert_allclose(exact["unit"][upto], plain["unit"][upto], rtol=3e-7, atol=1e-7)
        live = [float((exact["raw"][l] > 0).mean()) for l in range(upto + 1) if case["layers"][l][3]]
        assert min(live, default=1.0) > 0.1, (case["name"], live)          # the ReLU does not kill the tower
        assert exact["max_activation"] < (ref.SPLIT_RANGE if split else ref.TWO24)
        seen += 1
    assert seen >= 15
    # gathered input: multiples of 1 / 8
    case = cases.standard_cases(6, 7, 65, 64, split=True)[2]
    pool, parent, action, A = cases.case_gather(case, 11, 5)
    x = cases.gathered_input(case, pool, parent, action, A)
    with pytest.raises(AssertionError):
        ref.tower_reference(x, case["layers"], exact=True, split=True)      # (not integers)
    ref.tower_reference(x, case["layers"], exact=True, split=True, denom=A)


def test_the_two_float64_convolutions_agree():
    rs = np.random.RandomState(0)
    for b, cin, cout, h, w in ((3, 17, 16, 3, 3), (5, 65, 64, 6, 7), (2, 1, 16, 6, 6)):
        x = rs.randint(-3, 4, size=(b, cin, h, w)).astype(F32)
        weight = rs.randint(-2, 3, size=(cout, cin, 3, 3)).astype(F32)
        assert np.array_equal(ref.conv3x3_f64(x, weight), ref.conv3x3_numpy(x, weight))
        x = rs.standard_normal((b, cin, h, w))
        weight = rs.standard_normal((cout, cin, 3, 3))
        np.testing.assert_allclose(ref.conv3x3_f64(x, weight), ref.conv3x3_numpy(x, weight), rtol=0, atol=1e-12 * 9 * cin)


def test_exact_mode_refuses_what_is_not_exact():
    case = cases.integer_tower("big", 1, 3, 3, 16, 16, 2)
    x = cases.case_input(case, 3, 1)
    with pytest.raises(AssertionError, match="2\\^24"):
        ref.tower_reference(x * F32(2 ** 22), case["layers"], exact=True)
    with pytest.raises(AssertionError, match="split range"):
        ref.tower_reference(x * F32(4000), case["layers"], exact=True, split=True)
    with pytest.raises(AssertionError, match="not a multiple"):
        ref.tower_reference(x + F32(0.5), case["layers"], exact=True)


def test_gate_case_overflows_where_it_says():
    case, x, loose = cases.gate_case()
    keep = list(range(8)) + list(range(1022, 1029))          # (samples are independent: the flagged ones and neighbours)
    x, loose = x[keep], [keep.index(s) for s in loose]
    at = {s: keep.index(s) for s in (5, 1026, 1028)}
    with pytest.raises(AssertionError, match="split range"):
        ref.tower_reference(x, case["layers"], exact=True, split=True)
    got = ref.tower_reference(x, case["layers"], exact=True, split=True, loose=loose)
    assert np.abs(x[at[5]]).max() >= 8190 and np.abs(x[[at[1026], at[1028]]]).max() < ref.SPLIT_RANGE
    for s in (at[1026], at[1028]):
        tops = [float(np.abs(r[s]).max()) for r in got["raw"]]
        assert max(tops) >= 8190 and not any(ref.SPLIT_RANGE <= t < 8190 for t in tops), tops
    assert got["max_activation"] < ref.TWO24


@pytest.mark.parametrize("cin", [17, 80])
def test_bound_holds_for_an_fmaf_chain_in_float32(cin):
    """One layer as a k-ordered float32 fmaf chain over K = 9 cin terms (taps outermost, channels inside: the kernels'
    order), then the epilogue's three float32 operations, against the float64 layer: inside the bound, and not by orders
    of magnitude (a bound nobody can miss checks nothing)."""
    rs = np.random.RandomState(cin)
    b, cout, h, w = 6, 16, 3, 3
    x = rs.standard_normal((b, cin, h, w)).astype(F32)
    weight = (rs.standard_normal((cout, cin, 3, 3)) / (9 * cin) ** 0.5).astype(F32)
    scale = rs.uniform(0.5, 1.5, cout).astype(F32) * rs.choice([-1.0, 1.0], size=cout).astype(F32)
    shift = rs.standard_normal(cout).astype(F32)
    skip = rs.standard_normal((b, cout, h, w)).astype(F32)
    padded = np.zeros((b, cin, h + 2, w + 2), dtype=F32)
    padded[:, :, 1:-1, 1:-1] = x
    acc = np.zeros((b, cout, h, w), dtype=F32)
    for tap in range(9):
        for ci in range(cin):
            a = padded[:, ci, tap // 3:tap // 3 + h, tap % 3:tap % 3 + w].astype(np.float64)[:, None]
            wv = weight[:, ci, tap // 3, tap % 3].astype(np.float64).reshape(1, cout, 1, 1)
            acc = (a * wv + acc.astype(np.float64)).astype(F32)          # fmaf: the product is exact in float64
    v = (acc * scale.reshape(1, cout, 1, 1)).astype(F32)
    v = (v + shift.reshape(1, cout, 1, 1)).astype(F32)
    v = np.maximum((v + skip).astype(F32), F32(0))
    layer = (weight, scale, shift, 1, 1, 0)
    want, conv, magnitude = ref.layer_f64(x, layer, skip.astype(np.float64))
    bound = tower_layer_rounding_bound(magnitude, conv, scale, shift, skip.astype(np.float64))
    ratio = float((np.abs(v.astype(np.float64) - want) / bound).max())
    print(f"fmaf chain, K = {9 * cin}: worst error / bound = {ratio:.3f}")
    assert 0.02 < ratio < 1.0


# ---- discriminating power -------------------------------------------------------------------------------------------
DEFECTS = ["skip_from_previous_layer", "skip_pre_rescale", "taps_transposed", "last_channel_dropped", "relu_before_skip",
           "rescaled_raw_export", "raw_planes_read", "low_half_dropped"]
# the case and layer each defect must be rejected on (fp32 form of the 3 x 3 cases unless it says split)
REJECTED_ON = {
    "skip_from_previous_layer": ("dynpred5-3x3-17to16", 2),
    "skip_pre_rescale": ("dynpred5-3x3-17to16", 4),
    "taps_transposed": ("one-3x3-17to16", 0),
    "last_channel_dropped": ("one-3x3-17to16", 0),
    "relu_before_skip": ("dynpred5-3x3-17to16", 2),
    "rescaled_raw_export": ("dynpred5-3x3-17to16", 2),
    "raw_planes_read": ("dynpred5-3x3-17to16", 3),
    "low_half_dropped": ("float5-6x7-65to64", 0),
}


def test_the_emulation_without_a_defect_passes_every_case():
    for case, split in _case_set():
        x = cases.case_input(case, 7, 23, const_plane=split)
        failures, worst = _verdict(case, x, split=split)
        assert not failures, (case["name"], split, failures[:2])
        assert worst["all"] <= 1.0


@pytest.mark.parametrize("defect", DEFECTS)
def test_one_defect_at_a_time_is_rejected(defect):
    name, layer = REJECTED_ON[defect]
    rejected = {}
    for case, split in _case_set():
        if defect == "low_half_dropped" and (case["integer"] or not split):
            continue                                 # (the low half of an integer below 8188 is zero: float64 mode only)
        x = cases.case_input(case, 7, 23, const_plane=split)
        failures, _ = _verdict(case, x, split=split, defect=defect)
        if failures:
            rejected[(case["name"], split)] = sorted({f[0] for f in failures})
    key = (name, defect == "low_half_dropped")
    assert key in rejected and layer in rejected[key], (defect, rejected)
    print(defect, "rejected by", len(rejected), "towers")


def test_a_shifted_action_plane_is_rejected():
    """Sample b reading sample b - 1's action plane: the gathered cases (exact: action / 8, float64 mode: action / 7)."""
    for integer in (True, False):
        case = [c for c in cases.standard_cases(3, 3, 17, 16) if c["integer"] == integer][0]
        pool, parent, action, A = cases.case_gather(case, 9, 31)
        assert len(set(action.tolist())) > 2
        x = cases.gathered_input(case, pool, parent, action, A)
        wrong = cases.gathered_input(case, pool, parent, action, A, action_shift=1)
        assert not _verdict(case, x, denom=A)[0]
        failures, _ = _verdict(case, x, denom=A, emulated_input=wrong)
        assert failures and failures[0][0] == 0, (case["name"], failures[:1])


def test_sixty_four_channels_on_3x3_boards_have_no_tower(pkg):
    """mzmcts_board_conv_supported(.., 64, 3, 3) speaks for the single-layer kernel; the towers refuse that shape before
    anything is launched (two activation buffers of 16 boards never fitted a workgroup's LDS: the launch lines
    launch_board_tower<4,3,3,16> and launch_board_tower_split<3,3,16> could not run, and are gone).  No pointer is followed
    on the way to the refusal, so this runs without a GPU."""
    import ctypes
    native = importlib.import_module("muzero-hypermodel_amd._native")
    lib = native.load()
    assert lib.mzmcts_board_conv_supported(64, 64, 3, 3)
    room = np.zeros(256, dtype=F32)
    aligned = (room.ctypes.data + 15) // 16 * 16
    for cin0 in (1, 64, 65, 80):
        layers = (native.MzTowerLayer * 2)(*[native.MzTowerLayer(aligned, aligned, aligned, aligned, None, None, cin, 1, 0, 0, None)
                                             for cin in (cin0, 64)])
        assert lib.mzmcts_board_tower(aligned, 16, cin0, 64, 3, 3, ctypes.addressof(layers), 2, None) == -1
        assert lib.mzmcts_board_tower_split(aligned, 16, cin0, 0, 64, 3, 3, ctypes.addressof(layers), 2, None) == -1
    # the split form never stages its constant plane: a layer-1 skip that would read it (cin0 <= channels) is refused
    for cin0, const_plane, skip, want in ((64, 1, 1, -1), (2, 1, 1, -1)):
        layers = (native.MzTowerLayer * 2)(*[native.MzTowerLayer(aligned, aligned, aligned, aligned, None, None, cin, 1, s, 0, None)
                                             for cin, s in ((cin0, 0), (64, skip))])
        assert lib.mzmcts_board_tower_split(aligned, 4, cin0, const_plane, 64, 6, 7, ctypes.addressof(layers), 2, None) == want
    gather = native.MzTowerGather(aligned, aligned, aligned, 16, 64 * 9, 9.0)
    layers = (native.MzTowerLayer * 1)(native.MzTowerLayer(aligned, aligned, aligned, aligned, None, None, 65, 1, 0, 0, None))
    for split in (0, 1):
        assert lib.mzmcts_board_tower_gathered(ctypes.byref(gather), 16, 65, split, 64, 3, 3, ctypes.addressof(layers), 1, None) == -1
