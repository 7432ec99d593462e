"""The yardsticks of tests/test_gpu_net_heads.py and tests/test_gpu_downsample.py held to account on the CPU:

  * they are models.PointwiseConv2d + models.mlp, and models.DownsampleCNN, in float64 (1e-12 relative);
  * torch's float32 module path stays inside the derived bounds on every case: the bounds are bounds;
  * every integer case meets the conditions of exact mode (integral, ELU the identity, partial sums below 2^24, pooling
    windows of 1, 2, 4, 8 or 16 elements);
  * the dispatch restated in tests/net_head_cases.py gives every case the kernel it claims, and every kernel and every
    compile-time form has a case;
  * DISCRIMINATING POWER: a copy of each yardstick with one deliberate defect at a time breaks the bound on a named case
    and element -- the rigorous gamma(K + 2) bound still bites.
"""
import importlib

import numpy as np
import pytest
import torch

import downsample_reference as dref
import net_head_cases as cases
import net_head_reference as href

F64 = np.float64


def _small_batch(case):
    return min(9, max(case["batches"]))


# ---- heads ----------------------------------------------------------------------------------------------------------
def _torch_head(models, shape, p, dtype):
    c, plane, r, hd, o = shape
    conv = models.PointwiseConv2d(c, r)
    fc = models.mlp(r * plane, [hd], o)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(p["conv_w"]).reshape(r, c, 1, 1))
        conv.bias.copy_(torch.from_numpy(p["conv_b"]))
        fc[0].weight.copy_(torch.from_numpy(p["w1"]))
        fc[0].bias.copy_(torch.from_numpy(p["b1"]))
        fc[2].weight.copy_(torch.from_numpy(p["w2"]))
        fc[2].bias.copy_(torch.from_numpy(p["b2"]))
    return conv.to(dtype), fc.to(dtype)


@pytest.mark.parametrize("case_id", sorted(cases.HEAD_CASES))
def test_head_yardstick_is_the_module_path_and_its_bound_holds_in_float32(pkg, case_id):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    case = cases.HEAD_CASES[case_id]
    n = _small_batch(case)
    for integer in (True, False):
        params, boards = cases.case_data(case_id, integer)
        for shape, p, x in zip(case["shapes"], params, boards):
            x = x[:n]
            want, bound = href.head_reference(x, p, exact=integer)
            board = torch.from_numpy(x).reshape(n, shape[0], 1, shape[1])
            with torch.no_grad():
                conv, fc = _torch_head(models, shape, p, torch.float64)
                in64 = fc(conv(board.double()).reshape(n, -1)).numpy()
                conv, fc = _torch_head(models, shape, p, torch.float32)
                in32 = fc(conv(board).reshape(n, -1)).numpy()
            assert np.abs(in64 - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (case_id, shape)
            if integer:
                assert np.array_equal(in32.astype(F64), want), (case_id, shape, "torch's float32 leaves the integers")
            else:
                ratio, where = href.judge(in32, want, bound)
                assert ratio <= 1.0, (case_id, shape, ratio, where)
                # the inputs leave nothing undecided: the bound is far below the logits' own spread
                assert bound.max() < 0.05 * max(want.std(), 0.1), (case_id, shape, bound.max(), want.std())
                _, pre, _ = href.head_layers(x, p)
                if pre.size >= 32:
                    assert 0.2 < (pre < 0).mean() < 0.8, (case_id, shape, "hidden pre-activations of one sign")


def test_every_head_case_reaches_the_kernel_it_claims():
    """cases.dispatch restates mzmcts_conv_heads_multi (csrc/net_kernels.hip: launch_board_heads_cols first, then
    mfma_head_ok and MfmaHeadShape::total() <= 160 KB, then HeadShape::total() <= 160 KB, else MZMCTS_ERR_INVALID)."""
    C = cases.HEAD_CASES
    for case_id, case in C.items():
        assert cases.dispatch(case["shapes"], case["cols_off"]) == case["kernel"], case_id
        assert all(s[:2] == case["shapes"][0][:2] for s in case["shapes"]), case_id      # (heads agree on channels and plane)
    assert {c["kernel"] for c in C.values()} == {"cols", "mfma", "wave", "none"}
    forms = {cases.mfma_form(s) for c in C.values() if c["kernel"] == "mfma" for s in c["shapes"]}
    assert forms == cases.ALL_MFMA_FORMS, cases.ALL_MFMA_FORMS - forms
    # the paths the table names
    assert cases.mfma_form(C["H4"]["shapes"][0]) == (4, 2, 16, 2) and (17 + 15) // 16 == 2           # nt1 = 2 -> NT1 = 4
    assert (C["H5"]["shapes"][0][3] + 15) // 16 == 3 and C["H5"]["shapes"][0][4] == 32               # nt1 = 3, O full
    assert cases.mfma_form(C["H6"]["shapes"][0]) == (4, 2, 16, 2)
    assert cases.mfma_form(C["H7a"]["shapes"][0]) == (1, 2, 4, 6) and cases.cols_ok(C["H7a"]["shapes"][0])
    h8 = C["H8"]["shapes"]
    assert 80 * 1024 < 4 * cases.mfma_total(h8[0]) <= 160 * 1024 and cases.samples_per_round(h8, "mfma") == 16384
    assert C["H8"]["batches"] == (16384, 16384 + 17)                 # one round exactly; a second, ragged one
    for name in ("H1", "H2"):
        assert C[name]["shapes"][0][1] < 6                           # P < G
    assert C["H3"]["shapes"][0][1] == 6 and C["H4"]["shapes"][0][1] == 7
    assert len(C["H9c"]["shapes"]) == 2 and len(C["H9d"]["shapes"]) == 3 and len(C["H11"]["shapes"]) == 3
    w = {k: C[k]["shapes"][0] for k in C if k.startswith("W")}
    assert (w["W1"][0] * w["W1"][1]) % 4 != 0 and cases.wave_split(w["W1"][3]) == 64 and w["W1"][4] > 32
    assert (w["W2"][0] * w["W2"][1]) % 4 == 0 and cases.wave_split(w["W2"][3]) == 8 and w["W2"][2] > 16
    assert w["W3"][3] > w["W3"][2] * w["W3"][1] and cases.wave_split(w["W3"][3]) == 1
    assert [cases.wave_split(w[k][3]) for k in ("W4a", "W4b", "W4c", "W4d", "W4e")] == [2, 1, 1, 1, 1]
    assert [(w[k][3] - 1) // 64 for k in ("W4c", "W4d", "W4e")] == [0, 1, 2] and w["W4a"][4] > 64 > w["W4a"][3]
    assert cases.mfma_head_ok(w["W5"]) and 4 * cases.mfma_total(w["W5"]) > 160 * 1024
    assert cases.samples_per_round(C["W6"]["shapes"], "wave") == 8192 and C["W6"]["batches"] == (8192, 8192 + 5)
    r1 = C["R1"]["shapes"][0]
    assert cases.mfma_head_ok(r1) and 4 * cases.mfma_total(r1) > 160 * 1024 and 4 * cases.wave_total(r1) > 160 * 1024


def _defective_head(x, p, defect):
    """A copy of net_head_reference.head_layers with one deliberate defect."""
    x = np.asarray(x, dtype=F64).copy()
    conv_w, conv_b, w1, b1, w2, b2 = (np.asarray(p[k], dtype=F64).copy() for k in href.KEYS)
    batch = x.shape[0]
    if defect == "ragged_last_reads_neighbour":
        x[-1] = x[-2]
    if defect == "last_channel_dropped":
        conv_w[:, -1] = 0.0
    if defect == "conv_bias_last_dropped":
        conv_b[-1] = 0.0
    y = np.einsum("rc,bcp->brp", conv_w, x) + conv_b[None, :, None]
    flat = (y.transpose(0, 2, 1) if defect == "flatten_p_major" else y).reshape(batch, -1)
    if defect == "linear1_last_k_dropped":
        w1[:, -1] = 0.0
    if defect == "last_unit_row_zeroed":
        w1[-1, :] = 0.0
    pre = flat @ w1.T + b1
    if defect == "relu_for_elu":
        h = np.maximum(pre, 0.0)
    elif defect == "elu_without_minus_one":
        h = np.where(pre > 0, pre, np.exp(np.minimum(pre, 0.0)))
    else:
        h = href.elu64(pre)
    if defect == "linear2_reads_next_unit":
        h = np.roll(h, -1, axis=1)
    if defect == "b2_last_dropped":
        b2[-1] = 0.0
    return h @ w2.T + b2


# defect -> (case, batch, (sample, logit)) it must be rejected on (float data, first head of the case)
HEAD_DEFECTS = {
    "flatten_p_major": ("H2", 9, (5, 0)),
    "last_channel_dropped": ("H5", 9, (5, 23)),
    "conv_bias_last_dropped": ("H4", 9, (1, 8)),
    "linear1_last_k_dropped": ("H6", 9, (2, 7)),
    "relu_for_elu": ("H3", 9, (4, 4)),
    "elu_without_minus_one": ("H3", 9, (3, 11)),
    "linear2_reads_next_unit": ("W2", 9, (6, 2)),
    "b2_last_dropped": ("W1", 9, (2, 32)),
    "ragged_last_reads_neighbour": ("H2", 17, (16, 2)),
    "last_unit_row_zeroed": ("W4e", 9, (7, 8)),
}


@pytest.mark.parametrize("defect", [None] + sorted(HEAD_DEFECTS))
def test_one_head_defect_at_a_time_is_rejected(defect):
    if defect is None:
        for case_id in sorted({v[0] for v in HEAD_DEFECTS.values()}):
            params, boards = cases.case_data(case_id, False)
            want, bound = href.head_reference(boards[0][:9], params[0])
            assert href.judge(_defective_head(boards[0][:9], params[0], None), want, bound)[0] <= 1e-6, case_id
        return
    case_id, batch, element = HEAD_DEFECTS[defect]
    params, boards = cases.case_data(case_id, False)
    x = boards[0][:batch]
    want, bound = href.head_reference(x, params[0])
    got = _defective_head(x, params[0], defect)
    ratio = np.abs(got - want) / bound
    print(defect, case_id, "worst", href.judge(got, want, bound), "at the named element", ratio[element])
    assert ratio[element] > 1.0, (defect, case_id, element, ratio[element])
    # and the integer form of the case names it exactly: some logit is a different integer
    params, boards = cases.case_data(case_id, True)
    x = boards[0][:batch]
    want, _ = href.head_reference(x, params[0], exact=True)
    if defect not in ("relu_for_elu", "elu_without_minus_one"):        # (ELU is the identity on the integer cases)
        assert not np.array_equal(_defective_head(x, params[0], defect), want), (defect, case_id, "integers unmoved")


# ---- the down-sampler -------------------------------------------------------------------------------------------------
def _torch_downsample(models, params, mid, cout, oh, ow, dtype):
    net = models.DownsampleCNN(4, cout, (6, 6))
    net.features[0] = torch.nn.Conv2d(4, mid, kernel_size=12, stride=4, padding=2)
    net.features[3] = torch.nn.Conv2d(mid, cout, kernel_size=5, padding=2)
    net.avgpool = torch.nn.AdaptiveAvgPool2d((oh, ow))
    with torch.no_grad():
        for module, (w, b) in ((net.features[0], params[:2]), (net.features[3], params[2:])):
            module.weight.copy_(torch.from_numpy(w))
            module.bias.copy_(torch.from_numpy(b))
    return net.to(dtype).eval()


DOWN_PAIRS = [(shape, cases.DOWN_OUTPUTS[i % len(cases.DOWN_OUTPUTS)]) for i, shape in enumerate(cases.DOWN_SHAPES)] + \
             [(cases.DOWN_SHAPES[(i + 2) % len(cases.DOWN_SHAPES)], out) for i, out in enumerate(cases.DOWN_OUTPUTS)]


@pytest.mark.parametrize("pair", DOWN_PAIRS, ids=[f"mid{m}-cout{c}-{oh}x{ow}" for (m, c), (oh, ow) in DOWN_PAIRS])
def test_downsample_yardstick_is_the_module_and_its_bound_holds_in_float32(pkg, pair):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    (mid, cout), (oh, ow) = pair
    for integer in (True, False):
        params = cases.down_params(mid, cout, 10 * mid + cout, integer)
        x = cases.down_frames(3, 5 + mid, integer)
        if not integer:
            x[1, 2, 40, 41] = np.nan                                    # a NaN is kept where torch keeps it
        want, bound = dref.downsample_reference(x[:1] if integer else x, *params, oh, ow, exact=integer)
        frames = torch.from_numpy(x[:1] if integer else x)
        with torch.no_grad():
            in64 = _torch_downsample(models, params, mid, cout, oh, ow, torch.float64)(frames.double()).numpy()
            in32 = _torch_downsample(models, params, mid, cout, oh, ow, torch.float32)(frames).numpy()
        assert np.array_equal(np.isnan(in64), np.isnan(want)) and np.array_equal(np.isnan(in32), np.isnan(want))
        clean = ~np.isnan(want)
        assert np.abs(in64 - want)[clean].max() <= 1e-12 * np.abs(want[clean]).max()
        if integer:
            assert np.array_equal(in32.astype(F64), want)
        else:
            assert np.isnan(want[1]).any() and not np.isnan(want[[0, 2]]).any()
            ratio, where = href.judge(in32[[0, 2]], want[[0, 2]], bound[[0, 2]])
            assert ratio <= 1.0, (pair, ratio, where)
            assert bound[[0, 2]].max() < 0.05 * want[[0, 2]].std(), (pair, bound[[0, 2]].max())


def test_downsample_windows_are_torchs_and_exact_for_every_output_size():
    for n in range(1, 9):
        w = dref.windows(4, n)
        assert all(0 <= a < b <= 4 for a, b in w) and w[0][0] == 0 and w[-1][1] == 4
        assert {b - a for a, b in w} <= {1, 2, 4}
        pooled = torch.nn.AdaptiveAvgPool1d(n)(torch.arange(4.0).reshape(1, 1, 4)).reshape(-1).numpy()
        assert np.array_equal(pooled, [np.arange(4.0)[a:b].mean() for a, b in w])
    assert dref.windows(4, 5) == [(0, 1), (0, 2), (1, 3), (2, 4), (3, 4)] and dref.windows(4, 3) == [(0, 2), (1, 3), (2, 4)]


def _defective_downsample(x, w1, b1, w2, b2, out_h, out_w, defect):
    """A copy of downsample_reference.downsample_reference (values only) with one deliberate defect."""
    x, w1, b1, w2, b2 = (np.asarray(a, dtype=F64).copy() for a in (x, w1, b1, w2, b2))
    b, mid, cout = x.shape[0], w1.shape[0], w2.shape[0]
    if defect == "pad_left_1":
        x = np.concatenate((x[:, :, :, 1:], np.zeros_like(x[:, :, :, :1])), axis=3)      # (the frame one column to the left)
    rows, oh, ow = dref.patches(x, 12, 4, 2)
    c1 = (rows @ w1.reshape(mid, -1).T + b1).reshape(b, oh, ow, mid).transpose(0, 3, 1, 2)
    c1 = dref.relu_keep_nan(c1)
    if defect == "pool1_2x2":
        p1 = np.maximum(np.maximum(c1[:, :, 0:18:2, 0:18:2], c1[:, :, 0:18:2, 1:19:2]),
                        np.maximum(c1[:, :, 1:19:2, 0:18:2], c1[:, :, 1:19:2, 1:19:2]))
    elif defect == "max_keeps_first":
        p1 = c1[:, :, 0:18:2, 0:18:2]
    else:
        p1 = dref.max_pool_3_2(c1)
    if defect == "conv2_k_order":
        w2 = w2.transpose(0, 1, 3, 2)
    if defect == "b2_last_dropped":
        b2[-1] = 0.0
    rows, oh, ow = dref.patches(p1, 5, 1, 2)
    c2 = (rows @ w2.reshape(cout, -1).T + b2).reshape(b, oh, ow, cout).transpose(0, 3, 1, 2)
    if defect != "no_relu_2":
        c2 = dref.relu_keep_nan(c2)
    p2 = dref.max_pool_3_2(c2)
    out = np.empty((b, cout, out_h, out_w))

    def spans(n):
        if defect == "window_end_floor":
            return [((i * 4) // n, max((i * 4) // n + 1, ((i + 1) * 4) // n)) for i in range(n)]
        return dref.windows(4, n)

    for i, (y0, y1) in enumerate(spans(out_h)):
        for j, (x0, x1) in enumerate(spans(out_w)):
            total = p2[:, :, y0:y1, x0:x1].sum(axis=(2, 3))
            out[:, :, i, j] = total / (4.0 if defect == "divide_by_4" else (y1 - y0) * (x1 - x0))
    if defect == "previous_frame":
        out = np.roll(out, 1, axis=0)
    return out


# defect -> ((mid, cout), (out_h, out_w), element (frame, channel, i, j)) it must be rejected on (float frames)
DOWN_DEFECTS = {
    "pad_left_1": ((7, 12), (6, 6), (0, 3, 0, 3)),
    "pool1_2x2": ((7, 12), (6, 6), (1, 1, 5, 0)),
    "max_keeps_first": ((7, 12), (6, 6), (1, 1, 2, 0)),
    "conv2_k_order": ((5, 3), (5, 3), (1, 0, 3, 0)),
    "no_relu_2": ((4, 16), (8, 8), (1, 3, 2, 2)),
    "b2_last_dropped": ((4, 1), (1, 1), (0, 0, 0, 0)),
    "window_end_floor": ((10, 16), (3, 7), (0, 2, 0, 1)),
    "divide_by_4": ((10, 1), (5, 3), (1, 0, 0, 2)),
    "previous_frame": ((10, 16), (4, 4), (1, 13, 2, 1)),
}


@pytest.mark.parametrize("defect", [None] + sorted(DOWN_DEFECTS))
def test_one_downsample_defect_at_a_time_is_rejected(defect):
    (mid, cout), (oh, ow), element = DOWN_DEFECTS[defect or "pad_left_1"]
    params = cases.down_params(mid, cout, 10 * mid + cout, False)
    x = cases.down_frames(2, 5 + mid, False)
    want, bound = dref.downsample_reference(x, *params, oh, ow)
    got = _defective_downsample(x, *params, oh, ow, defect)
    ratio = np.abs(got - want) / bound
    if defect is None:
        assert ratio.max() <= 1e-6
        return
    print(defect, "worst", href.judge(got, want, bound), "at the named element", ratio[element])
    assert ratio[element] > 1.0, (defect, element, ratio[element])
    params = cases.down_params(mid, cout, 10 * mid + cout, True)
    x = cases.down_frames(2, 5 + mid, True)
    want, _ = dref.downsample_reference(x, *params, oh, ow, exact=True)
    assert not np.array_equal(_defective_downsample(x, *params, oh, ow, defect), want), (defect, "integers unmoved")


def test_exact_mode_refuses_what_is_not_exact():
    params, boards = cases.case_data("H2", True)
    p = dict(params[0])
    with pytest.raises(AssertionError, match="2\\^24"):
        href.head_reference(boards[0][:3], dict(p, b2=p["b2"] + np.float32(2.0 ** 24)), exact=True)
    with pytest.raises(AssertionError, match="positive"):
        href.head_reference(boards[0][:3], dict(p, b1=np.zeros_like(p["b1"])), exact=True)
    with pytest.raises(AssertionError, match="integer"):
        href.head_reference(boards[0][:3] + np.float32(0.5), p, exact=True)
    w1, b1, w2, b2 = cases.down_params(4, 1, 41, True)
    x = cases.down_frames(1, 9, True)
    with pytest.raises(AssertionError, match="2\\^24"):
        dref.downsample_reference(x * np.float32(2.0 ** 14), w1, b1, w2, b2, 1, 1, exact=True)
    with pytest.raises(AssertionError, match="integer"):
        dref.downsample_reference(x + np.float32(0.25), w1, b1, w2, b2, 1, 1, exact=True)
