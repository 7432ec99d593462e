"""The yardstick of tests/test_gpu_lockstep_decode.py, checked where no GPU is needed: the float64 reference
(parity_helpers.support_to_scalar64 / softmax64) and the derived rounding bounds (categorical_mean_rounding,
softmax_rounding_bound, value_transform_bound) against the three float32 evaluations that exist on the CPU -- this
package's torch expression (models.support_to_scalar), the C oracle's restatements (oracle support_to_scalar,
softmax_f32 over the legal logits) and the reference's own recorded outputs (fixture G1) -- on the same edge rows and
support sizes the GPU test feeds the tree kernels.  A sequential or vectorised sum of F terms is the `group = 1` case of
the bounds."""
import importlib

import numpy as np
import pytest
import torch

from lockstep_decode_cases import SHAPES, policy_cases, supports_for, value_rows
from parity_helpers import (F32_UNIT, categorical_mean, categorical_mean_rounding, inverse_value_transform64, load_golden,
                            softmax64, softmax_rounding_bound, support_to_scalar64, value_transform_bound)

SUPPORTS = sorted({s for _, _, G, _ in SHAPES for s in supports_for(G)})
GROUPS = sorted({G for _, _, G, _ in SHAPES})


def _torch_decode(logits, support):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    return models.support_to_scalar(torch.from_numpy(logits), support)[:, 0].double().numpy()


def _check_values(name, got, rows, kinds, support, group=1):
    want = support_to_scalar64(rows, support)
    bound = value_transform_bound(want, categorical_mean_rounding(rows, support, group))
    assert np.isfinite(got).all(), (name, [k for k, g in zip(kinds, got) if not np.isfinite(g)])
    ratio = np.abs(got - want) / bound
    worst = int(ratio.argmax())
    assert ratio[worst] <= 1.0, (name, support, kinds[worst], float(got[worst]), float(want[worst]), float(ratio[worst]))
    return float(ratio[worst])


@pytest.mark.parametrize("support", SUPPORTS)
def test_float64_reference_against_the_float32_restatements(oracle, support):
    # the rows depend on G only through which indices get a one-hot: take the union over the group widths
    worst = {}
    for G in GROUPS:
        rows, kinds = value_rows(support, G, 96, seed=1000 + support)
        for name, got in (("torch", _torch_decode(rows, support)),
                          ("oracle", oracle.support_to_scalar(rows, support).astype(np.float64))):
            worst[name] = max(worst.get(name, 0.0), _check_values(name, got, rows, kinds, support))
        want = support_to_scalar64(rows, support)
        for kind, row_want in zip(kinds, want):
            if kind == "log_onehot_centre" or support == 0:
                assert row_want == 0.0
            elif kind.startswith("log_onehot@"):
                # a single probability of one: the mean is the support value itself
                assert row_want == inverse_value_transform64(float(int(kind.split("@")[1]) - support))
            elif kind.startswith("equal_"):
                assert abs(row_want) <= 1e-12
    print(f"support {support}: worst error / bound {worst}")


def test_the_rounding_bound_follows_the_mass_and_the_chain_length():
    """delta_x is zero for a lone probability, a few ulps of the mean for a peaked row, and grows with the terms a chain
    adds up: not a constant that any result would pass."""
    s = 300
    rows, kinds = value_rows(s, 64, 64, seed=5)
    dx1, dx64 = categorical_mean_rounding(rows, s, 1), categorical_mean_rounding(rows, s, 64)
    for kind, a, b, row in zip(kinds, dx1, dx64, rows):
        if (softmax64(row) > 0).sum() == 1:
            assert a == 0.0 and b == 0.0                       # (the one-hots, and steps of 1e4 between neighbours)
            assert kind.startswith(("log_onehot", "arange_")), kind
        else:
            spread = (softmax64(row) * np.abs(np.arange(-s, s + 1))).sum()
            assert 0.0 < b < a                                 # 601 terms in one chain against 10 + 6 per lane
            assert b <= (2 * 16 + 5 + 800) * 1.03 * F32_UNIT * spread + 1e-30
            assert a >= 2 * 601 * F32_UNIT * spread
    # two float32 evaluations in different summation orders both stay within it
    rs = np.random.RandomState(3)
    logits = (rs.standard_normal((4096, 2 * s + 1)) * 4).astype(np.float32)
    soft = torch.softmax(torch.from_numpy(logits), dim=1)
    forward = (soft * torch.arange(-s, s + 1).float()).sum(dim=1).double().numpy()
    backward = (soft.flip(1) * torch.arange(s, -s - 1, -1).float()).sum(dim=1).double().numpy()
    exact = categorical_mean(logits, s)
    dx = categorical_mean_rounding(logits, s, 1)
    assert (np.abs(forward - exact) <= dx).all() and (np.abs(backward - exact) <= dx).all()
    assert np.abs(forward - exact).max() >= dx.min() / 2000      # within reach of what float32 really does


def test_fixture_g1_within_the_float64_bounds():
    fx = load_golden("g1_support_to_scalar")
    for key, out, support in (("logits21", "out21", 10), ("logits601", "out601", 300)):
        rows = fx[key]
        ratio = _check_values("G1 " + key, fx[out][:, 0].astype(np.float64), rows, [key] * len(rows), support)
        print(f"G1 {key}: worst error / bound {ratio:.3f}")


@pytest.mark.parametrize("A", sorted({A for A, _, _, _ in SHAPES}))
def test_float64_softmax_against_the_float32_restatements(oracle, A):
    legal, policy, kinds = policy_cases(A, 160, seed=2000 + A)
    worst = 0.0
    for actions, row, kind in zip(legal, policy, kinds):
        sel = row[actions]
        want = softmax64(sel)
        n = len(actions)
        bound = softmax_rounding_bound(sel, group=1, chunks=n)
        for name, got in (("oracle", oracle.softmax_f32(sel).astype(np.float64)),
                          ("torch", torch.softmax(torch.from_numpy(sel), dim=0).double().numpy())):
            assert (np.abs(got - want) <= bound).all(), (name, A, kind, float((np.abs(got - want) / bound).max()))
            worst = max(worst, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
            assert abs(got.sum() - 1.0) <= 1.01 * (n + 2) * F32_UNIT
        if "equal" in kind.split("/")[1] and n in (1, 2, 4, 8):
            assert np.array_equal(want, np.full(n, 1.0 / n))
        if kind.endswith("neg_inf_on_legal") and n >= 2:
            assert want[n // 2] == 0.0
    print(f"A = {A}: worst error / bound {worst:.3f}")
