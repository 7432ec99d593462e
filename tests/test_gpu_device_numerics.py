"""The narrow kernels' cut-down arithmetic (csrc/narrow_device.h) against the plain forms, over whole operand domains.

narrow_device.h replaces library calls by the instruction sequences their operands need and states that the results keep
the library's bits.  mzmcts_device_numerics (csrc/device_checks.hip) evaluates both forms side by side on the GPU and
reduces there; these tests walk the stated domains and hold the claims to them:

  exp_nonpositive(x)                  == expf(x)                    every float with the sign bit set, and +0.0
  reciprocal_of_sum(d)                == 1.0f / d                   every float in [1, 32]
  inverse_value_transform_narrow(x)   == inverse_value_transform(x) every float with |x| <= 16
  quotient_with(n, d, 1/d refined)    == n / d                      d = 1 .. 32768, n = +-m 2^e, e = -401 .. 401
  normalized_value / _pair, short     == (v - min) / (max - min)    float32-born bounds, ranges from one ulp to 1e3
  leaves_plain_range                  the rule written beside it, and: wherever the quotient forms differ, it fires

and two library calls of the loss kernel (csrc/trainer_kernels.hip) that have no short form, measured against float64:

  logf(x)                             every float in [1, 1024): what a soft-max normaliser can be
  powf(a, alpha)                      every non-negative finite float, alpha = 0.5 and 1: the PER priority

Each test prints the patterns it visited, the mismatches, the worst distance to float64 and its run time.
"""
import ctypes
import importlib
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(pkg):
    import torch
    assert torch.cuda.is_available()
    return importlib.import_module("muzero-hypermodel_amd._native")


def f32_pattern(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64_pattern(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_of(pattern):
    return struct.unpack("<d", struct.pack("<Q", pattern))[0]


def sweep(native, which, ranges, what):
    started = time.time()
    visited = mismatches = 0
    worst, bad = 0.0, []
    for first, count in ranges:
        m, b, w = native.device_numerics(which, first, count)
        visited += count
        mismatches += m
        bad += b
        worst = max(worst, w)
    print(f"\n{what}: {visited} patterns, {mismatches} mismatches, worst distance {worst:.6g}, "
          f"{time.time() - started:.1f} s")
    return visited, mismatches, bad, worst


def as_floats(patterns):
    return [struct.unpack("<f", struct.pack("<I", p & 0xFFFFFFFF))[0] for p in patterns]


def test_exp_nonpositive_is_expf_on_every_nonpositive_float(native):
    """+0.0 and all 2^31 patterns with the sign bit set: -0.0, negative denormals, the -103.97 cut-off's neighbourhood,
    -inf (what a masked soft-max lane produces: -inf - max); NaNs skipped.  Against float64 exp: within one float32 ulp."""
    visited, mismatches, bad, worst = sweep(native, "exp", [(0, 1), (0x80000000, 1 << 31)], "exp_nonpositive vs expf")
    assert visited == (1 << 31) + 1
    assert mismatches == 0, f"exp_nonpositive != expf at {[hex(p) for p in bad]} = {as_floats(bad)}"
    assert worst <= 1.0, worst


def test_reciprocal_of_sum_is_the_division_on_one_to_thirty_two(native):
    """Every float in [1, 32] (5 * 2^23 + 1 patterns).  A distance of at most half an ulp to the float64 quotient means the
    result is the correctly rounded one (1 / d cannot fall within 2^-49 of a float32 midpoint, so rounding the float64
    quotient again decides nothing)."""
    first, last = f32_pattern(1.0), f32_pattern(32.0)
    visited, mismatches, bad, worst = sweep(native, "reciprocal", [(first, last - first + 1)], "reciprocal_of_sum vs 1.0f / d")
    assert visited == 5 * (1 << 23) + 1
    assert mismatches == 0, f"reciprocal_of_sum != 1.0f / d at {as_floats(bad)}"
    assert worst <= 0.5 + 1e-7, worst


# |decode - float64 formula| / sqrt(|value| + 1) of the float32 evaluation (parity_helpers.value_transform_bound derives
# the lattice: w = 1 + 0.004 (|x| + 1.001) lies in [1, 2), where float32 numbers are 2^-23 apart; z = (sqrt(w) - 1) / 0.002
# then moves in steps of 6.0e-5 and the value z^2 - 1 in steps of 1.2e-4 sqrt(|value| + 1)).  The seven operations leave
# the result within two such steps.
INVERSE_TRANSFORM_BOUND = 2.4e-4


def test_inverse_value_transform_narrow_is_the_plain_decode_up_to_sixteen(native):
    """Every float with |x| <= 16 (the narrow kernel admits support <= 15), both signs, zeros and denormals included."""
    n = f32_pattern(16.0) + 1
    visited, mismatches, bad, worst = sweep(native, "inverse_transform", [(0, n), (0x80000000, n)],
                                            "inverse_value_transform_narrow vs inverse_value_transform")
    assert visited == 2 * n and visited > 2.19e9
    assert mismatches == 0, f"the short decode leaves the plain one at {as_floats(bad)}"
    assert worst <= INVERSE_TRANSFORM_BOUND, worst


def test_quotient_with_is_the_division_in_the_plain_range(native):
    """d = 1 .. 32768 (narrow_supported admits S < 32768) x both signs x exponents -401 .. 401 x mantissas all zeros, all
    ones and two seeded ones per case: 210 million quotients."""
    cases = 32768 * 2 * 803 * 4
    visited, mismatches, bad, worst = sweep(native, "quotient", [(0, cases)], "quotient_with vs n / d")
    assert mismatches == 0, f"cases {bad}: the forms are {worst} ulps apart"


def test_normalized_value_short_form_is_the_division(native):
    """2^27 seeded (min, max, v): bounds a backup would produce (r + 0.997 q from float32 r, q; a quarter start at 1.0),
    ranges of 1, 2, 4 .. 2^15 fp64 ulps and from 1e-13 to 1e3, v at, next to and between the bounds; normalized_value and
    both members of normalized_pair."""
    visited, mismatches, bad, worst = sweep(native, "normalized", [(0, 1 << 27)], "normalized_value vs the division")
    assert mismatches == 0, f"cases {bad}: the forms are {worst} ulps apart"


def test_logf_on_every_normaliser_the_loss_kernel_can_form(native):
    """logf as csrc/trainer_kernels.hip row_stats calls it, on every float in [1, 1024) (10 * 2^23 patterns): the argument
    is a sum of at most 601 terms in (0, 1] of which the largest is 1.  The domain is swept completely, so the figure is
    proven, not sampled: the worst distance to float64 log, in float32 ulps at the result, is at most
    unroll_loss_reference.LOGF_ULPS (the smallest integer that holds; the loss bounds charge exactly that), and
    logf(1) is exactly 0.  Measured on the MI355X: worst 1.883 ulps, so L = 2."""
    from unroll_loss_reference import LOGF_ULPS
    first, last = f32_pattern(1.0), f32_pattern(1024.0)
    visited, beyond_four, bad, worst = sweep(native, "log", [(first, last - first)], "logf vs float64 log on [1, 1024)")
    assert visited == 10 * (1 << 23)
    assert beyond_four == 0, f"logf more than 4 ulps from float64 at {as_floats(bad)}"
    assert worst <= LOGF_ULPS, worst


@pytest.mark.parametrize("which,alpha", [("pow_half", 0.5), ("pow_one", 1.0)])
def test_powf_on_every_nonnegative_finite_float(native, which, alpha):
    """powf(a, alpha) as the PER priority computes it (the exponent a run-time argument), alpha = 0.5 and 1 (the shipped
    values), on +0.0 and every positive finite float, denormals included (2^31 - 2^23 patterns each): the worst distance
    to float64 pow in float32 ulps is at most unroll_loss_reference.POWF_ULPS (the smallest integer that holds over both
    exponents; the priority bound charges exactly that).  Measured on the MI355X: worst 1.500 ulps for alpha = 0.5 and
    1.0000000019 for alpha = 1 (among the smallest operands powf(a, 1) is a neighbour of a, not a), so P = 2."""
    from unroll_loss_reference import POWF_ULPS
    n = f32_pattern(float("inf"))
    visited, beyond_four, bad, worst = sweep(native, which, [(0, n)], f"powf(a, {alpha}) vs float64 pow")
    assert visited == (1 << 31) - (1 << 23)
    assert beyond_four == 0, f"powf(a, {alpha}) more than 4 ulps from float64 at {as_floats(bad)}"
    assert worst <= POWF_ULPS, worst


def plain_by_the_rule(x):
    """The rule beside leaves_plain_range: a value is plain when it is zero or 2^-400 <= |x| < 2^400 (1 + 2^-20)."""
    return x == 0.0 or 2.0 ** -400 <= abs(x) < 2.0 ** 400 * (1.0 + 2.0 ** -20)


def test_leaves_plain_range_follows_its_rule(native):
    edges = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 2.0 ** -400, -(2.0 ** -400), 2.0 ** 400, -(2.0 ** 400),
             2.0 ** 400 * (1.0 + 2.0 ** -20), -(2.0 ** 400) * (1.0 + 2.0 ** -20), 2.0 ** -401, 2.0 ** 401, 1.0, -1.0,
             float("inf"), float("-inf"), 1.7976931348623157e308]
    patterns = set()
    for x in edges:
        p = f64_pattern(x)
        patterns.update(q for q in (p - 1, p, p + 1) if 0 <= q < 1 << 64)
    patterns.update([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001])   # NaNs
    rs = np.random.RandomState(5)
    for field in range(2048):                                 # a seeded double in every binade, either sign
        for _ in range(2):
            patterns.add((int(rs.randint(0, 2)) << 63) | (field << 52) | (int(rs.randint(0, 1 << 30)) << 22) | int(rs.randint(0, 1 << 22)))
    fired_wrongly, missed = [], []
    for p in sorted(patterns):
        fired, listed, _ = native.device_numerics("plain_range", p, 1)
        x = f64_of(p)
        assert fired in (0, 1) and (listed == [p] if fired else listed == [])
        want = not plain_by_the_rule(x)                      # (NaN compares false everywhere: not plain)
        if fired and not want:
            fired_wrongly.append(hex(p))
        if want and not fired:
            missed.append(hex(p))
    print(f"\nleaves_plain_range: {len(patterns)} doubles")
    assert not fired_wrongly and not missed, (fired_wrongly, missed)
    # a run of consecutive patterns across the lower edge: exactly those below 2^-400 fire
    edge = f64_pattern(2.0 ** -400)
    fired, listed, _ = native.device_numerics("plain_range", edge - 3, 6)
    assert fired == 3 and sorted(listed) == [edge - 3, edge - 2, edge - 1]


def test_wherever_the_quotient_forms_differ_the_guard_fires(native):
    """The same quotients with the numerator over every exponent field (subnormals, infinities, NaNs): outside the plain
    range the short form need not be the division, but leaves_plain_range must say so.  One operand is outside the claim
    and the sweep: a numerator of -0.0, where the short form answers +0.0 (the first run of this sweep found it: 32768
    cases, one per denominator); narrow_device.h shows beside quotient_with's claim that no caller produces it."""
    cases = 32768 * 2 * 2048 * 4
    visited, unguarded, bad, worst = sweep(native, "quotient_guarded", [(0, cases)], "quotient forms differ, guard silent")
    assert unguarded == 0, f"cases {bad}: forms {worst} ulps apart and leaves_plain_range silent"
