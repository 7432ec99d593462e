"""The float64 yardstick of the training-loss kernel (csrc/trainer_kernels.hip unroll_loss_kernel, include/mztrain.h) and
what a float32 evaluation in the kernel's operation order may differ from it by.

* two_hot32: models.scalar_to_support for float32 scalars, one numpy float32 operation at a time in the reference's order.
  numpy's float32 +, -, *, sqrt and floor are correctly rounded, and the kernel is compiled without contraction and with a
  correctly rounded sqrtf, so this -- not torch, whose vectorised float32 sqrt is one ulp off on ~0.7 % of operands on the
  CPU -- is the BIT-LEVEL yardstick of the targets.
* unroll_loss64: every output of mztrain_loss_args in float64 from the float32 inputs; only the two-hot rows are float32
  numbers (two_hot32 widened).  It follows the kernel's documented domain: the two-hot cross-entropy reads the logits at
  the two target entries only, step 0 has no reward term.  `mutation` switches on one deliberate defect (MUTATIONS): the
  CPU tests use them to show that the case matrix and the bounds below tell a wrong kernel from a right one.
* bounds: one function per output family, from the kernel's operation order (gamma_k = k u / (1 - k u), u = 2^-24).
  expf is charged one ulp (tests/test_gpu_device_numerics.py); logf and powf are charged LOGF_ULPS / POWF_ULPS, the figures
  the same file establishes over the whole operand domain the kernel can present.  No constant is fitted to a result.
"""
import numpy as np

from parity_helpers import F32_UNIT, _gamma, _softmax_terms, support_to_scalar64, value_transform_bound

# worst distance of the device's logf on [1, 1024) / powf(a, 0.5 | 1) on [0, FLT_MAX] to float64, in float32 ulps at the
# result, rounded up to an integer (test_gpu_device_numerics.py sweeps every operand and asserts these; measured on the
# MI355X: 1.883 for logf, 1.500 and 1.0000000019 for powf with alpha = 0.5 and 1)
LOGF_ULPS = 2
POWF_ULPS = 2

TINY = 2.0 ** -126           # below this float32 leaves its normal range: errors are charged absolutely

MUTATIONS = ("total_dropped", "weights_swapped", "overflow_rule_off_by_one", "scale_at_step_0", "no_scale_at_step_1",
             "value_weight_missing_in_gradient", "per_weight_missing_in_reward_gradient", "step_0_reward_counted",
             "targets_step_major", "last_stride_skipped", "softmax_without_maximum", "two_hot_one_ulp")


# ---- the targets, bit for bit -----------------------------------------------------------------------------------------
def value_transform32(x, ulp_shift=False):
    """t = sign(x) (sqrt(|x| + 1) - 1) + 0.001 x, clamped later: float32, one rounding per operation, reference order."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    with np.errstate(over="ignore", invalid="ignore"):
        sgn = np.sign(x)
        t = sgn * (np.sqrt(np.abs(x) + f(1.0)) - f(1.0)) + f(0.001) * x
    if ulp_shift:                                    # the size of torch's vectorised-sqrt slip, where t ~ 150
        big = (np.abs(t) >= 128) & (np.abs(t) < 256)
        t = np.where(big, np.nextafter(t, f(np.inf)), t).astype(f)
    return t


def two_hot32(x, s, ulp_shift=False, swap=False, overflow_off_by_one=False):
    """(lo, w_lo, hi, w_hi) of models.scalar_to_support(x, s) for float32 scalars x (any shape): entry indices (int64) and
    float32 weights; hi = -1, w_hi = 0 where the reference's `2 s < upper` rule drops the second entry (it scatters 0.0
    into entry 0 then)."""
    f = np.float32
    t = value_transform32(x, ulp_shift)
    t = np.minimum(np.maximum(t, f(-s)), f(s))
    low = np.floor(t)
    frac = t - low
    lo = low.astype(np.int64) + s
    w_lo = f(1.0) - frac
    hi = lo + 1
    w_hi = frac
    over = hi > (2 * s - 1 if overflow_off_by_one else 2 * s)
    hi = np.where(over, -1, hi)
    w_hi = np.where(over, f(0.0), w_hi).astype(f)
    if swap:
        w_lo, w_hi = np.where(hi >= 0, w_hi, w_lo).astype(f), np.where(hi >= 0, w_lo, w_hi).astype(f)
    return lo, w_lo.astype(f), hi, w_hi


def two_hot_rows(x, s, **how):
    """two_hot32 scattered into float32 rows [..., 2 s + 1]."""
    lo, w_lo, hi, w_hi = two_hot32(x, s, **how)
    rows = np.zeros(lo.shape + (2 * s + 1,), dtype=np.float32)
    np.put_along_axis(rows, lo[..., None], w_lo[..., None], axis=-1)
    present = hi >= 0
    at = np.where(present, hi, lo)
    np.put_along_axis(rows, at[..., None], np.where(present, w_hi, w_lo)[..., None], axis=-1)
    return rows


# ---- the loss in float64 ----------------------------------------------------------------------------------------------
def _log_softmax64(x, mutation=None):
    """(log-soft-max, soft-max) of the rows of x in float64.  -inf entries give -inf / 0; a row of -inf or with a NaN
    gives NaN, as every float evaluation does."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    seen = x
    if mutation == "last_stride_skipped" and 0 < 64 * (n // 64) < n:
        seen = x[..., :64 * (n // 64)]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if mutation == "softmax_without_maximum":
            mx = np.zeros(x.shape[:-1] + (1,))
        else:
            mx = seen.max(axis=-1, keepdims=True)
        log_sum = np.log(np.exp(seen - mx).sum(axis=-1, keepdims=True))
        ls = (x - mx) - log_sum
        return ls, np.exp(ls)


def unroll_loss64(case, mutation=None):
    """Every output of mztrain_unroll_loss for `case` (unroll_loss_cases.make_case: float32 arrays value / reward [K1, B, F],
    policy [K1, B, A], target_value / target_reward / gradient_scale [B, K1], target_policy [B, K1, A], weight [B] or None,
    support, value_loss_weight, per_alpha) in float64, keyed like the struct's output members."""
    assert mutation is None or mutation in MUTATIONS, mutation
    s, vw, alpha = case["support"], float(np.float32(case["value_loss_weight"])), float(np.float32(case["per_alpha"]))
    value, reward, policy = (np.asarray(case[k], dtype=np.float64) for k in ("value", "reward", "policy"))
    K1, B, F = value.shape

    def per_step(a):                                  # [B, K1, ...] -> [K1, B, ...]
        a = np.asarray(a)
        if mutation == "targets_step_major":
            return a.reshape((K1, B) + a.shape[2:])
        return np.swapaxes(a, 0, 1)

    tv32, tr32 = per_step(case["target_value"]), per_step(case["target_reward"])
    tp = per_step(case["target_policy"]).astype(np.float64)
    gs = per_step(case["gradient_scale"]).astype(np.float64)
    w = np.ones(B) if case["weight"] is None else np.asarray(case["weight"], dtype=np.float64)
    how = dict(ulp_shift=mutation == "two_hot_one_ulp", swap=mutation == "weights_swapped",
               overflow_off_by_one=mutation == "overflow_rule_off_by_one")
    step = 1.0 / gs
    if mutation != "scale_at_step_0":
        step[0] = 1.0
    if mutation == "no_scale_at_step_1" and K1 > 1:
        step[1] = 1.0
    out = {}
    sums = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for head, logits, targets in (("value", value, tv32), ("reward", reward, tr32)):
            lo, w_lo, hi, w_hi = two_hot32(targets, s, **how)
            w_lo, w_hi = w_lo.astype(np.float64), w_hi.astype(np.float64)
            ls, soft = _log_softmax64(logits, mutation)
            rows = two_hot_rows(targets, s, **how).astype(np.float64)
            total = np.where(hi >= 0, w_lo + w_hi, w_lo)
            ls_lo = np.take_along_axis(ls, lo[..., None], axis=-1)[..., 0]
            ls_hi = np.take_along_axis(ls, np.maximum(hi, 0)[..., None], axis=-1)[..., 0]
            loss = -w_lo * ls_lo + np.where(hi >= 0, -w_hi * ls_hi, 0.0)
            scale = w[None, :] * step
            if head == "value" and mutation != "value_weight_missing_in_gradient":
                scale = w[None, :] * vw * step
            if head == "reward" and mutation == "per_weight_missing_in_reward_gradient":
                scale = step.copy()
            if mutation == "total_dropped":
                total = np.ones_like(total)
            grad = scale[..., None] * (soft * total[..., None] - rows)
            if head == "reward" and mutation != "step_0_reward_counted":
                loss[0] = 0.0
                grad[0] = 0.0
            out["grad_" + head] = grad
            sums.append(loss.sum(axis=0))
            out[head + "_losses"] = loss
        ls, soft = _log_softmax64(policy, mutation)
        total = tp.sum(axis=-1)
        if mutation == "total_dropped":
            total = np.ones_like(total)
        loss = (-tp * ls).sum(axis=-1)
        out["grad_policy"] = (w[None, :] * step)[..., None] * (soft * total[..., None] - tp)
        out["policy_losses"] = loss
        sums.append(loss.sum(axis=0))
        out["head_sums"] = np.stack(sums)
        out["sample_loss"] = ((sums[0] * vw + sums[1]) + sums[2]) * w
        predicted = support_to_scalar64(value, s)                                   # [K1, B]
        out["predicted"] = predicted
        # (the true target lay-out here even under targets_step_major: the kernel reads one array one way)
        distance = np.abs(predicted - tv32.astype(np.float64))
        out["priorities"] = np.swapaxes(np.ones_like(distance) if alpha == 0.0 else distance ** alpha, 0, 1)
    return out


OUTPUTS = ("sample_loss", "head_sums", "priorities", "grad_value", "grad_reward", "grad_policy")


# ---- what float32 may differ by ---------------------------------------------------------------------------------------
def _ulp32(a):
    """Spacing of float32 numbers at |a| (the denormal spacing below 2^-126)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    with np.errstate(over="ignore"):
        return np.spacing(np.minimum(a, 3.0e38).astype(np.float32)).astype(np.float64)


def _chain(n, group):
    """Additions a term of an n-term sum passes through: a lane's chain of ceil(n / G), then the log2(G)-step butterfly
    (group = 1: a sequential sum)."""
    return -(-n // group) + int(np.log2(group))


def log_softmax_bound(logits, group=64):
    """Per-entry bound on |ls_f32 - ls| for ls_i = (x_i - mx) - logf(sum_j expf(x_j - mx)) (row_stats, then the
    subtraction at the point of use):

        d_i = fl(x_i - mx)                       |d_i| u            (the maximum itself is exact)
        S = fl-sum of expf(d_j)                  relative gamma(c + n): the entries' own errors c u (_softmax_terms) and a
                                                 sum in which every term passes through at most n = ceil(F / G) + log2(G)
                                                 additions; entries below float32's normal range absolutely
        logf(S)                                  log(1 + theta) <= 1.01 gamma(c + n), and LOGF_ULPS ulps of the result
        d_i - logf(S)                            one rounding of the result

    A row with a single non-zero probability has S = 1 and logf(1) = 0 exactly: only the first line remains, and nothing
    at all at the maximum.  Also returns the float64 log-soft-max and soft-max."""
    p, absd, c = _softmax_terms(logits)
    x = np.asarray(logits, dtype=np.float64)
    n = _chain(x.shape[-1], group)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - x.max(axis=-1, keepdims=True)
        log_sum = np.log(np.exp(d).sum(axis=-1, keepdims=True))
        ls = d - log_sum
    lone = (p > 0).sum(axis=-1, keepdims=True) == 1
    e_d = np.where(np.isfinite(d), np.abs(d), 0.0) * F32_UNIT
    e_log = 1.01 * (_gamma(c + n) + x.shape[-1] * TINY) + LOGF_ULPS * _ulp32(log_sum)
    mag = np.where(np.isfinite(ls), np.abs(ls), 0.0)
    general = e_d + e_log + F32_UNIT * (mag + e_d + e_log)
    return np.where(lone, e_d, general), ls, p


def two_hot_ce_bound(ls, e_ls, lo, w_lo, hi, w_hi):
    """|loss_f32 - loss| for loss = fl(fl(-w_lo ls_lo) + fl(-w_hi ls_hi)) (ce_two_hot): each product carries its entry's
    log-soft-max error times the weight and one rounding, the addition one more (both terms are non-negative: no
    cancellation).  Zero when the log-soft-max entries are exact and the products are (a weight of 1 on ls = 0)."""
    a_ls = np.take_along_axis(ls, lo[..., None], axis=-1)[..., 0]
    a_e = np.take_along_axis(e_ls, lo[..., None], axis=-1)[..., 0]
    b_ls = np.take_along_axis(ls, np.maximum(hi, 0)[..., None], axis=-1)[..., 0]
    b_e = np.take_along_axis(e_ls, np.maximum(hi, 0)[..., None], axis=-1)[..., 0]

    def product(w, v, e):
        with np.errstate(invalid="ignore"):
            mag = np.where(np.isfinite(v), np.abs(w * v), 0.0)
        rounds = np.where((w == 1.0) | (w == 0.0), 0.0, F32_UNIT)       # (a product by 1 or 0 is exact)
        return mag, w * e + rounds * (mag + w * e) + np.where((mag > 0) & (mag < 2 * TINY), 2.0 ** -149, 0.0)

    mag_a, e_a = product(w_lo, a_ls, a_e)
    mag_b, e_b = product(np.where(hi >= 0, w_hi, 0.0), b_ls, b_e)
    both = (mag_a + e_a > 0) & (mag_b + e_b > 0)
    return 1.01 * (e_a + e_b + np.where(both, F32_UNIT * (mag_a + mag_b + e_a + e_b), 0.0))


def dense_ce_bound(ls, e_ls, target):
    """|loss_f32 - loss| and |total_f32 - total| for ce_dense's two sequential chains over the A entries, in index order:
    loss = sum fl(-t_i ls_i) (all terms of one sign), total = sum t_i.  A product carries t_i e_ls_i and one rounding; a
    sum of m non-zero terms passes each through at most m - 1 roundings (adding an exact zero rounds nothing)."""
    with np.errstate(invalid="ignore"):
        mag = np.where(np.isfinite(ls), np.abs(target * ls), 0.0)
    e_in = target * np.where(np.isfinite(e_ls), e_ls, 0.0)
    e_prod = e_in + F32_UNIT * (mag + e_in) + np.where((mag > 0) & (mag < 2 * TINY), 2.0 ** -149, 0.0)
    m = ((mag + e_prod) > 0).sum(axis=-1)
    e_loss = 1.01 * (e_prod.sum(axis=-1) + _gamma(np.maximum(m - 1, 0)) * (mag + e_prod).sum(axis=-1))
    m_t = (target != 0).sum(axis=-1)
    e_total = 1.01 * _gamma(np.maximum(m_t - 1, 0)) * np.abs(target).sum(axis=-1)
    return e_loss, e_total


def scale_and_roundings(weight, value_loss_weight, gradient_scale, step0):
    """The factor in front of a gradient row as the kernel forms it, fl(fl(w * vw) * fl(1 / gs)) (vw = 1 for reward and
    policy; no 1 / gs at step 0), in float64 from the float32 inputs, with a bound on its float32 evaluation's distance:
    gamma(r) |scale|, r = the operations among the three that can round at all (a factor of 1 or a power-of-two divisor
    cannot)."""
    w = np.asarray(weight, dtype=np.float64)
    vw = float(np.float32(value_loss_weight))
    gs = np.asarray(gradient_scale, dtype=np.float64)
    divides = ~step0
    mantissa = np.frexp(gs)[0]
    r = ((w != 1.0) & (vw != 1.0)).astype(np.float64)            # w * vw
    r = r + (divides & (mantissa != 0.5))                          # 1 / gs
    r = r + (divides & (gs != 1.0) & (w * vw != 1.0))              # times the step
    scale = np.where(divides, w * vw / gs, w * vw)
    return scale, _gamma(r) * np.abs(scale)


def gradient_bound(ls, e_ls, p, target, total, e_total, scale, e_scale):
    """Per-entry |g_f32 - g| for g_i = fl(scale * fl(fl(expf(ls_i) * total) - t_i)):

        expf(ls_i)            p_i (1.01 e_ls_i + 2 u): the argument's error and expf's own ulp; exact where ls_i = 0 exactly
                              (expf(0) = 1) or p_i = 0 in float64 (-inf, or below -745); absolutely below the normal range
        * total               + p_i e_total, one rounding (none when total = 1)
        - t_i                 one rounding of the difference (t_i is an input or a two_hot32 weight: exact)
        * scale               |diff| e_scale (scale_and_roundings) and one rounding (none when scale = 1)
    """
    e_ls = np.where(np.isfinite(e_ls), e_ls, 0.0)
    exact = ((ls == 0.0) & (e_ls == 0.0)) | (p == 0.0)        # (p = 0 in float64: far below where expf returns 0)
    e_soft = np.where(exact, 0.0, p * (1.01 * e_ls + 2.0 * F32_UNIT) + np.where(p < 2 * TINY, TINY, 0.0))
    total, e_total = total[..., None], e_total[..., None]
    prod = p * total
    e_prod = e_soft * total + p * e_total + np.where(total == 1.0, 0.0, F32_UNIT) * (prod + e_soft * total)
    diff = prod - target
    e_diff = e_prod + F32_UNIT * (np.abs(diff) + e_prod)
    e_diff = np.where((e_prod == 0.0) & ((prod == 0.0) | (target == 0.0)), 0.0, e_diff)     # x - 0 and 0 - t are exact
    scale, e_scale = scale[..., None], e_scale[..., None]
    g = scale * diff
    rounds = np.where((np.abs(scale) == 1.0) | (scale == 0.0), 0.0, F32_UNIT)
    e_g = np.abs(scale) * e_diff + np.abs(diff) * e_scale + rounds * (np.abs(g) + np.abs(scale) * e_diff)
    e_g = e_g + np.where((np.abs(g) + e_g > 0) & (np.abs(g) < 2 * TINY), TINY, 0.0)
    return 1.01 * e_g


def step_sum_bound(losses, e_losses):
    """|sum_f32 - sum| of a head's per-step losses [K1, ...] added in step order: the terms' own errors and at most
    K1 - 1 roundings on each (all terms are non-negative)."""
    k = losses.shape[0]
    with np.errstate(invalid="ignore"):
        mag = np.where(np.isfinite(losses), np.abs(losses), 0.0)
    e = np.where(np.isfinite(e_losses), e_losses, 0.0)
    m = ((mag + e) > 0).sum(axis=0)
    return 1.01 * (e.sum(axis=0) + _gamma(np.maximum(np.minimum(m, k) - 1, 0)) * (mag + e).sum(axis=0))


def sample_loss_bound(sums, e_sums, value_loss_weight, weight):
    """|loss_f32 - loss| for fl(fl(fl(fl(sum_v * vw) + sum_r) + sum_p) * w): the sums' errors through the factors, and one
    rounding per operation on non-negative terms -- gamma(4) of the result."""
    vw = float(np.float32(value_loss_weight))
    with np.errstate(invalid="ignore"):
        mag = np.where(np.isfinite(sums), np.abs(sums), 0.0)
    inner = vw * mag[0] + mag[1] + mag[2]
    e_inner = vw * e_sums[0] + e_sums[1] + e_sums[2]
    return 1.01 * np.abs(weight) * (e_inner + _gamma(4) * (inner + e_inner))


def decoded_value_bound(logits, support, group=64):
    """|predicted_f32 - predicted| for decode_row.  The categorical mean is NOT normalised by the sum S it has in a
    register but by inv = 1 / expf(logf(S)), so the logarithm's ABSOLUTE error comes back as a RELATIVE one on every
    probability:

        expf(fl(x_i - mx))                      |d_i| + 2
        inv = fl(1 / expf(logf(S)))             logf(S) is off by delta <= 1.01 gamma(c + n) + LOGF_ULPS ulp(log S)
                                                (log_softmax_bound); expf turns that into a relative delta, adds its own
                                                ulp (2 u), the reciprocal one rounding
        e_i * inv, (i - s) * p_i                one rounding each
        the weighted sum                        a lane's chain and the butterfly: n roundings

    delta_x = sum_i |i - s| p_i (gamma(|d_i| + 6 + n) + delta); then value_transform_bound.  For F = 601 and log S ~ 6 the
    logarithm's ulp (4.8e-7) weighs as much as eight roundings: a form that divides by S would not carry it.  A single
    non-zero probability costs nothing: S = 1, logf(1) = 0, expf(0) = 1, 1 / 1 = 1, (i - s) * 1 and + 0 are exact."""
    p, absd, c = _softmax_terms(logits)
    x = np.asarray(logits, dtype=np.float64)
    F = x.shape[-1]
    n = _chain(F, group)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = x - x.max(axis=-1, keepdims=True)
        log_sum = np.log(np.exp(d).sum(axis=-1, keepdims=True))
    delta = 1.01 * (_gamma(c + n) + F * TINY) + LOGF_ULPS * _ulp32(log_sum)
    weight = np.abs(np.arange(-support, support + 1, dtype=np.float64))
    lone = (p > 0).sum(axis=-1) == 1
    delta_x = 1.01 * (weight * p * (_gamma(absd + 6 + n) + delta)).sum(axis=-1) + weight.sum() * TINY
    delta_x = np.where(lone, 0.0, delta_x)
    predicted = support_to_scalar64(x, support)
    return value_transform_bound(predicted, delta_x), delta_x


def priority_bound(predicted, e_predicted, target, alpha):
    """|priority_f32 - priority| for powf(|fl(predicted - target)|, alpha): the distance a = |predicted - target| is off by
    e_a = e_predicted + one rounding.  alpha = 0: powf(., 0) = 1 exactly.  alpha = 1: the map is 1-Lipschitz.  0 < alpha < 1:
    |a'^alpha - a^alpha| <= |a' - a|^alpha (the power is steep at 0: no relative bound holds there), or, where a is well
    away from 0, the mean-value form alpha (a - e_a)^(alpha - 1) e_a (the derivative falls with a): the smaller of the two.
    powf itself is charged POWF_ULPS ulps of the result."""
    assert 0.0 <= alpha <= 1.0
    a = np.abs(predicted - target)
    e_a = e_predicted + F32_UNIT * (a + e_predicted)
    if alpha == 0.0:
        return np.zeros_like(a)
    if alpha == 1.0:
        moved = e_a
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            slope = np.where(a > 2.0 * e_a, alpha * np.maximum(a - e_a, TINY) ** (alpha - 1.0) * e_a, np.inf)
        moved = np.minimum(e_a ** alpha, slope)
    return moved + POWF_ULPS * _ulp32(a ** alpha + moved)


def unroll_loss_bounds(case, ref=None, group=64):
    """Bounds on |float32 evaluation - unroll_loss64(case)| for every output (OUTPUTS), per element; `group` = 64 is the
    kernel's 64-lane row sums, 1 a sequential or vectorised float32 evaluation (torch).  Entries whose yardstick is not
    finite carry no bound here: the tests hold them to the same non-finite class."""
    ref = unroll_loss64(case) if ref is None else ref
    s, vw, alpha = case["support"], case["value_loss_weight"], float(np.float32(case["per_alpha"]))
    K1, B, F = case["value"].shape
    w = np.ones(B) if case["weight"] is None else np.asarray(case["weight"], dtype=np.float64)
    gs = np.swapaxes(np.asarray(case["gradient_scale"]), 0, 1)
    step0 = np.zeros((K1, B), dtype=bool)
    step0[0] = True
    bounds, e_sums = {}, []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for head in ("value", "reward"):
            targets = np.swapaxes(np.asarray(case["target_" + head]), 0, 1)
            lo, w_lo, hi, w_hi = two_hot32(targets, s)
            w_lo, w_hi = w_lo.astype(np.float64), w_hi.astype(np.float64)
            logits = np.asarray(case[head], dtype=np.float64)
            if head == "reward":                              # step 0's row is ignored: anything may stand there
                logits = logits.copy()
                logits[0] = 0.0
            e_ls, ls, p = log_softmax_bound(logits, group)
            e_loss = two_hot_ce_bound(ls, e_ls, lo, w_lo, hi, w_hi)
            total = np.where(hi >= 0, w_lo + w_hi, w_lo)
            e_total = np.where((hi >= 0) & (w_hi != 0.0) & (w_lo != 0.0), F32_UNIT * total, 0.0)
            scale, e_scale = scale_and_roundings(w[None, :], vw if head == "value" else 1.0, gs, step0)
            rows = two_hot_rows(targets, s).astype(np.float64)
            e_grad = gradient_bound(ls, e_ls, p, rows, total, e_total, scale, e_scale)
            losses = ref[head + "_losses"]
            if head == "reward":
                e_grad[0] = 0.0
                e_loss[0] = 0.0
            bounds["grad_" + head] = e_grad
            e_sums.append(step_sum_bound(losses, e_loss))
        tp = np.swapaxes(np.asarray(case["target_policy"], dtype=np.float64), 0, 1)
        e_ls, ls, p = log_softmax_bound(case["policy"], group)
        e_loss, e_total = dense_ce_bound(ls, e_ls, tp)
        scale, e_scale = scale_and_roundings(w[None, :], 1.0, gs, step0)
        bounds["grad_policy"] = gradient_bound(ls, e_ls, p, tp, tp.sum(axis=-1), e_total, scale, e_scale)
        e_sums.append(step_sum_bound(ref["policy_losses"], e_loss))
        bounds["head_sums"] = np.stack(e_sums)
        bounds["sample_loss"] = sample_loss_bound(ref["head_sums"], bounds["head_sums"], vw, w)
        e_predicted, _ = decoded_value_bound(case["value"], s, group)
        tv = np.swapaxes(np.asarray(case["target_value"], dtype=np.float64), 0, 1)
        bounds["priorities"] = np.swapaxes(priority_bound(ref["predicted"], e_predicted, tv, alpha), 0, 1)
    return bounds


def nonfinite_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def compare(got, ref, bounds, kinds=None):
    """Per output: every element of `got` within its bound of `ref`, non-finite expectations met by the same class.
    Returns {output: (worst error / bound, index of the worst element or of the first failure, passed)}; an exact
    expectation (bound 0) met exactly counts as ratio 0, missed as inf."""
    report = {}
    for key in OUTPUTS:
        g, r, b = np.asarray(got[key], dtype=np.float64), ref[key], bounds[key]
        assert g.shape == r.shape == b.shape, (key, g.shape, r.shape, b.shape)
        cls = nonfinite_class(r)
        same_class = nonfinite_class(g) == cls
        finite = cls == 0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            err = np.where(finite & same_class, np.abs(g - r), 0.0)
            bound = np.where(finite, b, 0.0)
            bound = np.where(np.isfinite(bound), bound, np.inf)
            ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1.0))
            ratio = np.where((err > 0) & (bound == 0), np.inf, ratio)
        ratio = np.where(same_class, ratio, np.inf)
        worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
        report[key] = (float(ratio.max()) if ratio.size else 0.0, tuple(int(i) for i in worst), bool((ratio <= 1.0).all()))
    return report


# ---- the reference's torch expression ---------------------------------------------------------------------------------
def torch_reference(trainer_mod, models, value, reward, policy, b, support, vw, alpha):
    """The CPU branch of Trainer.update_weights on given logits (lists of per-step tensors that require grad)."""
    import torch
    value_targets = models.scalar_to_support(b["values"], support)
    reward_targets = models.scalar_to_support(b["rewards"], support)
    priorities = torch.zeros_like(b["values"])
    sums = {"value": 0, "reward": 0, "policy": 0}
    for k in range(len(value)):
        per_head = dict(zip(("value", "reward", "policy"), trainer_mod.Trainer.loss_function(
            value[k], reward[k], policy[k], value_targets[:, k], reward_targets[:, k], b["policies"][:, k])))
        if k == 0:
            del per_head["reward"]
        for head, term in per_head.items():
            if k > 0:
                term = trainer_mod._scale_gradient(term, b["gradient_scales"][:, k])
            sums[head] = sums[head] + term
        with torch.no_grad():
            predicted = models.support_to_scalar(value[k], support).squeeze(-1)
            priorities[:, k] = torch.abs(predicted - b["values"][:, k]) ** alpha
    loss = sums["value"] * vw + sums["reward"] + sums["policy"]
    if b["weights"] is not None:
        loss = loss * b["weights"]
    return loss, sums, priorities


def torch_outputs(trainer_mod, models, case, dtype, exact_targets=True):
    """torch_reference on `case` in `dtype` on the CPU, gradients by autograd with an upstream gradient of 1 per sample:
    a dict keyed like OUTPUTS (numpy float64).  exact_targets: the two-hot rows are two_hot_rows (float32 numbers, widened
    to `dtype`) instead of models.scalar_to_support evaluated in `dtype`, so that what follows the targets is compared on
    identical targets."""
    import types

    import torch
    if exact_targets:
        def rows(x, support):
            return torch.from_numpy(two_hot_rows(x.detach().to(torch.float32).numpy(), support)).to(dtype)
        models = types.SimpleNamespace(scalar_to_support=rows, support_to_scalar=models.support_to_scalar)
    heads = [[torch.from_numpy(np.ascontiguousarray(step)).to(dtype).requires_grad_() for step in case[name]]
             for name in ("value", "reward", "policy")]
    b = {"values": torch.from_numpy(case["target_value"]).to(dtype), "rewards": torch.from_numpy(case["target_reward"]).to(dtype),
         "policies": torch.from_numpy(case["target_policy"]).to(dtype),
         "gradient_scales": torch.from_numpy(case["gradient_scale"]).to(dtype),
         "weights": None if case["weight"] is None else torch.from_numpy(case["weight"]).to(dtype)}
    loss, sums, priorities = torch_reference(trainer_mod, models, *heads, b, case["support"], case["value_loss_weight"],
                                             case["per_alpha"])
    loss.sum().backward()
    out = {"sample_loss": loss, "priorities": priorities,
           "head_sums": torch.stack([sums[h] if torch.is_tensor(sums[h]) else torch.zeros_like(loss) for h in ("value", "reward", "policy")])}
    for name, head in zip(("value", "reward", "policy"), heads):
        out["grad_" + name] = torch.stack([t.grad if t.grad is not None else torch.zeros_like(t) for t in head])
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}
