"""Inputs of the training-loss kernel's tests (test_gpu_unroll_loss.py on the card, test_unroll_loss_reference.py on the
CPU): the shape matrix, the parameter cycles and the edge rows.  Everything is seeded; every row is named by a `kind`, so
a failure says what it was.  Layouts are the kernel's (include/mztrain.h): logits step-major [K1, B, .], targets [B, K1]."""
import numpy as np

from lockstep_decode_cases import value_rows
from unroll_loss_reference import two_hot32, value_transform32

# (B, K1, support, A).  support: F = 2 s + 1 on both sides of one and two 64-lane strides (63 | 65, 127 | 129) and the shipped
# 10 and 300; A: the shipped 2, 4, 7, 9, 121 and both sides of one and two strides; every listed value at least twice.
SHAPES = [
    (1, 1, 1, 1), (1, 2, 10, 2), (1, 6, 64, 121), (1, 11, 300, 9),
    (7, 1, 300, 4), (7, 2, 31, 63), (7, 6, 32, 64), (7, 11, 63, 65),
    (128, 1, 10, 129), (128, 2, 1, 128), (128, 6, 10, 121), (128, 11, 10, 7),
    (1024, 1, 31, 1), (1024, 2, 32, 2), (1024, 6, 10, 9), (1024, 11, 1, 4),
    (7, 6, 64, 128), (128, 2, 63, 129), (7, 11, 10, 65), (11, 11, 10, 63), (6, 6, 300, 64), (7, 2, 64, 7),
]
VALUE_LOSS_WEIGHTS = (0.25, 1.0, 1.5)
PER_ALPHAS = (0.5, 1.0, 0.0)
WEIGHT_MODES = ("absent", "random", "ones", "zeros_among", "tiny_among")
STAND_IN = -1e4               # finite stand-in for -inf in value / reward rows: the soft-max entry is still exactly 0 in float32


def shape_id(B, K1, s, A):
    return f"B{B}-K{K1}-s{s}-A{A}"


def parameters_for(index):
    """(value_loss_weight, per_alpha, weight mode) of the index-th shape: the three cycles have coprime lengths 3, 3 (offset
    by index // 3) and 5, so the 22 shapes meet every pair of the first two and every weight mode at least four times."""
    return (VALUE_LOSS_WEIGHTS[index % 3], PER_ALPHAS[(index + index // 3) % 3], WEIGHT_MODES[index % 5])


# ---- scalar targets ---------------------------------------------------------------------------------------------------
def _crossing(n, s):
    """The two neighbouring float32 scalars between which t = value_transform32(x) reaches the integer n: the largest x
    with t < n (frac just below 1, or clamped) and the smallest with t >= n (frac = 0 exactly), found by bisection on the
    float32 bit patterns (t is monotone in x)."""
    f = np.float32

    def key(bits):                                    # monotone map int -> float32, through the sign-magnitude patterns
        bits = np.int64(bits)
        pattern = np.uint32(bits) if bits >= 0 else np.uint32(0x80000000 + (-bits - 1) + 1)
        return np.array([pattern], dtype=np.uint32).view(f)[0]

    low, high = -0x7F000000, 0x7F000000                # finite floats
    while high - low > 1:
        mid = (low + high) // 2
        if value_transform32(key(mid)) < f(n):
            low = mid
        else:
            high = mid
    return key(low), key(high)


def scalar_targets(s, seed):
    """Float32 scalar targets and their kinds: zeros, tiny and ordinary magnitudes, values far beyond the support, and for
    integers n in -s .. s (every one up to s = 64, 41 spread ones for s = 300) the scalars on both sides of the point where
    the transformed target crosses n, where the two-hot weights are (1, 0) on one side and (~0, ~1) on the other."""
    rs = np.random.RandomState(seed)
    values, kinds = [], []

    def add(kind, x):
        values.append(np.float32(x))
        kinds.append(kind)

    add("zero", 0.0)
    add("minus_zero", -0.0)
    add("+1e-30", 1e-30)
    add("-1e-30", -1e-30)
    for i in range(6):
        add("normal_x1e-4", rs.standard_normal() * 1e-4)
        add("normal_x40", rs.standard_normal() * 40.0)
        add("normal_x(s+3)^2", rs.standard_normal() * (s + 3.0) ** 2)
    ns = list(range(-s, s + 1)) if s <= 64 else sorted(set(np.linspace(-s, s, 41).round().astype(int).tolist() + [-150, 150]))
    for n in ns:
        below, at = _crossing(n, s)
        add(f"just_below_t={n}", below)
        add(f"at_t={n}", at)
    below, at = _crossing(s, s)
    add("largest_unclamped", below)
    add("smallest_clamped", at)
    below, at = _crossing(-s, s)
    add("largest_clamped_negative", below)
    add("smallest_unclamped_negative", at)
    for x in (1e9, -1e9, 3e38, -3e38):
        add(f"{x:g}", x)
    return np.array(values, dtype=np.float32), kinds


# ---- rows -------------------------------------------------------------------------------------------------------------
def support_rows(s, n, seed):
    """[n, F] finite float32 value / reward logits and kinds: lockstep_decode_cases.value_rows for 64 lanes per row with
    the -inf entries of its log_onehot rows replaced by STAND_IN; fewer than the named rows: a seeded choice of them."""
    rows, kinds = value_rows(s, 64, max(n, 48), seed)
    rows = np.where(np.isneginf(rows), np.float32(STAND_IN), rows).astype(np.float32)
    if n < len(rows):
        pick = np.random.RandomState(seed + 1).permutation(len(rows))[:n]
        rows, kinds = rows[pick], [kinds[i] for i in pick]
    return rows, kinds


POLICY_LOGIT_KINDS = ("normal_x1", "normal_x8", "equal", "equal_3e38", "arange_1e4", "peak_last", "peak_entry_64")
POLICY_TARGET_KINDS = ("softmax", "one_hot", "zeros", "uniform", "sums_to_0.97", "sums_to_1.5", "denormal_entries")


def policy_logit_row(kind, A, rs):
    idx = np.arange(A, dtype=np.float64)
    if kind == "normal_x1":
        row = rs.standard_normal(A)
    elif kind == "normal_x8":
        row = rs.standard_normal(A) * 8.0
    elif kind == "equal":
        row = np.full(A, 0.75)
    elif kind == "equal_3e38":
        row = np.full(A, 3e38)
    elif kind == "arange_1e4":
        row = 1e4 * idx
    elif kind in ("peak_last", "peak_entry_64"):
        row = rs.standard_normal(A)
        row[A - 1 if kind == "peak_last" or A <= 64 else 64] = row.max() + 200.0
    else:
        raise KeyError(kind)
    return row.astype(np.float32)


def policy_target_row(kind, A, rs):
    if kind == "softmax":
        e = np.exp(rs.standard_normal(A))
        row = e / e.sum()
    elif kind == "one_hot":
        row = (np.arange(A) == rs.randint(A)).astype(np.float64)
    elif kind == "zeros":
        row = np.zeros(A)
    elif kind == "uniform":
        row = np.full(A, 1.0 / A)
    elif kind in ("sums_to_0.97", "sums_to_1.5"):
        e = np.exp(rs.standard_normal(A))
        row = e / e.sum() * (0.97 if kind == "sums_to_0.97" else 1.5)
    elif kind == "denormal_entries":
        e = np.exp(rs.standard_normal(A))
        row = e / e.sum()
        row[::2] = 1e-42 * (1 + np.arange(len(row[::2])))
    else:
        raise KeyError(kind)
    return row.astype(np.float32)


def _spread(named, n, rs):
    """Indices into `named` (a count) for n positions: every named row once while they fit, in seeded positions, then -1
    (the caller fills these); fewer positions than rows: a seeded choice."""
    take = rs.permutation(named)[:n]
    slots = np.full(n, -1, dtype=np.int64)
    slots[rs.permutation(n)[:len(take)]] = take
    return slots


def make_case(B, K1, s, A, index=0, nan_sample=True):
    """One launch's inputs for shape (B, K1, s, A) with the parameters of parameters_for(index), and per-position kinds.
    `nan_sample` False replaces the -inf policy entries of the NaN / +inf samples by finite logits (the twin run that shows
    the other samples do not depend on them).  Shapes with B = 1 carry no non-finite sample (their one per-sample loss
    would be all there is to check), shapes with B = 2 or A = 1 the NaN sample only."""
    seed = 1000 * index + 7 * B + 3 * K1 + s + A
    rs = np.random.RandomState(seed)
    F, N = 2 * s + 1, B * K1
    vw, alpha, mode = parameters_for(index)
    kinds = {}

    def support_head(name, row_seed):
        rows, row_kinds = support_rows(s, N, row_seed)
        order = rs.permutation(len(rows))[:N]
        kinds[name] = np.array([row_kinds[i] for i in order], dtype=object).reshape(K1, B)
        return rows[order].reshape(K1, B, F).copy()

    value = support_head("value", seed + 11)
    reward = support_head("reward", seed + 12)

    def scalar_head(name, scalar_seed):
        values, value_kinds = scalar_targets(s, scalar_seed)
        slots = _spread(len(values), N, rs)
        out = np.empty(N, dtype=np.float32)
        names = []
        for i, slot in enumerate(slots):
            if slot >= 0:
                out[i], kind = values[slot], value_kinds[slot]
            else:
                scale, kind = ((40.0, "fill_normal_x40") if i % 2 else (3.0, "fill_normal_x3"))
                out[i] = rs.standard_normal() * scale
            names.append(kind)
        kinds[name] = np.array(names, dtype=object).reshape(B, K1)
        return out.reshape(B, K1)

    target_value = scalar_head("target_value", seed + 13)
    target_reward = scalar_head("target_reward", seed + 14)

    policy = np.empty((K1, B, A), dtype=np.float32)
    target_policy = np.empty((B, K1, A), dtype=np.float32)
    kinds["policy"] = np.empty((K1, B), dtype=object)
    kinds["target_policy"] = np.empty((B, K1), dtype=object)
    pairs = [(lk, tk) for lk in POLICY_LOGIT_KINDS for tk in POLICY_TARGET_KINDS]
    slots = _spread(len(pairs), N, rs)
    for i, slot in enumerate(slots):
        k, b = divmod(i, B)
        lk, tk = pairs[slot] if slot >= 0 else (("normal_x1", "softmax") if i % 2 else ("normal_x8", "softmax"))
        policy[k, b] = policy_logit_row(lk, A, rs)
        target_policy[b, k] = policy_target_row(tk, A, rs)
        kinds["policy"][k, b], kinds["target_policy"][b, k] = lk, tk

    # the reward row of step 0 is documented as ignored: NaN in every other shape, the root's log(one_hot(centre)) else
    if index % 2 == 0:
        reward[0] = np.nan
        kinds["reward"][0, :] = "step0_nan"
    else:
        with np.errstate(divide="ignore"):
            reward[0] = np.log((np.arange(F) == s).astype(np.float32))
        kinds["reward"][0, :] = "step0_log_onehot_centre"

    # the documented domain edge: a value row with true -inf entries outside the two target entries of its target (0.0:
    # entries s and s + 1), at the last step of sample 0
    row = rs.standard_normal(F).astype(np.float32)
    row[0] = -np.inf
    if F - 1 > s + 1:
        row[F - 1] = -np.inf
    value[K1 - 1, 0] = row
    target_value[0, K1 - 1] = 0.0
    kinds["value"][K1 - 1, 0] = "neg_inf_off_target"
    kinds["target_value"][0, K1 - 1] = "zero"

    # policy heads with -inf: zero targets on -inf logits (NaN loss, sample B - 1) and a positive target on one (+inf loss,
    # sample B - 2); both must stay inside their sample
    special = {}
    if B >= 2:
        special["nan"] = B - 1
        b = B - 1
        policy[0, b] = policy_logit_row("normal_x1", A, rs)
        target = np.zeros(A, dtype=np.float32)
        target[0] = 1.0
        target_policy[b, 0] = target
        if A > 1:
            policy[0, b, 1::2] = -np.inf if nan_sample else -3.0
        else:
            policy[0, b, 0] = -np.inf if nan_sample else -3.0       # a lone -inf logit: -inf - -inf
        kinds["policy"][0, b], kinds["target_policy"][b, 0] = "neg_inf_on_zero_targets", "one_hot"
    if B >= 3 and A > 1:
        special["inf"] = B - 2
        b, k = B - 2, K1 - 1
        policy[k, b] = policy_logit_row("normal_x1", A, rs)
        policy[k, b, A - 1] = -np.inf if nan_sample else -3.0
        target_policy[b, k] = policy_target_row("uniform", A, rs)
        policy[k, b, :A - 1] = np.where(np.isneginf(policy[k, b, :A - 1]), 0.0, policy[k, b, :A - 1])
        kinds["policy"][k, b], kinds["target_policy"][b, k] = "neg_inf_under_a_target", "uniform"

    gradient_scale = rs.randint(1, max(K1, 2), size=(B, K1)).astype(np.float32)
    gradient_scale[:, 0] = rs.randint(2, 8, size=B)               # never applied: a kernel that applies it is caught
    for b in range(B):                                            # 3, 5, 7: reciprocals that round
        for k, g in ((1, 3.0), (2, 5.0), (3, 7.0)):
            if k < K1 and g <= K1 - 1 and (b + k) % 2 == 0:
                gradient_scale[b, k] = g

    if mode == "absent":
        weight = None
    elif mode == "ones":
        weight = np.ones(B, dtype=np.float32)
    else:
        weight = (rs.random_sample(B) + 0.1).astype(np.float32)
        if mode == "zeros_among":
            weight[::3] = 0.0
        elif mode == "tiny_among":
            weight[::3] = 1e-20
    return dict(B=B, K1=K1, support=s, A=A, value=value, reward=reward, policy=policy, target_value=target_value,
                target_reward=target_reward, target_policy=target_policy, gradient_scale=gradient_scale, weight=weight,
                value_loss_weight=vw, per_alpha=alpha, weight_mode=mode, kinds=kinds, special=special, id=shape_id(B, K1, s, A))


def describe(case, output, index):
    """The kinds of the rows behind element `index` of `output` (unroll_loss_reference.OUTPUTS lay-outs)."""
    kinds = case["kinds"]
    if output in ("sample_loss", "head_sums"):
        b = index[-1]
        return f"sample {b}: targets {sorted(set(kinds['target_value'][b]))[:4]}..."
    if output == "priorities":
        b, k = index
        return f"sample {b} step {k}: value {kinds['value'][k, b]}, target {kinds['target_value'][b, k]}"
    k, b = index[0], index[1]
    head = output.split("_")[1]
    target = "target_" + head
    return f"sample {b} step {k} entry {index[2]}: {head} {kinds[head][k, b]}, target {kinds[target][b, k]}"


def probe_case(s, seed=0):
    """The bit-level launch: every scalar target of scalar_targets(s) as the value target of step 0 and the reward target
    of step 1 of its own sample (B = number of scalars, K1 = 2), probe logits (0 at one entry j, -200 elsewhere: every
    other soft-max entry is exactly 0 in float32, so the gradient row is -target away from j), weight absent,
    value_loss_weight 1, gradient scale 1.  j is the entry furthest from the two target entries.  Returns (case, j [B])."""
    values, kinds = scalar_targets(s, seed)
    B, F = len(values), 2 * s + 1
    lo, _, hi, _ = two_hot32(values, s)
    j = np.where(lo >= s, 0, F - 1)                    # lo, hi >= s: entry 0 is free; lo < s: hi <= s < F - 1
    logits = np.full((2, B, F), -200.0, dtype=np.float32)
    logits[:, np.arange(B), j] = 0.0
    target = np.stack([values, values], axis=1)
    case = dict(B=B, K1=2, support=s, A=2, value=logits, reward=logits.copy(), policy=np.zeros((2, B, 2), dtype=np.float32),
                target_value=target, target_reward=target.copy(), target_policy=np.full((B, 2, 2), 0.5, dtype=np.float32),
                gradient_scale=np.ones((B, 2), dtype=np.float32), weight=None, value_loss_weight=1.0, per_alpha=0.5,
                kinds={"target_value": kinds}, special={}, id=f"probe-s{s}")
    return case, j
