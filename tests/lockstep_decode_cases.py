"""Inputs of the lock-step decode tests (test_gpu_lockstep_decode.py on the card, test_lockstep_decode_reference.py on
the CPU): the shape matrix of the tree kernels' lane groups, the support sizes on both sides of the register-resident
form's limit, and the edge rows.  Everything is seeded; a row is named by its `kind` so a failure says what it was."""
import numpy as np

# (A, group_width argument of BatchedMCTS) -> (G lanes per tree, CH children per lane): every pair
# mcts_kernels.hip dispatch_group can produce, through every way mzmcts_create arrives at it.
SHAPES = [
    (1, 0, 1, 1), (2, 0, 2, 1), (2, 1, 1, 2), (2, 64, 64, 1), (3, 0, 4, 1), (4, 0, 4, 1), (5, 4, 4, 2),
    (5, 0, 8, 1), (7, 0, 8, 1), (8, 0, 8, 1), (9, 8, 8, 2), (9, 0, 16, 1), (16, 0, 16, 1), (17, 0, 32, 1),
    (33, 0, 64, 1), (64, 0, 64, 1), (9, 64, 64, 1), (65, 0, 64, 4), (121, 0, 64, 4), (129, 0, 64, 4), (256, 0, 64, 4),
]


def supports_for(G):
    """F = 2 s + 1 is odd, so the register-resident form (F <= 4 G) ends at F = 4 G - 1 and the strided one starts at
    4 G + 1: s = 2 G - 1 | 2 G.  Plus the shipped sizes (10: the board games and CartPole, 300: Atari), F = 1, and for the
    widest group a vector shorter than the group."""
    sizes = [2 * G - 1, 2 * G, 10, 300, 0]
    if G == 64:
        sizes.append(1)
    return sorted(set(sizes))


def shape_id(A, gw, G, CH, s=None):
    return f"A{A}-gw{gw}-G{G}x{CH}" + ("" if s is None else f"-s{s}")


def players_for(A):
    """The board-game action counts search as two-player games (the sign of the backed-up value changes)."""
    return 2 if A in (7, 9, 121) else 1


def value_rows(s, G, E, seed):
    """[E, F] float32 value / reward logits and their kinds.  The named rows come first, seeded normal rows at scales 1 and
    8 fill the rest."""
    F = 2 * s + 1
    rs = np.random.RandomState(seed)
    rows, kinds = [], []

    def add(kind, row):
        rows.append(np.asarray(row, dtype=np.float32))
        kinds.append(kind)

    idx = np.arange(F)
    with np.errstate(divide="ignore"):
        # what initial_inference hands over as the root reward: log of a one-hot at the centre
        add("log_onehot_centre", np.log((idx == s).astype(np.float32)))
        # a single element of probability one at the ends of the vector, of a lane's strides and of the register form
        last_of_last_lane = ((F - G) // G) * G + G - 1 if F >= G else -1
        for i in sorted({0, 1, F - 2, F - 1, G - 1, G, 4 * G - 1, 4 * G, last_of_last_lane}):
            if 0 <= i < F:
                add(f"log_onehot@{i}", np.log((idx == i).astype(np.float32)))
    add("equal_0", np.zeros(F))
    add("equal_3e38", np.full(F, 3e38))
    add("equal_-3e38", np.full(F, -3e38))
    if s > 0:
        tilt = 1e-6 / (s * (s + 1) / 3.0)        # mean = tilt * variance of the uniform distribution over [-s .. s]
        add("mean_+1e-6", tilt * (idx - s))
        add("mean_-1e-6", -tilt * (idx - s))
        add("arange_1e4", 1e4 * idx)
        add("arange_-1e4", -1e4 * idx)
        for i in sorted({0, F - 1, int(rs.randint(0, F))}):
            row = rs.standard_normal(F)
            row[i] = row.max() + 200.0
            add(f"peak200@{i}", row)
        add("ramp_0.01", 0.01 * idx)
        add("ramp_-0.01", -0.01 * idx)
        add("ramp_1", 1.0 * idx)
    while len(rows) < E:
        scale = 1.0 if len(rows) % 2 else 8.0
        add(f"normal_x{scale:g}", rs.standard_normal(F) * scale)
    assert len(rows) == E, "more named rows than envs"
    return np.stack(rows), kinds


LEGAL_KINDS = ("all_sorted", "all_shuffled", "subset_shuffled", "single", "two", "four", "eight", "seven_two_five",
               "ends_in_chunk_65", "ends_in_chunk_128", "all_but_one_shuffled", "subset_sorted")
POLICY_KINDS = ("ramp_up", "ramp_down", "normal_x1", "normal_x8", "peak_last_slot", "peak_slot_5", "neg_inf_on_legal",
                "equal", "equal_3e38", "arange_1e4")


def legal_set(kind, A, rs):
    """Legal actions of one env, in the order the caller hands them over (the root's child slots), or None if the kind
    does not exist for this action count."""
    everything = np.arange(A)
    if kind == "all_sorted":
        return everything
    if kind == "all_shuffled":
        return rs.permutation(A)
    if kind == "subset_shuffled":
        return rs.permutation(A)[:max(1, (A + 1) // 2)] if A > 1 else None
    if kind == "subset_sorted":
        return np.sort(rs.permutation(A)[:max(1, (2 * A) // 3)]) if A > 2 else None
    if kind == "single":
        return np.array([A - 1])
    if kind in ("two", "four", "eight"):
        n = {"two": 2, "four": 4, "eight": 8}[kind]
        return rs.permutation(A)[:n] if A >= n else None
    if kind == "seven_two_five":
        return np.array([7, 2, 5]) if A >= 8 else None
    if kind == "ends_in_chunk_65":
        return rs.permutation(A)[:65] if A > 65 else None
    if kind == "ends_in_chunk_128":
        return rs.permutation(A)[:128] if A > 128 else None
    if kind == "all_but_one_shuffled":
        return rs.permutation(A)[:A - 1] if A > 2 else None
    raise KeyError(kind)


def policy_row(kind, A, legal, rs):
    """[A] float32 policy logits.  Ramps give every action its own logit, so a prior paired with the wrong action is far
    outside any tolerance; the peaks sit 200 above the rest in the root's last legal slot (the last live chunk when
    A > 64) or in slot 5 (a lane of chunk 0), where a soft-max that misses them in its maximum overflows."""
    idx = np.arange(A, dtype=np.float64)
    n = len(legal)
    if kind == "ramp_up":
        row = 0.37 * idx - 3.0
    elif kind == "ramp_down":
        row = 2.0 - 0.11 * idx
    elif kind == "normal_x1":
        row = rs.standard_normal(A)
    elif kind == "normal_x8":
        row = rs.standard_normal(A) * 8.0
    elif kind in ("peak_last_slot", "peak_slot_5"):
        row = rs.standard_normal(A)
        row[legal[n - 1] if kind == "peak_last_slot" else legal[min(5, n - 1)]] = row.max() + 200.0
    elif kind == "neg_inf_on_legal":
        row = rs.standard_normal(A)
        if n >= 2:
            row[legal[n // 2]] = -np.inf
    elif kind == "equal":
        row = np.full(A, 0.75)
    elif kind == "equal_3e38":
        row = np.full(A, 3e38)
    elif kind == "arange_1e4":
        row = 1e4 * idx
    else:
        raise KeyError(kind)
    return row.astype(np.float32)


def policy_cases(A, E, seed):
    """Per env: (legal actions in slot order, policy row, "legal kind/policy kind").  The first envs walk the whole
    product of the kinds that exist for A, the rest draw from it."""
    rs = np.random.RandomState(seed)
    product = [(lk, pk) for lk in LEGAL_KINDS for pk in POLICY_KINDS if legal_set(lk, A, np.random.RandomState(0)) is not None]
    legal, policy, kinds = [], [], []
    for e in range(E):
        lk, pk = product[e] if e < len(product) else product[rs.randint(len(product))]
        actions = np.asarray(legal_set(lk, A, rs), dtype=np.int32)
        legal.append(actions)
        policy.append(policy_row(pk, A, actions, rs))
        kinds.append(f"{lk}/{pk}")
    return legal, np.stack(policy), kinds
