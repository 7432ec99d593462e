"""Inputs of the native replay tests (test_gpu_native_replay.py on the card, test_native_replay_cases_cpu.py on the CPU):
whole searches of T = 19 trees x S = 32 simulations for every lane-group shape of lockstep_decode_cases.SHAPES, driven by
seeded logits.  Everything is seeded; no torch, no HIP."""
import numpy as np

from lockstep_decode_cases import SHAPES, players_for, shape_id

T, S = 19, 32
DISCOUNT = 0.997
TEMPERATURES = (1.0, 0.5, 0.25, 0.0)
VALUE_SCALE, POLICY_SCALE = 3.0, 1.5
# the ways a native search is driven: select + expand_backup | expand_backup_select | the former with a wavefront-local
# queue of 40 / 256 trees in select (trees tiled 3x: 57 envs, a refill and a ragged last wavefront at 40)
FORMS = ("steps", "fused", "queue40", "queue256")
QUEUE = {"queue40": 40, "queue256": 256}
REPEAT = {"steps": 1, "fused": 1, "queue40": 3, "queue256": 3}

# (A, gw, support) -> seed, where the default A * 1000 + gw * 10 + support does not reach what
# test_native_replay_cases_cpu.py asks of a case (depth, tie-break words, both players)
SEEDS = {(64, 0, 10): 364019, (64, 0, 128): 264134, (121, 0, 10): 421019, (121, 0, 128): 421137,
         (256, 0, 10): 1156037, (256, 0, 128): 456134}


def storm(t):
    """Every third tree is a tie storm: flat priors (policy logits all zero), values and rewards that decode to exactly 0
    (the one-hot-centre row), so its normaliser bounds never separate and every unvisited level is a tie.  (An all-zero
    value row would not do: its mean is 0 only up to the rounding of the sum, the inverse transform's float32 evaluation
    at 0 is sign(x) * 2.59e-5 -- measured on the MI355X at G = 1, F = 21: -2.587e-5 -- and float64's sign(x) * 1.8e-15.)"""
    return t % 3 == 0


def cases():
    """(A, gw, G, CH, support, form): every shape at support 10 in every form (the queue needs A <= 64), and in `steps`
    at support 2 G as well: F = 4 G + 1, the first size of the decode's strided form."""
    out = []
    for A, gw, G, CH in SHAPES:
        for form in FORMS:
            if form in QUEUE and A > 64:
                continue
            out.append((A, gw, G, CH, 10, form))
        out.append((A, gw, G, CH, 2 * G, "steps"))
    return out


def case_id(A, gw, G, CH, s, form):
    return shape_id(A, gw, G, CH, s) + "-" + form


def log_onehot_centre(s):
    """What initial_inference hands over as the root's reward logits: it decodes to exactly 0."""
    with np.errstate(divide="ignore"):
        return np.log((np.arange(2 * s + 1) == s).astype(np.float32))


def inputs(A, gw, s):
    """The inputs of one case: engine seeds, root legal sets (random subsets, as parity_helpers.random_streams draws
    them), to_play cycling over the players, temperatures cycling over 1, 0.5, 0.25, 0, value / reward logits [T, S, F]
    (normal, scale 3), policy logits [T, S, A] and the root's [T, A] (normal, scale 1.5); a storm tree's: see storm()."""
    rs = np.random.RandomState(SEEDS.get((A, gw, s), A * 1000 + gw * 10 + s))
    F = 2 * s + 1
    players = players_for(A)
    legal = []
    for _ in range(T):
        n = int(rs.randint(1, A + 1))
        legal.append(sorted(rs.choice(A, size=n, replace=False).tolist()))
    case = dict(
        A=A, gw=gw, support=s, players=players,
        seeds=[int(x) for x in rs.randint(0, 2**31 - 1, size=T)],
        legal=legal,
        to_play=[t % players for t in range(T)],
        temperature=[TEMPERATURES[t % 4] for t in range(T)],
        storm=np.array([storm(t) for t in range(T)]),
        value_logits=(rs.standard_normal((T, S, F)) * VALUE_SCALE).astype(np.float32),
        reward_logits=(rs.standard_normal((T, S, F)) * VALUE_SCALE).astype(np.float32),
        policy_logits=(rs.standard_normal((T, S, A)) * POLICY_SCALE).astype(np.float32),
        root_value_logits=(rs.standard_normal((T, F)) * VALUE_SCALE).astype(np.float32),
        root_policy_logits=(rs.standard_normal((T, A)) * POLICY_SCALE).astype(np.float32),
        root_reward_logits=np.tile(log_onehot_centre(s), (T, 1)),
    )
    for key in ("value_logits", "reward_logits", "root_value_logits"):
        case[key][case["storm"]] = log_onehot_centre(s)
    for key in ("policy_logits", "root_policy_logits"):
        case[key][case["storm"]] = 0.0
    return case
