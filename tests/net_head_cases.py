"""Seeded cases for the conv-head and down-sampler tests (tests/net_head_reference.py and tests/downsample_reference.py are
the yardsticks), and the launchers' dispatch restated in Python, so that every case SAYS which kernel and which
compile-time form it reaches and tests/test_net_head_reference.py can hold the set to account without a GPU.

A head shape is (C, P, R, Hd, O): channels, board positions, reduced channels, hidden units, outputs.

Integer heads (exact mode): boards in [-2, 2], conv_w in [-2, 2], conv_b in [-2, 2], W1 in [-1, 1], W2 in [-2, 2], b2 in
[-3, 3] and b1[j] = 1 + sum_k |W1[j, k]| max|y_k|, which makes every hidden pre-activation positive whatever the boards
are: ELU is the identity.  The entries a defect would have to lose (last channel, last k, last bias, last hidden unit)
are forced away from zero.  head_reference(exact=True) asserts that every partial sum stays below 2^24.

Float heads: normal boards and weights of variance 1 / K per layer (logits of order 1, about half of the hidden
pre-activations negative), biases of a few tenths.

Down-sampler frames have their outermost two rows and columns 3 (integers) or 8 (floats) times the interior's range, so
the zero padding is felt; both kinds carry negative values.
"""
import numpy as np

F32 = np.float32
PERIOD = 509        # boards of a large batch repeat with this (prime) period: sample b is given board b % PERIOD
FRAME_PERIOD = 13   # the same for frames

# ---- the dispatch of mzmcts_conv_heads_multi, restated --------------------------------------------------------------
K_HEAD_WAVES = 4          # csrc/net_kernels.hip kHeadWaves
TILE = 16                 # kTileSamples
LDS_LIMIT = 160 * 1024


def mfma_head_ok(shape):
    """csrc/net_kernels.hip mfma_head_ok: reduced <= 16, channels <= 4 * kMaxConvSteps, hidden <= 64, outputs <= 32."""
    c, p, r, hd, o = shape
    return r <= 16 and c <= 64 and hd <= 64 and o <= 32


def mfma_total(shape):
    """MfmaHeadShape::total() in floats: W1 [16 nt1][RP + 1] | b1 | W2 [16 nt2][Hd + 1] | b2 | 4 waves x 16 x (ys, hs)."""
    c, p, r, hd, o = shape
    rp, nt1, nt2 = r * p, (hd + 15) // 16, (o + 15) // 16
    off_waves = 16 * nt1 * (rp + 1) + 16 * nt1 + 16 * nt2 * (hd + 1) + 16 * nt2
    return off_waves + K_HEAD_WAVES * TILE * (rp + 1 + hd + 1)


def wave_split(hd):
    """mzmcts_conv_heads_multi: lanes per hidden unit, a power of two; 1 from 33 units on."""
    split = 1
    while split * 2 * hd <= 64:
        split *= 2
    return split


def wave_total(shape):
    """HeadShape::total() in floats: the staged parameters padded to 4, then per wave [x | y | partial sums | h] padded to 4."""
    c, p, r, hd, o = shape
    per_wave = (r * c + r + hd * r * p + hd + o * hd + o + 3) & ~3
    wave_floats = (c * p + r * p + wave_split(hd) * hd + hd + 3) & ~3
    return per_wave + K_HEAD_WAVES * wave_floats


def cols_ok(shape):
    """csrc/board_conv.hip launch_board_heads_cols: 16 channels on 9 positions, reduced and hidden <= 16, outputs <= 32."""
    c, p, r, hd, o = shape
    return c == 16 and p == 9 and r <= 16 and hd <= 16 and o <= 32


def dispatch(shapes, cols_off=False):
    """The kernel a launch of these heads takes: "cols", "mfma", "wave" or "none" (MZMCTS_ERR_INVALID: no form fits the
    160 KB of a workgroup).  mzmcts_conv_heads_multi asks launch_board_heads_cols first, then takes the matrix-core
    kernel if every head passes mfma_head_ok and the largest layout fits, then the wave-per-sample kernel."""
    if not cols_off and all(cols_ok(s) for s in shapes):
        return "cols"
    if all(mfma_head_ok(s) for s in shapes) and 4 * max(mfma_total(s) for s in shapes) <= LDS_LIMIT:
        return "mfma"
    if 4 * max(wave_total(s) for s in shapes) <= LDS_LIMIT:
        return "wave"
    return "none"


def mfma_form(shape):
    """mfma_head_dispatch's instantiation <NT1, NT2, KS, G> for one head (nt1 in {2, 3} is rounded up to NT1 = 4)."""
    c, p, r, hd, o = shape
    nt1, nt2 = (hd + 15) // 16, (o + 15) // 16
    ks, g = (4, 6) if c <= 16 else (16, 2)
    return (1 if nt1 == 1 else 4, nt2, ks, g)


def samples_per_round(shapes, kernel):
    """Samples a launch covers before its persistent workgroups start a second round: grid cap 256 * per_cu workgroups of
    4 wavefronts, a wavefront taking 16 samples (mfma) or 1 (wave); per_cu = clamp(160 KB / LDS, 1, 4 or 8)."""
    if kernel == "mfma":
        lds = 4 * max(mfma_total(s) for s in shapes)
        return 256 * max(1, min(4, LDS_LIMIT // lds)) * K_HEAD_WAVES * TILE
    lds = 4 * max(wave_total(s) for s in shapes)
    return 256 * max(1, min(8, LDS_LIMIT // lds)) * K_HEAD_WAVES


MFMA_BATCHES = (1, 15, 16, 17, 63, 64, 65, 130)
WAVE_BATCHES = (1, 3, 4, 5, 9)
COLS_BATCHES = MFMA_BATCHES

# id -> dict(kernel, shapes (one per head of the launch), batches, cols_off, same_input, reaches)
HEAD_CASES = {
    "H1": dict(kernel="mfma", shapes=[(1, 1, 1, 1, 1)], batches=(1, 17), reaches="every guard at 1; steps = 1 with kParts = 4; P < G"),
    "H2": dict(kernel="mfma", shapes=[(3, 5, 2, 5, 3)], batches=MFMA_BATCHES, reaches="C, RP, Hd no multiples of 4; P < 6"),
    "H3": dict(kernel="mfma", shapes=[(16, 6, 16, 16, 16)], batches=MFMA_BATCHES, reaches="KS = 4 full, P == G, R = 16, one full tile each"),
    "H4": dict(kernel="mfma", shapes=[(17, 7, 3, 17, 17)], batches=MFMA_BATCHES, reaches="KS = 16 at 17 channels, P = G + 1, nt1 = 2 -> NT1 = 4, nt2 = 2"),
    "H5": dict(kernel="mfma", shapes=[(63, 9, 2, 33, 32)], batches=MFMA_BATCHES, reaches="63 channels, nt1 = 3 -> NT1 = 4, O full"),
    "H6": dict(kernel="mfma", shapes=[(64, 42, 2, 64, 21)], batches=MFMA_BATCHES, reaches="the Connect4 head <4, 2>"),
    "H7a": dict(kernel="mfma", shapes=[(16, 9, 16, 8, 21)], batches=(1, 17, 65), cols_off=True, reaches="the TicTacToe head on this kernel <1, 2>"),
    "H7b": dict(kernel="mfma", shapes=[(16, 36, 4, 16, 4)], batches=(1, 17, 65), reaches="the 6 x 6 head"),
    "H8": dict(kernel="mfma", shapes=[(4, 42, 6, 48, 7)], batches=(16384, 16384 + 17), reaches="per_cu = 1: a second, ragged round of the persistent loop; <4, 1, 4>"),
    "H10a": dict(kernel="mfma", shapes=[(17, 2, 1, 3, 2)], batches=(1, 17, 65), reaches="<1, 1, 16>"),
    "H10b": dict(kernel="mfma", shapes=[(20, 3, 2, 16, 17)], batches=(1, 17, 65), reaches="<1, 2, 16>"),
    "H10c": dict(kernel="mfma", shapes=[(33, 4, 3, 20, 5)], batches=(1, 17, 65), reaches="<4, 1, 16>"),
    "H10d": dict(kernel="mfma", shapes=[(8, 5, 3, 40, 20)], batches=(1, 17, 65), reaches="<4, 2, 4>"),
    "H11": dict(kernel="mfma", shapes=[(17, 7, 3, 17, 17), (17, 7, 1, 1, 1), (17, 7, 16, 64, 32)], batches=(1, 17, 65),
                reaches="three heads, wide and narrow, on different tensors: mlds is the widest's, each addresses its own layout"),
    "H12": dict(kernel="mfma", shapes=[(4, 42, 6, 48, 7), (4, 42, 1, 2, 3)], batches=(1, 65), same_input=True, reaches="two heads on one tensor"),
    "H9a": dict(kernel="cols", shapes=[(16, 9, 1, 1, 1)], batches=COLS_BATCHES, reaches="one head, every size 1"),
    "H9b": dict(kernel="cols", shapes=[(16, 9, 16, 16, 32)], batches=COLS_BATCHES, reaches="one head, every size full"),
    "H9c": dict(kernel="cols", shapes=[(16, 9, 3, 8, 21), (16, 9, 2, 16, 9)], batches=COLS_BATCHES, same_input=True, reaches="two heads on one tensor"),
    "H9d": dict(kernel="cols", shapes=[(16, 9, 5, 7, 17), (16, 9, 3, 8, 21), (16, 9, 2, 16, 9)], batches=COLS_BATCHES,
                reaches="three heads on two different tensors"),
    "W1": dict(kernel="wave", shapes=[(3, 5, 1, 1, 33)], batches=WAVE_BATCHES, reaches="scalar board load, split = 64, O > 32"),
    "W2": dict(kernel="wave", shapes=[(4, 9, 17, 5, 3)], batches=WAVE_BATCHES, reaches="R > 16, float4 load, split = 8 with Hd = 5"),
    "W3": dict(kernel="wave", shapes=[(5, 3, 1, 40, 33)], batches=WAVE_BATCHES, reaches="Hd > RP: the start column j % RP wraps"),
    "W4a": dict(kernel="wave", shapes=[(8, 4, 2, 32, 65)], batches=WAVE_BATCHES, reaches="split = 2, O past a wave, o % Hd wraps"),
    "W4b": dict(kernel="wave", shapes=[(8, 4, 2, 33, 65)], batches=WAVE_BATCHES, reaches="split = 1"),
    "W4c": dict(kernel="wave", shapes=[(8, 4, 2, 64, 65)], batches=WAVE_BATCHES, reaches="Hd = a wave"),
    "W4d": dict(kernel="wave", shapes=[(8, 4, 2, 65, 65)], batches=WAVE_BATCHES, reaches="the jj loop once"),
    "W4e": dict(kernel="wave", shapes=[(8, 4, 2, 130, 65)], batches=WAVE_BATCHES, reaches="the jj loop twice"),
    "W5": dict(kernel="wave", shapes=[(4, 25, 16, 33, 5)], batches=WAVE_BATCHES, reaches="passes mfma_head_ok, over 160 KB there: the LDS fallback"),
    "W6": dict(kernel="wave", shapes=[(3, 5, 1, 1, 33)], batches=(8192, 8192 + 5), reaches="past the grid cap at per_cu = 8"),
    "W7": dict(kernel="wave", shapes=[(4, 9, 17, 5, 3), (4, 9, 1, 70, 40), (4, 9, 2, 3, 1)], batches=(1, 5, 9),
               reaches="three heads, wide and narrow, on different tensors: lds is the widest's"),
    "R1": dict(kernel="none", shapes=[(64, 42, 16, 64, 21)], batches=(3,), reaches="both forms over 160 KB: -1, outputs untouched"),
}
for _case in HEAD_CASES.values():
    _case.setdefault("cols_off", False)
    _case.setdefault("same_input", False)

ALL_MFMA_FORMS = {(nt1, nt2, ks, g) for nt1 in (1, 4) for nt2 in (1, 2) for ks, g in ((4, 6), (16, 2))}


def head_params(shape, seed, integer):
    """One head's parameters (float32 arrays); see the module docstring."""
    c, p, r, hd, o = shape
    rs = np.random.RandomState(seed)
    if integer:
        def ints(lo, hi, size):
            return rs.randint(lo, hi + 1, size=size).astype(np.float64)

        def nonzero(a):
            return np.where(a == 0, 1.0, a)

        conv_w, conv_b = ints(-2, 2, (r, c)), ints(-2, 2, (r,))
        conv_w[:, c - 1] = nonzero(conv_w[:, c - 1])
        conv_b[r - 1] = nonzero(conv_b[r - 1])
        w1 = ints(-1, 1, (hd, r * p))
        w1[:, r * p - 1] = nonzero(w1[:, r * p - 1])
        w1[:, 0] = nonzero(w1[:, 0])
        y_max = np.repeat(2.0 * np.abs(conv_w).sum(axis=1) + np.abs(conv_b), p)          # [r * p], index r P + p
        b1 = 1.0 + np.abs(w1) @ y_max
        w2, b2 = ints(-2, 2, (o, hd)), ints(-3, 3, (o,))
        w2[:, hd - 1] = nonzero(w2[:, hd - 1])
        b2[o - 1] = nonzero(b2[o - 1])
    else:
        conv_w, conv_b = rs.standard_normal((r, c)) / np.sqrt(c), 0.3 * rs.standard_normal(r)
        w1, b1 = rs.standard_normal((hd, r * p)) / np.sqrt(r * p), 0.3 * rs.standard_normal(hd)
        w2, b2 = rs.standard_normal((o, hd)) / np.sqrt(hd), 0.3 * rs.standard_normal(o)
    return {k: np.ascontiguousarray(v, dtype=F32) for k, v in
            dict(conv_w=conv_w, conv_b=conv_b, w1=w1, b1=b1, w2=w2, b2=b2).items()}


def head_boards(shape, count, seed, integer):
    """`count` distinct boards [count, C, P] (float32)."""
    c, p = shape[:2]
    rs = np.random.RandomState(seed)
    if integer:
        x = rs.randint(-2, 3, size=(count, c, p)).astype(F32)
        x[:, c - 1, :] = np.where(x[:, c - 1, :] == 0, 1.0, x[:, c - 1, :])   # (a dropped last channel shows on every board)
        return x
    return rs.standard_normal((count, c, p)).astype(F32)


def case_seed(case_id, head=0):
    return 1000 * (sorted(HEAD_CASES).index(case_id) + 1) + 7 * head


def case_data(case_id, integer):
    """(params per head, boards per head [min(PERIOD, largest batch), C, P]) of a case.  Heads after the first read a second
    tensor (as the value / policy heads read the prediction features, the reward head the dynamics output) unless the case
    says same_input."""
    case = HEAD_CASES[case_id]
    distinct_inputs = not case["same_input"]
    count = min(PERIOD, max(case["batches"]))
    params = [head_params(s, case_seed(case_id, h) + (0 if integer else 3), integer) for h, s in enumerate(case["shapes"])]
    first = head_boards(case["shapes"][0], count, case_seed(case_id) + 1, integer)
    second = head_boards(case["shapes"][0], count, case_seed(case_id) + 2, integer)
    boards = [first if (h == 0 or not distinct_inputs) else second for h in range(len(params))]
    return params, boards


# ---- the down-sampler -------------------------------------------------------------------------------------------------
DOWN_SHAPES = ((4, 1), (4, 16), (7, 12), (10, 16), (10, 1), (5, 3))                      # (mid, cout)
DOWN_OUTPUTS = ((6, 6), (1, 1), (8, 8), (4, 4), (5, 3), (3, 7), (1, 8))                  # (out_h, out_w)
DOWN_REFUSED = (dict(mid=11), dict(mid=3), dict(cout=17), dict(oh=0), dict(oh=9), dict(ow=0), dict(ow=9))


def down_batches(cus):
    return (1, 2, 3, cus - 1, cus, cus + 1, 2 * cus, 2 * cus + 1)


def down_params(mid, cout, seed, integer):
    rs = np.random.RandomState(seed)
    if integer:
        w1, b1 = rs.randint(-1, 2, size=(mid, 4, 12, 12)), rs.randint(-3, 4, size=mid)
        w2, b2 = rs.randint(-1, 2, size=(cout, mid, 5, 5)), rs.randint(-3, 4, size=cout)
        b2[cout - 1] = b2[cout - 1] or 2
    else:
        w1, b1 = rs.standard_normal((mid, 4, 12, 12)) / 24.0, 0.2 * rs.standard_normal(mid)
        w2, b2 = rs.standard_normal((cout, mid, 5, 5)) / np.sqrt(25.0 * mid), 0.2 * rs.standard_normal(cout)
    return tuple(np.ascontiguousarray(a, dtype=F32) for a in (w1, b1, w2, b2))


def down_frames(count, seed, integer):
    """[count, 4, 84, 84] float32: the outermost two rows and columns large against the interior, both signs."""
    rs = np.random.RandomState(seed)
    edge = np.ones((84, 84))
    edge[:2, :] = edge[-2:, :] = edge[:, :2] = edge[:, -2:] = 3.0 if integer else 8.0
    if integer:
        return (rs.randint(-2, 3, size=(count, 4, 84, 84)) * edge).astype(F32)
    return (rs.standard_normal((count, 4, 84, 84)) * edge).astype(F32)
