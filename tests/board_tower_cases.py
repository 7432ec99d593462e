"""Seeded towers and inputs for the board-conv tower tests (tests/board_tower_reference.py is the yardstick).

Integer towers (exact mode) follow one recipe: inputs in [-3, 3]; every output channel of a SPARSE layer has exactly
three nonzero weights in {-1, +1} at random (tap, input channel) slots; DENSE layers draw every weight from [-2, 2]
(asymmetric in every index with overwhelming probability); scale = 1 (a negative integer on every fifth channel where a
case asks for it); shift in [-4, 2].  Sparse sixteen-layer towers stay in the low thousands, inside the split form's range of
8188; tower_reference(exact=True) asserts it for every case it is given, so nothing here relies on that remark.

Float64-mode towers draw normal weights of variance 1 / (9 cin), scales of either sign in 0.5 .. 1.5 and small shifts.

A case is a dict: name, h, w, cin0, channels, layers [(weight, scale, shift, relu, skip, rescale)], integer (bool).
"""
import numpy as np

F32 = np.float32


def sparse_weight(rs, cout, cin):
    w = np.zeros((cout, cin * 9), dtype=F32)
    for n in range(cout):
        slots = rs.choice(cin * 9, size=min(3, cin * 9), replace=False)
        w[n, slots] = rs.choice([-1.0, 1.0], size=len(slots))
    # [cout][cin][tap]: slot = channel * 9 + tap
    return w.reshape(cout, cin, 3, 3)


def dense_weight(rs, cout, cin):
    return rs.randint(-2, 3, size=(cout, cin, 3, 3)).astype(F32)


def integer_tower(name, seed, h, w, cin0, channels, n_layers, dense=(), skips="even", rescale=(), no_relu=(),
                  negative_scale=False, flat_channel=None):
    """skips: "even" = layers 2, 4, 6, ... (a dynamics tower: one convolution, then residual blocks; the skip reads what
    layer l - 2 left in the SECOND activation buffer), "odd" = layers 1, 3, 5, ... (a tower that starts with a residual
    block: layer 1 takes its skip from the tower's input, later ones from the FIRST buffer).  flat_channel: that channel of
    every rescale layer gets scale 0 -- a plane of one constant, span 0 under the rescale."""
    rs = np.random.RandomState(seed)
    layers = []
    for l in range(n_layers):
        cin = cin0 if l == 0 else channels
        weight = dense_weight(rs, channels, cin) if l in dense else sparse_weight(rs, channels, cin)
        scale = np.ones(channels, dtype=F32)
        if negative_scale:
            scale[l % 5::5] = -(1.0 + l % 2)
        shift = rs.randint(-4, 3, size=channels).astype(F32)
        if flat_channel is not None and l in rescale:
            scale[flat_channel] = 0.0
            shift[flat_channel] = 3.0
        skip = int(l >= 1 and ((skips == "even" and l % 2 == 0) or (skips == "odd" and l % 2 == 1)))
        layers.append((weight, scale, shift, int(l not in no_relu), skip, int(l in rescale)))
    return dict(name=name, h=h, w=w, cin0=cin0, channels=channels, layers=layers, integer=True)


def float_tower(name, seed, h, w, cin0, channels, n_layers, skips="even", rescale=(), tiny_span_channel=None):
    """tiny_span_channel: that channel of every rescale layer gets scale 2^-22 and shift 1 -- its plane spans a few float32
    steps next to 1.0, nonzero and far below 1e-5 (the rescale's `span + 1e-5` branch with a live numerator)."""
    rs = np.random.RandomState(seed)
    layers = []
    for l in range(n_layers):
        cin = cin0 if l == 0 else channels
        weight = (rs.standard_normal((channels, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(F32)
        scale = (rs.uniform(0.5, 1.5, channels) * rs.choice([-1.0, 1.0, 1.0, 1.0], size=channels)).astype(F32)
        shift = (0.2 * rs.standard_normal(channels)).astype(F32)
        if tiny_span_channel is not None and l in rescale:
            scale[tiny_span_channel] = F32(2.0 ** -22)
            shift[tiny_span_channel] = F32(1.0)
        skip = int(l >= 1 and ((skips == "even" and l % 2 == 0) or (skips == "odd" and l % 2 == 1)))
        layers.append((weight, scale, shift, 1, skip, int(l in rescale)))
    return dict(name=name, h=h, w=w, cin0=cin0, channels=channels, layers=layers, integer=False)


def case_input(case, batch, seed, const_plane=False):
    """The tower's input as float32 [batch, cin0, h, w]; const_plane: the last plane is one value per sample (the dynamics
    input's action plane: an integer in exact mode, action / 7 otherwise)."""
    rs = np.random.RandomState(seed)
    shape = (batch, case["cin0"], case["h"], case["w"])
    if case["integer"]:
        x = rs.randint(-3, 4, size=shape).astype(F32)
        if const_plane:
            x[:, -1] = rs.randint(-3, 4, size=(batch, 1, 1)).astype(F32)
    else:
        x = rs.standard_normal(shape).astype(F32)
        if const_plane:
            x[:, -1] = (rs.randint(0, 7, size=(batch, 1, 1)).astype(F32) / F32(7.0)).astype(F32)
    return x


EXACT_ACTIONS = 8            # gathered input in exact mode: action / 8 is exact, every value a multiple of 1 / 8
FLOAT_ACTIONS = 7


def case_gather(case, batch, seed):
    """A gathered input (include/mzmcts.h mzmcts_tower_gather): a pool of 3 slabs [3][batch][channels * h * w], a parent
    slab per sample (mixed), an action per sample, and the action count A.  Returns (pool, parent i32, action i64, A)."""
    rs = np.random.RandomState(seed)
    hidden = case["channels"] * case["h"] * case["w"]
    assert case["cin0"] == case["channels"] + 1
    if case["integer"]:
        pool = rs.randint(-3, 4, size=(3, batch, hidden)).astype(F32)
        actions = EXACT_ACTIONS
    else:
        pool = rs.standard_normal((3, batch, hidden)).astype(F32)
        actions = FLOAT_ACTIONS
    parent = rs.randint(0, 3, size=batch).astype(np.int32)
    action = rs.randint(0, actions, size=batch).astype(np.int64)
    return pool, parent, action, actions


def gathered_input(case, pool, parent, action, actions, action_shift=0):
    """The [batch, channels + 1, h, w] tensor a gathered tower reads: sample b takes pool[parent[b]][b] and a plane of
    float32(action[b]) / float32(A) (models.py:553-568).  action_shift = 1: sample b is given sample b - 1's action (a
    defect for the discrimination test)."""
    batch = len(parent)
    c, h, w = case["channels"], case["h"], case["w"]
    x = np.empty((batch, c + 1, h, w), dtype=F32)
    x[:, :c] = pool[parent.astype(np.int64), np.arange(batch)].reshape(batch, c, h, w)
    plane = (np.roll(action, action_shift).astype(F32) / F32(actions)).astype(F32)
    x[:, c] = plane.reshape(batch, 1, 1)
    return x


def standard_cases(h, w, cin0, channels, split=False):
    """The towers every form is run on, smallest first.  Dense layers only where the exact regime allows them: a dense
    layer 0 for the fp32 forms (and for the split form where the asserted range holds: one layer deep)."""
    tag = f"{h}x{w}-{cin0}to{channels}"
    seed = 1000 * h + 100 * w + cin0 + channels
    cases = [
        # one dense layer; a negative scale on every fifth channel
        integer_tower(f"one-{tag}", seed + 1, h, w, cin0, channels, 1, dense=(0,), negative_scale=True),
        # two layers, no ReLU on the first (the descriptor allows it; kept short so that the magnitudes hold)
        integer_tower(f"two-{tag}", seed + 2, h, w, cin0, channels, 2, dense=() if split else (0,), no_relu=(0,), negative_scale=True),
        # dynamics + rescale + prediction: a rescale on a MIDDLE layer (with a flat plane), then layers and a skip that
        # must see the rescaled planes; the last layer rescaled too
        integer_tower(f"dynpred5-{tag}", seed + 3, h, w, cin0, channels, 5, dense=() if split else (0,), rescale=(2, 4), flat_channel=3),
        float_tower(f"float5-{tag}", seed + 4, h, w, cin0, channels, 5, rescale=(2, 4), tiny_span_channel=5),
    ]
    if cin0 >= channels:
        # a tower that starts with a residual block: layer 1 takes its skip from the tower's input
        cases.append(integer_tower(f"root3-{tag}", seed + 5, h, w, cin0, channels, 3, skips="odd", rescale=(2,), no_relu=(2,)))
        cases.append(float_tower(f"rootfloat3-{tag}", seed + 6, h, w, cin0, channels, 3, skips="odd", rescale=(1,)))
    return cases


def deep_case(h, w, cin0, channels):
    """n_layers = 16, the descriptor's limit: sparse all the way, skips on layers 2, 4, ..., a rescale on the last."""
    return integer_tower(f"deep16-{h}x{w}-{cin0}to{channels}", 7000 + 100 * h + 10 * w + cin0, h, w, cin0, channels, 16, rescale=(15,))


def gate_case():
    """The overflow hand-over pair: a 64-channel 6 x 7 tower of 5 sparse layers on 1029 boards.  Sample 5 leaves the split
    range in its INPUT (integers near 9000); samples 1026 and 1028 only in a LATER layer (inputs near 3000, all positive:
    a channel whose three weights are +1 sums past 8190).  Returns (case, x, loose samples)."""
    case = integer_tower("gate-6x7-64to64", 4242, 6, 7, 64, 64, 5, rescale=(4,))
    batch = 1029
    x = case_input(case, batch, 99)
    rs = np.random.RandomState(5)
    x[5] = rs.randint(8990, 9011, size=x[5].shape).astype(F32)
    for s in (1026, 1028):
        x[s] = rs.randint(2990, 3011, size=x[s].shape).astype(F32)
    return case, x, (5, 1026, 1028)
