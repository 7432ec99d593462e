"""Seeded towers and inputs for the board-conv tower tests (tests/board_tower_reference.py is the yardstick).

Integer towers (exact mode) follow one recipe: inputs in [-3, 3]; every output channel of a SPARSE layer has exactly
three nonzero weights in {-1, +1} at random (tap, input channel) slots; DENSE layers draw every weight from [-2, 2]
(asymmetric in every index with overwhelming probability); scale = 1 (a negative integer on every fifth channel where a
case asks for it); shift in [-4, 2].  Sparse sixteen-layer towers stay in the low thousands, inside the split form's range of
8188; tower_reference(exact=True) asserts it for every case it is given, so nothing here relies on that remark.

Float64-mode towers draw normal weights of variance 1 / (9 cin), scales of either sign in 0.5 .. 1.5 and small shifts.

A case is a dict: name, h, w, cin0, channels, layers [(weight, scale, shift, relu, skip, rescale)], integer (bool).

Below the cases: the launch lines the GPU tests are named after (FP32_FORMS, SPLIT_FORMS, MANY) and the launch plans of
csrc/launch_plan.h restated in numpy (tower_plan, conv_plan), so that tests/test_launch_plan_cpu.py can hold every id to
the kernel it names and the header to the restatement without a GPU.  No torch here.
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


# ---- the launch lines the GPU tests are named after (tests/test_gpu_board_towers.py) ----------------------------------------
FP32_FORMS = [
    # id (the launch line), channels, h, w, MZ_TOWER_COLS, samples per workgroup / wavefront, wider unit, cin0s
    ("launch_board_tower<4,6,7,4>", 64, 6, 7, None, 4, None, (65, 3, 64, 80)),          # 80 -> 64: 158 KB of LDS, the largest admitted
    ("launch_board_tower<4,6,6,4>", 64, 6, 6, None, 4, None, (65, 2, 64, 80)),
    ("launch_board_tower<1,6,7,4>", 16, 6, 7, None, 4, None, (17, 1, 15, 16)),
    ("launch_board_tower<1,6,6,4>", 16, 6, 6, "off", 4, None, (17, 2, 16, 20)),
    ("launch_board_tower<1,3,3,16>", 16, 3, 3, "off", 16, None, (17, 1, 3, 15, 16)),
    ("launch_board_tower<1,6,6,4>-cin0-outside-16-17", 16, 6, 6, None, 4, None, (20, 15)),   # (the patch kernel does not apply)
    ("launch_board_tower<1,3,3,16>-cin0-outside-16-17", 16, 3, 3, None, 16, None, (20, 2)),
    ("launch_board_tower_cols", 16, 3, 3, None, 16, 64, (17, 16)),                      # a wavefront: 16 boards, a workgroup: 64
    ("launch_board_tower_patch66", 16, 6, 6, None, 4, 16, (17, 16)),                    # BPW = 4 boards, a workgroup: 16
]

SPLIT_FORMS = [
    ("launch_board_tower_split<6,7,2,4>", 6, 7, 2, (65, 2, 64, 80)),
    ("launch_board_tower_split<6,6,4>", 6, 6, 4, (65, 2, 64)),
]

MANY = [
    # id, h, w, MZ_TOWER_COLS, cin0 -- the 16-channel forms across the `many` switch at 16384 boards
    ("launch_board_tower<1,6,7,6>", 6, 7, None, 17),
    ("launch_board_tower<1,6,6,3>", 6, 6, "off", 17),
    ("launch_board_tower<1,3,3,14>", 3, 3, "off", 17),
    ("launch_board_tower<1,3,3,14>-cin0-1", 3, 3, None, 1),
    ("launch_board_tower_cols-many", 3, 3, None, 17),
    ("launch_board_tower_patch66-many", 6, 6, None, 16),
]


# ---- the launch plans of csrc/launch_plan.h, restated ---------------------------------------------------------------------------
# Every argument broadcasts (numpy), every result is an int64 array of the broadcast shape.  A field the header leaves at
# zero is zero here: everything when the arguments are refused outright, the grid when the shape is refused for its size.
KERNELS = ("none", "row", "cols", "cols+heads", "patch", "split")      # TowerKernel, in the header's order
LDS_LIMIT = 160 * 1024
MAX_BATCH = 0x3fffffff
OK, INVALID = 0, -1


def supported(cin, cout, h, w):
    """mzmcts_board_conv_supported."""
    cin, cout, h, w = map(np.asarray, (cin, cout, h, w))
    board = ((h == 6) & (w == 7)) | ((h == 6) & (w == 6)) | ((h == 3) & (w == 3))
    return board & ((cout == 64) | (cout == 16)) & (cin >= 1) & (cin <= 80)


def padded_plane(h, w):
    return (h + 2) * (w + 1) + 1


def split_samples(h, w, split_boards=2):
    """Boards per workgroup of the split tower = samples per gate entry: 6 x 7 MZ_SPLIT_BOARDS (4, 2 or 1; default 2),
    3 x 3 16, 6 x 6 4."""
    h, w, split_boards = map(np.asarray, (h, w, split_boards))
    boards = np.where((split_boards == 4) | (split_boards == 1), split_boards, 2)
    return np.where((h == 6) & (w == 7), boards, np.where(h == 3, 16, 4)).astype(np.int64)


def tower_plan(batch, cin0, channels, h, w, n_layers, split=False, const_plane=False, gated=False, n_heads=0, cols_on=True,
               aligned=True, split_boards=2, layer1_skip=False):
    """board_tower_impl / board_tower_split_impl and their launchers (layer l states cin0 or channels as the descriptors
    must).  Returns dict(rc, kernel (index into KERNELS), nt, sb, waves, samples, cp0, cp1, grid, block, lds, gate_samples)."""
    args = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in
                                 (batch, cin0, channels, h, w, n_layers, split, const_plane, gated, n_heads, cols_on, aligned,
                                  split_boards, layer1_skip)])
    batch, cin0, channels, h, w, n_layers = args[:6]
    split, const_plane, gated, n_heads, cols_on, aligned, split_boards, layer1_skip = args[6:]
    split, const_plane, gated, cols_on, aligned, layer1_skip = (a != 0 for a in (split, const_plane, gated, cols_on, aligned, layer1_skip))
    b33, b66, b67 = (h == 3) & (w == 3), (h == 6) & (w == 6), (h == 6) & (w == 7)

    valid = (batch >= 0) & (batch <= MAX_BATCH) & (n_layers >= 1) & (n_layers <= 16) & supported(cin0, channels, h, w) & \
        (n_heads >= 0) & (n_heads <= 3)
    cols_applies = cols_on & (channels == 16) & (b33 | b66) & ((cin0 == 16) | (cin0 == 17))
    valid_split = (channels == 64) & (n_heads == 0) & ~(const_plane & (cin0 < 2)) & \
        ~(const_plane & (n_layers > 1) & layer1_skip & (cin0 <= channels))
    valid_fp32 = ~(gated & (channels != 64)) & ~((n_heads > 0) & ~(b33 & cols_applies))
    valid = valid & np.where(split, valid_split, valid_fp32)

    many = batch >= 16384
    gate_samples = split_samples(h, w, split_boards)
    none = (channels == 64) & b33                                   # 64 channels on 3 x 3: no tower in either form
    is_split = ~none & split
    wide = ~none & ~split & (channels == 64)
    cols = ~none & ~split & (channels == 16) & b33 & cols_applies
    patch = ~none & ~split & (channels == 16) & b66 & cols_applies & aligned
    narrow = ~none & ~split & (channels == 16) & ~cols & ~patch
    kernel = np.select([none, is_split, wide | narrow, cols & (n_heads > 0), cols, patch],
                       [0, 5, 1, 3, 2, 4])
    row = wide | narrow
    nt = np.select([wide, narrow], [4, 1], 0)
    sb = np.select([is_split, wide, narrow & b67, narrow & b66, narrow & b33],
                   [gate_samples, 4, np.where(many, 6, 4), np.where(many, 3, 4), np.where(many, 14, 16)], 0)
    waves = np.where(is_split, np.where(b67 & (sb < 4), 2 * sb, 8), 0)
    samples = np.select([none, cols, patch], [16, 64, 16], sb)
    block = np.select([is_split, row, cols | patch], [64 * waves, 512, 256], 0)

    g16 = lambda c: (c + 15) // 16 * 16 + 4                          # a buffer's channel stride: whole groups of 16, + 4
    g32 = lambda c: (c + 31) // 32 * 32 + 8                          # split: whole groups of 32, + 8
    r0 = np.where(n_layers > 2, np.maximum(g16(cin0), g16(channels)), g16(cin0))    # layers 0, 2, 4, ... read buffer 0
    r1 = np.where(n_layers > 1, np.maximum(4, g16(channels)), 4)                     # layers 1, 3, ... read buffer 1
    r0, r1 = np.maximum(r0, 16 * nt + 4), np.maximum(r1, 16 * nt + 4)                 # outputs land in either
    s0 = np.maximum(72, g32(cin0 - const_plane))
    s0 = np.where(n_layers > 2, np.maximum(s0, g32(channels)), s0)
    s1 = np.where(n_layers > 1, np.maximum(72, g32(channels)), 72)
    cp0, cp1 = np.select([row, is_split], [r0, s0], 0), np.select([row, is_split], [r1, s1], 0)
    pp = padded_plane(h, w)
    lds = np.select([row, is_split, cols, patch],
                    [4 * sb * pp * (cp0 + cp1) + 12 * sb, 2 * sb * pp * 2 * (cp0 + cp1) + 12 * sb,
                     4 * (4 * 2592 + np.where(n_heads > 0, 3 * 2320, 0)), 4 * 4 * (2 * 4 * (36 * 16 + 4) + 4 * 36 + 32)], 0)

    refused = (batch > 0) & (none | (lds > LDS_LIMIT))
    blocks = (batch + np.maximum(samples, 1) - 1) // np.maximum(samples, 1)
    grid = np.where((batch > 0) & ~refused, np.where(~split & gated, np.minimum(blocks, 256), blocks), 0)
    rc = np.where(valid & ~refused, OK, INVALID)
    out = dict(kernel=kernel, nt=nt, sb=sb, waves=waves, samples=samples, cp0=cp0, cp1=cp1, grid=grid, block=block, lds=lds,
               gate_samples=gate_samples)
    out = {k: np.where(valid, v, 0).astype(np.int64) for k, v in out.items()}
    out["rc"] = rc.astype(np.int64)
    return out


def conv_plan(batch, cin, cout, h, w):
    """mzmcts_board_conv3x3 and launch_board_conv: dict(rc, nt, sb, grid, block, lds) of board_conv3x3_kernel<nt, h, w, sb, ., .>."""
    batch, cin, cout, h, w = np.broadcast_arrays(*[np.asarray(a, dtype=np.int64) for a in (batch, cin, cout, h, w)])
    valid = (batch >= 0) & (batch <= MAX_BATCH) & supported(cin, cout, h, w)
    wide = cout == 64
    sb = np.select([(h == 6) & (w == 7), (h == 6) & (w == 6)], [np.where(wide, 4, 8), np.where(wide, 4, 16)], np.where(wide, 16, 32))
    nt = cout // 16
    planes = sb * padded_plane(h, w) * ((cin + 15) // 16 * 16 + 4)
    stage = 16 * nt * (sb * h * w + 1) + 2 * 16 * nt
    lds = 4 * np.maximum(planes, stage)
    refused = (batch > 0) & (lds > LDS_LIMIT)
    grid = np.where((batch > 0) & ~refused, (batch + sb - 1) // sb, 0)
    out = dict(nt=nt, sb=sb, grid=grid, block=np.full_like(sb, 512), lds=lds)
    out = {k: np.where(valid, v, 0).astype(np.int64) for k, v in out.items()}
    out["rc"] = np.where(valid & ~refused, OK, INVALID).astype(np.int64)
    return out
