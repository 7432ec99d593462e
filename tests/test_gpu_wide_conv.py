"""include/mzmcts.h mzmcts_board_conv_wide -- relu(bn(conv3x3(x)) [+ skip]) for 11 x 11 boards with 128 output channels
(Gomoku's residual layers; csrc/wide_conv.hip), one board per workgroup on the 16-bit matrix path with every operand
carried as two fp16 halves -- against:

  * integer data, where every product and partial sum is exact whatever the summation order;
  * data that needs BOTH halves of one operand and is still exact (a lost or swapped low half shows);
  * an fp64 convolution on random data, within the bar the project holds one layer of its towers to;
  * boards outside the two-halves form's range, which the same launch computes as plain fp32 chains;
  * the modules and a captured search that reach it through models.py.
"""
import copy
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 11
COUT = 128
PAIRS = [(1, 128), (3, 129), (2, 3), (2, 1), (1, 32), (2, 33), (1, 160)]     # (batch, cin): group edges, ragged last group
CHAIN_BAR = 4e-7             # max |got - want| / sum |a b|: test_gpu_board_conv.py::test_split_tower_single_layer_against_fp64


@pytest.fixture(scope="module")
def lib(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native").load()


def _pack(lib, weight):
    cout, cin = weight.shape[:2]
    packed = torch.empty(lib.mzmcts_board_conv_wide_halfs(cin, cout), dtype=torch.float16, device="cuda")
    assert lib.mzmcts_board_conv_wide_pack(weight.data_ptr(), packed.data_ptr(), cin, cout, torch.cuda.current_stream().cuda_stream) == 0
    return packed


def _call(lib, x, weight, scale=None, shift=None, residual=None, relu=False, counter=None, packed=None):
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    assert lib.mzmcts_board_conv_wide_supported(cin, cout, h, w)
    packed = packed if packed is not None else _pack(lib, weight)
    scale = scale if scale is not None else torch.ones(cout, device="cuda")
    shift = shift if shift is not None else torch.zeros(cout, device="cuda")
    out = torch.full((b, cout, h, w), float("nan"), device="cuda")
    rc = lib.mzmcts_board_conv_wide(x.data_ptr(), packed.data_ptr(), weight.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                    residual.data_ptr() if residual is not None else None, out.data_ptr(),
                                    counter.data_ptr() if counter is not None else None, b, cin, cout, h, w, 1 if relu else 0,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _conv64(x, weight):
    return torch.nn.functional.conv2d(x.double().cpu(), weight.double().cpu(), padding=1)


@pytest.mark.parametrize("pair", PAIRS)
def test_integer_data_is_exact(lib, pair):
    """x in [-3, 3], w in [-2, 2]: the scaled operands 8 x and 64 w are integers with a zero low half, every product and
    every partial sum of the <= 1440 terms is an integer below 1440 * 24 * 128 = 4.4 M < 2^24."""
    b, cin = pair
    g = torch.Generator().manual_seed(b * 1000 + cin)
    x = torch.randint(-3, 4, (b, cin, H, W), generator=g).float().cuda()
    weight = torch.randint(-2, 3, (COUT, cin, 3, 3), generator=g).float().cuda()      # asymmetric in every index
    scale = torch.randint(1, 4, (COUT,), generator=g).float().cuda()
    shift = torch.randint(-5, 6, (COUT,), generator=g).float().cuda()
    residual = torch.randint(-4, 5, (b, COUT, H, W), generator=g).float().cuda()
    conv = _conv64(x, weight)
    packed = _pack(lib, weight)
    for res, relu in ((None, True), (residual, True), (residual, False), (None, False)):
        want = conv * scale.double().cpu().view(1, -1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1)
        if res is not None:
            want = want + res.double().cpu()
        if relu:
            want = want.clamp_min(0)
        got = _call(lib, x, weight, scale, shift, res, relu, packed=packed)
        assert np.array_equal(got.cpu().numpy(), want.float().numpy()), (pair, res is not None, relu)


@pytest.mark.parametrize("pair", PAIRS)
def test_two_half_data_is_exact(lib, pair):
    """Data whose scaled form needs both fp16 halves of ONE operand, and is still summed exactly.

    (a) x = m / 4096, |m| <= 4096, w an integer in [-2, 2]: 8 x = m / 512 has up to 13 significant bits, so
        h0 = fp16(8 x) keeps 11 of them and h1 = 8 x - h0 != 0 holds the rest, both multiples of 2^-9; 64 w is an integer
        multiple of 64 with a zero low half.
    (b) w = n / 1024, |n| <= 1024, x an integer in [-3, 3]: 64 w = n / 16 splits the same way (multiples of 2^-4), 8 x is
        a multiple of 8 with a zero low half.
    In both the dropped product (low half x low half) is exactly zero, and each of the three accumulated products is a
    multiple of 2^-9 * 64 = 2^-3 (a), 2^-4 * 8 = 2^-1 (b) in scaled units.  A term is at most 8 * 128 = 1024 (a),
    64 * 24 = 1536 (b), so every partial sum of the <= 1440 terms, in any order, stays below
        (a) 1440 * 1024 < 2^21 in steps of 2^-3: fewer than 2^24 steps,     (b) 1440 * 1536 < 2^22 in steps of 2^-1: fewer than 2^23,
    exact fp32 numbers all (the test also asserts these peaks on its own data, `scaled_peak`).  hi + lo is then exact
    and 1 / 512 is a power of two: the result must equal the fp64 convolution bit for bit.
    (c) |n| <= 1024 fits fp16's 11 significant bits, so (b) leaves the WEIGHT's low half zero.  w = n / 8192, |n| <= 8192
        with x in {-1, 0, 1} fills it: 64 w = n / 128 has up to 14 bits (multiples of 2^-7), 8 x = +-8 has a zero low half,
        products are multiples of 2^-4 of at most 64 * 8 = 512, partial sums stay below 1440 * 512 < 2^20: fewer than
        2^24 steps of 2^-4."""
    b, cin = pair
    g = torch.Generator().manual_seed(b * 77 + cin)
    for case in ("a", "b", "c"):
        if case == "a":
            x = (torch.randint(-4096, 4097, (b, cin, H, W), generator=g).float() / 4096).cuda()
            weight = torch.randint(-2, 3, (COUT, cin, 3, 3), generator=g).float().cuda()
        elif case == "b":
            x = torch.randint(-3, 4, (b, cin, H, W), generator=g).float().cuda()
            weight = (torch.randint(-1024, 1025, (COUT, cin, 3, 3), generator=g).float() / 1024).cuda()
        else:
            x = torch.randint(-1, 2, (b, cin, H, W), generator=g).float().cuda()
            weight = (torch.randint(-8192, 8193, (COUT, cin, 3, 3), generator=g).float() / 8192).cuda()
        scaled_peak = float(_conv64(x.abs() * 8, weight.abs() * 64).max())         # bounds every partial sum, any order
        assert scaled_peak < {"a": 2 ** 21, "b": 2 ** 22, "c": 2 ** 20}[case], (pair, case, scaled_peak)
        want = _conv64(x, weight)
        got = _call(lib, x, weight)
        assert np.array_equal(got.cpu().numpy(), want.float().numpy()), (pair, case)
        assert np.array_equal(want.float().double().numpy(), want.numpy())          # (the expectation is itself an fp32 number)


@pytest.mark.parametrize("pair", [(5, 128), (5, 129)])
def test_random_data_against_fp64(lib, pair):
    b, cin = pair
    g = torch.Generator().manual_seed(11 + cin)
    x = torch.randn((b, cin, H, W), generator=g).cuda()
    weight = (torch.randn((COUT, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    got = _call(lib, x, weight).double().cpu()
    magnitude = _conv64(x.abs(), weight.abs())                                      # sum |a b|
    err = float(((got - _conv64(x, weight)).abs() / magnitude).max())
    print(f"wide conv layer {cin}->{COUT}: max error / sum|a b| = {err:.2e}")
    assert err < CHAIN_BAR


def test_range_hand_over(lib):
    """Boards outside the two-halves form's range are computed by the same launch as plain fp32 fmaf chains in k order
    (tap-major, then channel), and counted.

    Where the large values sit: channel cin - 1, cell (10, 10).  An output that sees it at tap t sees only cells outside
    the board at every later tap (they lie further down or right), and it is the last channel of its tap: the large product
    is the LAST non-zero term of every chain that contains it.  The chain before it is an ordinary one on ordinary data
    (the project's bar for a k-ordered fp32 chain, 4e-7 of sum |a b|), and adding the large term rounds once, 2^-24 of a
    result that is at most sum |a b|: the same bar holds.  (Anywhere else the terms that follow a 3e7-sized partial sum
    would each round to its ulp, and no fp32 chain could hold 4e-7.)"""
    b, cin = 6, 129
    g = torch.Generator().manual_seed(4)
    x = torch.randn((b, cin, H, W), generator=g)
    below = float(np.nextafter(np.float32(8188.0), np.float32(0.0)))
    x[0, 5, 3, 3] = below
    x[1, cin - 1, 10, 10] = 8188.0
    x[4, cin - 1, 10, 10] = 3e7
    x[5, 0, 1, 1] = float("nan")
    x = x.cuda()
    weight = (torch.randn((COUT, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    packed = _pack(lib, weight)
    counter = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    got = _call(lib, x, weight, relu=True, counter=counter, packed=packed)
    assert int(counter.item()) == 7 + 3
    want = _conv64(x, weight).clamp_min(0)
    magnitude = _conv64(x.abs(), weight.abs())
    for board in (1, 4):
        assert torch.isfinite(got[board]).all()
        err = float(((got[board].double().cpu() - want[board]).abs() / magnitude[board]).max())
        print(f"board {board} (plain fp32 branch): max error / sum|a b| = {err:.2e}")
        assert err < CHAIN_BAR
    nan = torch.isnan(got[5]).cpu()
    expected = torch.zeros((COUT, H, W), dtype=torch.bool)
    expected[:, 0:3, 0:3] = True
    assert torch.equal(nan, expected) and torch.isfinite(got[5].cpu()[~expected]).all()
    alone = _call(lib, x[[0, 2, 3]].contiguous(), weight, relu=True, packed=packed)
    assert torch.equal(got[[0, 2, 3]], alone) and torch.isfinite(alone).all()
    uncounted = _call(lib, x, weight, relu=True, counter=None, packed=packed)
    assert np.array_equal(uncounted.cpu().numpy(), got.cpu().numpy(), equal_nan=True)


def test_a_board_does_not_depend_on_its_neighbours(lib):
    b, cin = 7, 33
    g = torch.Generator().manual_seed(21)
    x = torch.randn((b, cin, H, W), generator=g).cuda()
    weight = (torch.randn((COUT, cin, 3, 3), generator=g) / (9 * cin) ** 0.5).cuda()
    scale, shift = torch.rand(COUT, generator=g).cuda() + 0.5, torch.randn(COUT, generator=g).cuda()
    residual = torch.randn((b, COUT, H, W), generator=g).cuda()
    packed = _pack(lib, weight)
    whole = _call(lib, x, weight, scale, shift, residual, True, packed=packed)
    for k in range(b):
        one = _call(lib, x[k:k + 1].contiguous(), weight, scale, shift, residual[k:k + 1].contiguous(), True, packed=packed)
        assert torch.equal(whole[k:k + 1], one), k


def test_refusals(lib):
    """Outside the plan: non-zero before any launch, `out` untouched."""
    assert lib.mzmcts_board_conv_supported(128, 128, 11, 11) == 0                    # the other kernels' answer stays
    assert lib.mzmcts_board_conv_wide_supported(128, 128, 11, 11) == 1
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(4 * 161 * 11 * 12, device="cuda")                             # an input large enough for every case below
    weight = torch.zeros(128 * 161 * 9, device="cuda")
    packed = torch.zeros(lib.mzmcts_board_conv_wide_halfs(160, 128) + 4096, dtype=torch.float16, device="cuda")
    s = torch.ones(128, device="cuda")
    out = torch.full((4 * 128 * 11 * 12,), float("nan"), device="cuda")

    def call(batch=2, cin=128, cout=128, h=11, w=11, x=buf, p=packed):
        return lib.mzmcts_board_conv_wide(x.data_ptr() if x is not None else None, p.data_ptr(), weight.data_ptr(), s.data_ptr(),
                                          s.data_ptr(), None, out.data_ptr(), None, batch, cin, cout, h, w, 1, stream)

    for bad in (dict(cout=64), dict(w=12), dict(cin=161), dict(batch=-1), dict(cin=0), dict(h=6, w=7), dict(x=None),
                dict(batch=0x40000000)):
        assert call(**bad) != 0, bad
    assert lib.mzmcts_board_conv_wide_pack(weight.data_ptr(), packed.data_ptr(), 161, 128, stream) != 0
    assert lib.mzmcts_board_conv_wide_pack(weight.data_ptr(), packed.data_ptr(), 128, 64, stream) != 0
    assert call(batch=0) == 0                                                        # an empty batch: OK, nothing launched
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call() == 0                                                               # (and the good call does write)
    torch.cuda.synchronize()
    assert torch.isfinite(out[:2 * 128 * 121]).all() and torch.isnan(out[2 * 128 * 121:]).all()


def _gomoku_config(blocks, channels=128, simulations=8):
    config = importlib.import_module("muzero-hypermodel_amd.games.gomoku").MuZeroConfig()
    config.blocks, config.channels, config.num_simulations = blocks, channels, simulations
    return config


def _reference64(module):
    ref = copy.deepcopy(module).cpu().double().eval()
    if hasattr(ref, "_zero_reward_cache"):
        ref._zero_reward_cache = None
    return ref


def _judge(what, kernel, plain, want):
    """The kernel path's max error against fp64 is at most twice the torch path's (both are rounding-sized and sum in
    different orders), or inside the rtol = atol = 5e-5 the module tests of the other board kernels use."""
    kernel, plain = kernel.double().cpu(), plain.double().cpu()
    finite = torch.isfinite(want)                      # (the constant reward row of an initial inference holds -inf)
    assert torch.equal(torch.isfinite(kernel), finite) and torch.equal(kernel[~finite], want[~finite])
    e_kernel = float((kernel - want)[finite].abs().max())
    e_plain = float((plain - want)[finite].abs().max())
    print(f"{what}: max error against fp64: wide kernel {e_kernel:.3e}, torch path {e_plain:.3e}")
    floor = torch.allclose(kernel[finite], want[finite], rtol=5e-5, atol=5e-5)
    assert e_kernel <= 2 * e_plain or floor, (what, e_kernel, e_plain)


def test_modules_take_the_kernel_and_keep_fp32_accuracy(pkg, monkeypatch):
    models = importlib.import_module("muzero-hypermodel_amd.models")
    from parity_helpers import synthetic_model
    monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "on")
    g = torch.Generator().manual_seed(8)
    # ---- a residual block on its own -----------------------------------------------------------------------------------
    torch.manual_seed(3)
    block = models.ResidualBlock(128).cuda().eval()
    with torch.no_grad():
        for bn in (block.bn1, block.bn2):
            bn.running_var.uniform_(0.5, 2.0)
            bn.running_mean.normal_()
        x = torch.randn((5, 128, H, W), generator=g).cuda()
        assert block.conv1.takes_wide_path(x) and not block.conv1.takes_mfma_path(x)
        kernel = block(x)
        assert block.conv1.__dict__.get("_packed_wide") is not None and block.conv2.__dict__.get("_packed_wide") is not None
        monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "off")
        assert not block.conv1.takes_wide_path(x)
        fresh = copy.deepcopy(block)
        for conv in (fresh.conv1, fresh.conv2):
            conv.__dict__.pop("_packed_wide", None)
        plain = fresh(x)
        assert fresh.conv1.__dict__.get("_packed_wide") is None
        _judge("residual block", kernel, plain, _reference64(block)(x.double().cpu()))
        monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "on")
    # training mode and autograd keep torch's convolution
    assert not block.conv1.takes_wide_path(x)                                       # (grad mode is on outside no_grad)
    block.train()
    with torch.no_grad():
        assert not block.conv1.takes_wide_path(x)
    block.eval()
    assert block.conv1(x[:2].requires_grad_(True)).requires_grad

    # ---- a Gomoku network ------------------------------------------------------------------------------------------------
    config = _gomoku_config(blocks=2)
    model, _ = synthetic_model(models, config, "cuda")
    obs = torch.randint(0, 2, (5, 3, H, W), generator=g).float().cuda()
    action = torch.randint(0, 121, (5, 1), generator=g).cuda()
    convs = [m for m in model.modules() if isinstance(m, models.BoardConv2d)]
    assert len(convs) == 1 + 4 + 1 + 4 + 4
    ref = _reference64(model)
    with torch.no_grad():
        want_root = ref.initial_inference(obs.double().cpu())
        monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "off")
        plain_root = model.initial_inference(obs)
        plain_next = model.recurrent_inference(want_root[3].float().cuda(), action)
        assert all(conv.__dict__.get("_packed_wide") is None for conv in convs)
        monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "on")
        kernel_root = model.initial_inference(obs)
        kernel_next = model.recurrent_inference(want_root[3].float().cuda(), action)
        assert all(conv.__dict__.get("_packed_wide") is not None for conv in convs)
        assert model.wide_conv_exact_boards() == 0
        # the recurrent reference starts from the same fp32 state the two GPU paths were given
        want_next = ref.recurrent_inference(want_root[3].float().double(), action.cpu())
    names = ("value", "reward", "policy logits", "hidden state")
    for name, k, p, w in zip(names, kernel_root, plain_root, want_root):
        _judge("initial " + name, k, p, w.double())
    for name, k, p, w in zip(names, kernel_next, plain_next, want_next):
        _judge("recurrent " + name, k, p, w.double())


def test_graph_replay_follows_a_weight_refresh(pkg, monkeypatch):
    """The shape of test_gpu_net.py::test_resnet_graph_replay_follows_a_weight_refresh on a 128-channel Gomoku network: the
    captured simulation loop equals the eager one bit for bit, and after new weights land in the flat buffer the replayed
    graph searches with them -- the packed halves are refilled in place, at the address the graph reads."""
    from parity_helpers import synthetic_model
    eng = importlib.import_module("muzero-hypermodel_amd.engine")
    models = importlib.import_module("muzero-hypermodel_amd.models")
    weights_mod = importlib.import_module("muzero-hypermodel_amd.weights")
    monkeypatch.setenv("MZ_BOARD_CONV_WIDE", "on")
    config = _gomoku_config(blocks=1)
    E = 3
    rs = np.random.RandomState(5)
    boards = np.zeros((E, 3, H, W), dtype=np.float32)
    stones = rs.randint(0, 3, (E, H, W))
    boards[:, 0], boards[:, 1], boards[:, 2] = stones == 1, stones == 2, 1.0
    legal = [np.flatnonzero(stones[e].ravel() == 0).tolist() for e in range(E)]
    to_play = [0] * E
    model, _ = synthetic_model(models, config, "cuda", seed=0)
    _, new_weights = synthetic_model(models, config, "cpu", seed=1)
    flat = weights_mod.FlatWeights(model)

    def visits_and_values(engine, net):
        st = engine.search(net, boards, legal, to_play, True)
        return st["visits"].copy(), st["root_value_sum"].copy()

    graphed = eng.BatchedMCTS(config, E, use_graph=True)
    before = visits_and_values(graphed, model)
    conv = model.prediction_network.module.resblocks[0].conv1
    assert conv.__dict__.get("_packed_wide") is not None                           # the search ran the kernel
    packed_ptr = conv.packed_wide().data_ptr()
    replayed = visits_and_values(graphed, model)                                     # a replay of the captured graph
    assert graphed._graph is not None
    old_model, _ = synthetic_model(models, config, "cuda", seed=0)
    eager = eng.BatchedMCTS(config, E, use_graph=False)
    visits_and_values(eager, old_model)
    same = visits_and_values(eager, old_model)
    eager.close()
    assert np.array_equal(replayed[0], same[0]) and np.array_equal(replayed[1], same[1])
    flat.load_state_dict(new_weights)                                                # in place + refresh_inference_constants()
    after = visits_and_values(graphed, model)
    graphed.close()
    assert conv.packed_wide().data_ptr() == packed_ptr
    fresh_model, _ = synthetic_model(models, config, "cuda", seed=1)
    eager = eng.BatchedMCTS(config, E, use_graph=False)
    visits_and_values(eager, fresh_model)                                            # same RNG stream positions as the graphed engine
    visits_and_values(eager, fresh_model)
    want = visits_and_values(eager, fresh_model)
    eager.close()
    assert not np.array_equal(before[1], after[1])
    assert np.array_equal(after[0], want[0]) and np.array_equal(after[1], want[1])
    assert model.wide_conv_exact_boards() == 0
