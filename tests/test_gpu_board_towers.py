"""The five tower kernels of csrc/board_conv.hip, driven through the C entry points directly (ctypes: mzmcts_board_tower,
_split, _gathered, _heads; no network module in between) and compared with a yardstick that owes nothing to them
(tests/board_tower_reference.py; tests/test_board_tower_reference.py holds it to account on the CPU):

  exact      integer towers (tests/board_tower_cases.py): every product and partial sum is exact in fp32 in any order, and
             in the split form too (integers x 8 below 65504 split exactly into two fp16 halves, weights in {-2..2} x 64
             have a zero low half, the dropped a1 b1 term is zero, the constant plane's table is an fp32 sum of integers):
             EVERY form must return the integers, bit for bit -- up to and including the first rescale layer;
  float64    every layer exports, and layer l is judged on the launch's OWN exported input within
             parity_helpers.tower_layer_rounding_bound, so a 16-layer tower is held as tightly as one layer;
  rescale    unit exports are bit for bit the numpy float32 expression on the launch's own raw export.  The split form
             rescales the float32 values h0 + h1 with the same two operations and writes the quotient back as two fp16
             halves before it exports it: its unit export must be split22 of that expression, bit for bit.

Every launch line of the tower plan (csrc/launch_plan.h plan_tower) is a test id below; the ids live in
tests/board_tower_cases.py (FP32_FORMS, SPLIT_FORMS, MANY), and tests/test_launch_plan_cpu.py holds every one of them, at
every cin0 and batch it is run with here, to the kernel and template arguments it names -- on the CPU, from the header
itself.  Not reached on the GPU: launch_board_tower_split<6,7,1,2> and <6,7,4>.  MZ_SPLIT_BOARDS selects them and is read
once per process; this file tests the default (2 boards on 4 wavefronts) only, the CPU test holds the plan of all three.
64 channels on 3 x 3 boards have no tower (179 KB / 189 KB of activation buffers whatever cin0 is): the plan refuses them by
name (tests/test_board_tower_reference.py holds the refusal).
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import board_tower_cases as cases
import board_tower_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
WORST = {}


@pytest.fixture(scope="module")
def lib(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native").load()


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


_packed = {}


def _pack(lib, case, split, const_plane):
    """Device copies of a case's parameters: [(packed, scale, shift, table)] per layer, cached per case."""
    key = (case["name"], split, const_plane)
    if key in _packed:
        return _packed[key]
    stream = torch.cuda.current_stream().cuda_stream
    h, w = case["h"], case["w"]
    out = []
    for l, (weight, scale, shift, _, _, _) in enumerate(case["layers"]):
        cout, cin = weight.shape[:2]
        wd = torch.from_numpy(weight).cuda()
        table = None
        if split:
            cp = 1 if (const_plane and l == 0) else 0
            packed = torch.empty(lib.mzmcts_board_conv_split_halfs(cin - cp, cout), dtype=torch.float16, device="cuda")
            table = torch.empty(cout * h * w, device="cuda")
            assert lib.mzmcts_board_conv_pack_split(wd.data_ptr(), packed.data_ptr(), table.data_ptr(), cin, cout, cp, h, w, stream) == 0
        else:
            packed = torch.empty(lib.mzmcts_board_conv_packed_floats(cin, cout), dtype=torch.float32, device="cuda")
            assert lib.mzmcts_board_conv_pack(wd.data_ptr(), packed.data_ptr(), cin, cout, stream) == 0
        out.append((packed, torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda(), table))
    torch.cuda.synchronize()
    _packed[key] = out
    return out


def _exports(case, batch, which):
    """NaN-filled export tensors, one sample longer than the batch: the extra one must keep its sentinel."""
    c, h, w = case["channels"], case["h"], case["w"]
    n = len(case["layers"])

    def fresh():
        t = torch.full((batch + 1, c, h, w), float("nan"), device="cuda")
        t[batch] = SENTINEL
        return t

    raws = [fresh() if (which == "all" or l == n - 1) else None for l in range(n)]
    units = [fresh() if case["layers"][l][5] else None for l in range(n)]      # (an export_unit IS the rescale: always given)
    return raws, units


def _descs(native, case, params, raws, units, split, const_plane, gate=None):
    n = len(case["layers"])
    descs = (native.MzTowerLayer * n)()
    for l, (weight, _, _, relu, skip, _) in enumerate(case["layers"]):
        packed, scale, shift, table = params[l]
        descs[l] = native.MzTowerLayer(packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                       table.data_ptr() if (split and const_plane and l == 0) else None,
                                       raws[l].data_ptr() if raws[l] is not None else None,
                                       units[l].data_ptr() if units[l] is not None else None,
                                       weight.shape[1], relu, skip, 0, gate.data_ptr() if (gate is not None and l == 0) else None)
    return descs


def _collect(raws, units, batch):
    torch.cuda.synchronize()
    for t in raws + units:
        if t is not None:
            assert bool((t[batch] == SENTINEL).all()), "a launch wrote past its last sample"
    return ([t[:batch].cpu().numpy() if t is not None else None for t in raws],
            [t[:batch].cpu().numpy() if t is not None else None for t in units])


def launch(lib, native, case, batch, split=False, const_plane=False, x=None, gather=None, which="all", heads=None):
    """One tower launch; returns (raws, units) as numpy arrays (None where nothing was exported)."""
    params = _pack(lib, case, split, const_plane or gather is not None)
    raws, units = _exports(case, batch, which)
    descs = _descs(native, case, params, raws, units, split, const_plane or gather is not None)
    stream = torch.cuda.current_stream().cuda_stream
    c, h, w, n = case["channels"], case["h"], case["w"], len(case["layers"])
    keep = []
    if gather is not None:
        pool, parent, action, actions = (torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in gather)
        keep = [pool, parent, action]
        g = native.MzTowerGather(pool.data_ptr(), parent.data_ptr(), action.data_ptr(), batch, c * h * w, float(actions))
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        keep = [xd]
    if heads is not None:
        rc = lib.mzmcts_board_tower_heads(None if gather is not None else xd.data_ptr(), ctypes.addressof(g) if gather is not None else None,
                                          batch, case["cin0"], c, h, w, ctypes.addressof(descs), n, ctypes.addressof(heads), len(heads), stream)
    elif gather is not None:
        rc = lib.mzmcts_board_tower_gathered(ctypes.byref(g), batch, case["cin0"], 1 if split else 0, c, h, w, ctypes.addressof(descs), n, stream)
    elif split:
        rc = lib.mzmcts_board_tower_split(xd.data_ptr(), batch, case["cin0"], 1 if const_plane else 0, c, h, w, ctypes.addressof(descs), n, stream)
    else:
        rc = lib.mzmcts_board_tower(xd.data_ptr(), batch, case["cin0"], c, h, w, ctypes.addressof(descs), n, stream)
    assert rc == 0, (case["name"], batch, rc)
    out = _collect(raws, units, batch)
    del keep
    return out


PERIOD = 509                  # (prime: no multiple of any form's samples per wavefront or workgroup)


def run_and_judge(lib, native, form, case, batch, split=False, const_plane=False, gathered=False, heads=None, seed=0):
    """Launch, then the three verdicts of the module docstring.  Returns (raws, units, x).

    Above 4096 boards the float64 work is kept to a few seconds: samples are independent of each other, so the verdicts
    are given on a subset -- the first PERIOD samples, the last 130 (the ragged end) and every 61st in between -- and, for
    a tensor input, sample b is given sample b % PERIOD's boards, so that EVERY sample's exports are held, bit for bit, to
    those of a sample inside the judged subset."""
    denom = 1
    large = batch > 4096
    if gathered:
        gather = cases.case_gather(case, batch, 100 + seed + batch)
        x = cases.gathered_input(case, *gather)
        denom = gather[3] if case["integer"] else 1
        raws, units = launch(lib, native, case, batch, split=split, gather=gather, heads=heads)
    else:
        x = cases.case_input(case, min(batch, PERIOD) if large else batch, 200 + seed + batch, const_plane=const_plane)
        if large:
            x = np.ascontiguousarray(x[np.arange(batch) % PERIOD])
        raws, units = launch(lib, native, case, batch, split=split, const_plane=const_plane, x=x, heads=heads)
    what = (form, case["name"], f"batch {batch}", "gathered" if gathered else ("const plane" if const_plane else "tensor"))
    judged = slice(None)
    if large:
        if not gathered:
            for l, t in enumerate(raws + units):
                assert t is None or ref.same_bits(t, t[np.arange(batch) % PERIOD]), (what, "equal boards, different exports", l)
        judged = np.unique(np.concatenate([np.arange(PERIOD), np.arange(PERIOD, batch, 61), np.arange(batch - 130, batch)]))
    pick = lambda ts: [t[judged] if t is not None else None for t in ts]
    reference = ref.tower_reference(x[judged], case["layers"], exact=True, split=split, denom=denom) if case["integer"] else None
    failures, worst = ref.judge_exports(x[judged], case["layers"], pick(raws), pick(units), split=split, reference=reference)
    assert not failures, (what, failures[:3])
    if not case["integer"]:
        seen = WORST.setdefault(form, dict(all=0.0, ordinary=0.0))
        for k in seen:
            seen[k] = max(seen[k], worst[k])
    return raws, units, x


def report(form):
    print(f"{form}: worst error / bound over the float64-mode towers = {WORST[form]['ordinary']:.3f} "
          f"({WORST[form]['all']:.3f} with the tiny-span channels, whose single rounding next to 1.0 is the bound)")


def sweep(S, wide=None):
    """1 and k S - 1, k S, k S + 1 around the form's samples per wavefront / workgroup S (and around `wide`)."""
    out = {1, S + 1, 2 * S - 1, 2 * S, 2 * S + 1}
    if S > 1:
        out |= {S - 1, S}
    if wide:
        out |= {wide - 1, wide, wide + 1, 2 * wide - 1, 2 * wide, 2 * wide + 1}
    return sorted(b for b in out if b >= 1)


def exercise(lib, native, form, h, w, channels, cin0s, S, wide=None, split=False):
    """The whole programme of one form: every cin0; the standard towers; the full batch sweep on the dynamics + prediction
    tower of the first cin0; 16 layers; exports on every layer and on none but the last; gathered input where cin0 =
    channels + 1."""
    for i, cin0 in enumerate(cin0s):
        planes = (False, True) if (split and cin0 >= 2) else (False,)
        for const_plane in planes:
            for case in cases.standard_cases(h, w, cin0, channels, split=split):
                if const_plane and cin0 <= channels and len(case["layers"]) > 1 and case["layers"][1][4]:
                    continue        # (a layer-1 skip would read the constant plane: refused, tests/test_board_tower_reference.py)
                full = i == 0 and case["name"].startswith("dynpred5") and const_plane == planes[-1]
                for batch in (sweep(S, wide) if full else (1, 2 * S + 1)):
                    raws, units, x = run_and_judge(lib, native, form, case, batch, split=split, const_plane=const_plane)
                if case["name"].startswith("dynpred5"):
                    # raw exports on none but the last layer (the unit exports stay: they ARE the rescale): the same bits
                    last_raw, last_unit = launch(lib, native, case, batch, split=split, const_plane=const_plane, x=x, which="last")
                    assert all(r is None for r in last_raw[:-1])
                    assert ref.same_bits(last_raw[-1], raws[-1]), (form, case["name"])
                    assert all(ref.same_bits(u, v) for u, v in zip(last_unit, units) if v is not None), (form, case["name"])
        if cin0 == channels + 1:
            for case in cases.standard_cases(h, w, cin0, channels, split=split):
                if case["name"].startswith(("dynpred5", "float5", "root3")):
                    for batch in (1, S + 1, 2 * S - 1) + ((wide + 1,) if wide else ()):
                        run_and_judge(lib, native, form, case, batch, split=split, gathered=True)
    deep = cases.deep_case(h, w, cin0s[-1] if not split else 64, channels)
    for batch in (1, S + 1):
        run_and_judge(lib, native, form, deep, batch, split=split)
    if form in WORST:
        report(form)


FP32_FORMS, SPLIT_FORMS, MANY = cases.FP32_FORMS, cases.SPLIT_FORMS, cases.MANY    # (the launch lines; tests/test_launch_plan_cpu.py
                                                                                    #  holds every id to the kernel it names)


@pytest.mark.parametrize("form", FP32_FORMS, ids=[f[0] for f in FP32_FORMS])
def test_fp32_tower_forms(lib, native, monkeypatch, form):
    name, channels, h, w, cols, S, wide, cin0s = form
    if cols is None:
        monkeypatch.delenv("MZ_TOWER_COLS", raising=False)
    else:
        monkeypatch.setenv("MZ_TOWER_COLS", cols)
    for cin0 in cin0s:
        assert lib.mzmcts_board_conv_supported(cin0, channels, h, w)
    exercise(lib, native, name, h, w, channels, cin0s, S, wide)


@pytest.mark.parametrize("form", SPLIT_FORMS, ids=[f[0] for f in SPLIT_FORMS])
def test_split_tower_forms(lib, native, form):
    """cin0 in {2, 64, 65, 80} with and without a constant last plane; cin0 = 2 with one is a ONE-channel convolution."""
    name, h, w, S, cin0s = form
    assert lib.mzmcts_board_tower_blocks(2 * S + 1, 64, h, w) == 3          # (S is the form's block)
    exercise(lib, native, name, h, w, 64, cin0s, S, split=True)


@pytest.mark.parametrize("form", MANY, ids=[f[0] for f in MANY])
def test_sixteen_channel_towers_across_the_many_switch(lib, native, monkeypatch, form):
    """16383 boards take the few-boards instantiation, 16384 and 16385 the many-boards one (other samples per workgroup,
    ragged last workgroups): the same integers from both."""
    name, h, w, cols, cin0 = form
    if cols is None:
        monkeypatch.delenv("MZ_TOWER_COLS", raising=False)
    else:
        monkeypatch.setenv("MZ_TOWER_COLS", cols)
    standard = cases.standard_cases(h, w, cin0, 16)
    two, dynpred = standard[1:3]
    for batch in (16383, 16384, 16385):
        run_and_judge(lib, native, name, two, batch)
    if h * w == 9:
        run_and_judge(lib, native, name, dynpred, 16385)
    if cin0 == 17:
        assert standard[5]["name"].startswith("rootfloat3")
        run_and_judge(lib, native, name, standard[5], 16385, gathered=True)
        report(name)


def _head(native, rs, reduced, hidden, outputs, batch, layer, keep):
    tensors = [torch.from_numpy((0.3 * rs.standard_normal(shape)).astype(np.float32)).cuda()
               for shape in ((reduced, 16), (reduced,), (hidden, reduced * 9), (hidden,), (outputs, hidden), (outputs,))]
    out = torch.full((batch, outputs), float("nan"), device="cuda")
    keep += tensors + [out]
    desc = native.MzHeadDesc(*[t.data_ptr() for t in tensors], 16, 9, reduced, hidden, outputs)
    return native.MzTowerHead(desc, out.data_ptr(), layer, 0), out


def test_cols_tower_with_heads_exports_the_same_numbers(lib, native, monkeypatch):
    """launch_board_tower_cols, HEADS instantiation (mzmcts_board_tower_heads): a head on the middle rescale layer and two
    on the last layer; the layers' exports are held to the same verdicts as the plain launch (the logits are not judged
    here: tests/test_gpu_board_conv.py compares them with the two-launch form)."""
    monkeypatch.delenv("MZ_TOWER_COLS", raising=False)
    rs = np.random.RandomState(8)
    for case in cases.standard_cases(3, 3, 17, 16)[2:4]:               # dynpred5 (integers), float5: rescales on layers 2 and 4
        for batch in (1, 17, 65):
            for gathered in (False, True):
                keep = []
                made = [_head(native, rs, 3, 8, 21, batch, 2, keep), _head(native, rs, 2, 16, 9, batch, 4, keep),
                        _head(native, rs, 16, 5, 32, batch, 4, keep)]
                heads = (native.MzTowerHead * 3)(*[m[0] for m in made])
                run_and_judge(lib, native, "launch_board_tower_cols<heads>", case, batch, gathered=gathered, heads=heads)
                for _, out in made:
                    assert bool(torch.isfinite(out).all())
    report("launch_board_tower_cols<heads>")


def test_gated_pair_hands_overflowed_blocks_to_the_fp32_tower(lib, native):
    """The overflow hand-over by direct calls: a 64-channel 6 x 7 tower of 5 layers on 1029 boards = 515 split blocks of 2
    and 258 fp32 blocks of 4 on a grid of 256 workgroups, so two workgroups take a second trip through the gate loop and
    the last block is ragged.  Sample 5 overflows in its input, 1026 and 1028 in a later layer; every value stays below 2^24,
    so BOTH forms are exact on what they keep: every export of every sample must be the integers, the gate entries exactly
    what the flagged samples imply, and an unflagged split block that shares an fp32 workgroup with a flagged one is
    re-run with the same integers.  (NaN / inf are made on purpose inside the split launch, as the existing overflow test
    does; nothing faults.)"""
    case, x, loose = cases.gate_case()
    batch, S = x.shape[0], 2
    blocks = int(lib.mzmcts_board_tower_blocks(batch, 64, 6, 7))
    assert blocks == (batch + S - 1) // S
    gate = torch.full((blocks + 1,), 7, dtype=torch.int32, device="cuda")
    gate[blocks] = 0                                                  # (the count is the caller's to clear; the entries are written)
    raws, units = _exports(case, batch, "all")
    xd = torch.from_numpy(x).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    n = len(case["layers"])
    split_descs = _descs(native, case, _pack(lib, case, True, False), raws, units, True, False, gate=gate)
    assert lib.mzmcts_board_tower_split(xd.data_ptr(), batch, 64, 0, 64, 6, 7, ctypes.addressof(split_descs), n, stream) == 0
    fp32_descs = _descs(native, case, _pack(lib, case, False, False), raws, units, False, False, gate=gate)
    assert lib.mzmcts_board_tower(xd.data_ptr(), batch, 64, 64, 6, 7, ctypes.addressof(fp32_descs), n, stream) == 0
    got_raws, got_units = _collect(raws, units, batch)
    flags = gate.cpu().numpy()
    want = np.zeros(blocks + 1, dtype=np.int32)
    want[[s // S for s in loose]] = 1
    want[blocks] = len({s // S for s in loose})
    assert np.array_equal(flags, want), (np.nonzero(flags[:blocks])[0], flags[blocks])
    rerun = np.zeros(batch, dtype=bool)                               # samples of the fp32 workgroups (4 boards) that ran
    for s in loose:
        rerun[(s // 4) * 4:(s // 4) * 4 + 4] = True
    reference = ref.tower_reference(x, case["layers"], exact=True, split=True, loose=loose)
    failures, _ = ref.judge_exports(x, case["layers"], got_raws, got_units, split=True, reference=reference, samples=~rerun)
    assert not failures, failures[:3]
    assert reference["exact_upto"] == n - 1
    for l in range(n):
        assert np.array_equal(got_raws[l].astype(np.float64), reference["raw"][l]), l
