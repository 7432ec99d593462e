"""The three head kernels -- conv_head_mfma_kernel and conv_head_kernel (csrc/net_kernels.hip), board_heads_cols_kernel
(csrc/board_conv.hip) -- driven through the C entry points directly (ctypes: mzmcts_conv_heads_multi, mzmcts_conv_heads; no
network module in between) and compared with a yardstick that owes nothing to them (tests/net_head_reference.py;
tests/test_net_head_reference.py holds it to account on the CPU).  tests/net_head_cases.py names, for every case, the kernel
and the compile-time form the dispatch takes.  Three verdicts:

  exact         integer heads whose hidden pre-activations are all positive (ELU is the identity) and whose partial sums
                stay below 2^24: every kernel and form must return the integers, bit for bit;
  float64       seeded float heads: every logit within parity_helpers.head_rounding_bound of the float64 yardstick; the
                worst error / bound per kernel is kept in WORST and printed by the last test of the file;
  independence  a sample's logits do not depend on the batch it runs in: bit for bit the same in every batch of a case, and,
                for the batches past a launch's grid cap, the same as in a batch of 1..16; a NaN in one board reaches that
                sample's logits and no other's.

Every output tensor is one sample longer than the batch and starts as NaN: the extra row holds a sentinel that must
survive, an unwritten logit shows.  LAUNCHES counts the launches per kernel as the restated dispatch predicts them (a
kernel trace of this file shows the same counts).
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import net_head_cases as cases
import net_head_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
WORST = {}
LAUNCHES = {"mfma": 0, "wave": 0, "cols": 0}
KERNEL_NAMES = {"mfma": "conv_head_mfma_kernel", "wave": "conv_head_kernel", "cols": "board_heads_cols_kernel"}


@pytest.fixture(scope="module")
def lib(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native").load()


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def _device_params(params):
    return [{k: torch.from_numpy(p[k]).cuda() for k in ref.KEYS} for p in params]


def launch(lib, native, shapes, dparams, xs, batch, cols_off=False, expect=0, single=False, monkeypatch=None):
    """One launch of the heads `shapes` on the device boards xs (one tensor per head; the same object twice = one tensor
    read by two heads).  Returns the logits per head as numpy [batch, O]; checks the sentinel rows."""
    if monkeypatch is not None:
        if cols_off:
            monkeypatch.setenv("MZ_HEADS_COLS", "off")
        else:
            monkeypatch.delenv("MZ_HEADS_COLS", raising=False)
    n = len(shapes)
    outs = []
    for s in shapes:
        out = torch.full((batch + 1, s[4]), float("nan"), device="cuda")
        out[batch] = SENTINEL
        outs.append(out)
    descs = (native.MzHeadDesc * n)(*[native.MzHeadDesc(*[p[k].data_ptr() for k in ref.KEYS], *s) for s, p in zip(shapes, dparams)])
    x_ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    out_ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    stream = torch.cuda.current_stream().cuda_stream
    if single:
        assert all(x is xs[0] for x in xs)
        rc = lib.mzmcts_conv_heads(xs[0].data_ptr(), ctypes.addressof(descs), n, ctypes.addressof(out_ptrs), batch, stream)
    else:
        rc = lib.mzmcts_conv_heads_multi(ctypes.addressof(x_ptrs), ctypes.addressof(descs), n, ctypes.addressof(out_ptrs), batch, stream)
    torch.cuda.synchronize()
    assert rc == expect, (shapes, batch, rc)
    kernel = cases.dispatch(shapes, cols_off)
    if rc == 0 and batch > 0:
        LAUNCHES[kernel] += 1
    for out in outs:
        assert bool((out[batch] == SENTINEL).all()), ("a launch wrote past its last sample", shapes, batch)
    return [out[:batch].cpu().numpy() for out in outs]


def _boards(base_d, batch):
    """Sample b of a batch is given board b % (boards there are): one device tensor per distinct base tensor."""
    made = {}
    out = []
    for base in base_d:
        if id(base) not in made:
            index = torch.arange(batch, device="cuda") % base.shape[0]
            made[id(base)] = base[index].contiguous()
        out.append(made[id(base)])
    return out


def _base_tensors(boards):
    made = {}
    for b in boards:
        if id(b) not in made:
            made[id(b)] = torch.from_numpy(b).cuda()
    return [made[id(b)] for b in boards]


RUNNABLE = [c for c in sorted(cases.HEAD_CASES) if cases.HEAD_CASES[c]["kernel"] != "none"]


@pytest.mark.parametrize("case_id", RUNNABLE)
def test_head_case(lib, native, monkeypatch, case_id):
    case = cases.HEAD_CASES[case_id]
    shapes, kernel, cols_off = case["shapes"], case["kernel"], case["cols_off"]
    assert cases.dispatch(shapes, cols_off) == kernel
    rs = np.random.RandomState(cases.case_seed(case_id))
    for integer in (True, False):
        params, boards = cases.case_data(case_id, integer)
        dparams, base_d = _device_params(params), _base_tensors(boards)
        wanted = [ref.head_reference(x, p, exact=integer) for x, p in zip(boards, params)]       # once per case and kind
        period = boards[0].shape[0]
        seen = None                                                   # the largest batch's logits so far
        for batch in sorted(case["batches"], reverse=True):
            xs = _boards(base_d, batch)
            got = launch(lib, native, shapes, dparams, xs, batch, cols_off=cols_off, monkeypatch=monkeypatch)
            index = np.arange(batch) % period
            for h, (out, (want, bound)) in enumerate(zip(got, wanted)):
                what = (case_id, kernel, shapes[h], f"batch {batch}", "integer" if integer else "float")
                if integer:
                    wrong = np.argwhere(out.astype(np.float64) != want[index])
                    assert len(wrong) == 0, (what, "first wrong (sample, logit)", wrong[0], out[tuple(wrong[0])], want[index][tuple(wrong[0])])
                else:
                    ratio, where = ref.judge(out, want[index], bound[index])
                    print(what, f"worst error / bound {ratio:.4f} at", where)
                    assert ratio <= 1.0, (what, ratio, where)
                    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
                if seen is not None:                                  # the same boards in a larger batch: the same bits
                    assert ref.same_bits(out, seen[h][:batch]), (what, "logits depend on the batch size")
            if seen is None:
                seen = got
            if kernel == "cols":                                      # conv_head_mfma_kernel's arithmetic, operation for operation
                other = launch(lib, native, shapes, dparams, xs, batch, cols_off=True, monkeypatch=monkeypatch)
                assert cases.dispatch(shapes, True) == "mfma"
                assert all(ref.same_bits(a, b) for a, b in zip(got, other)), (case_id, batch, "cols and mfma kernels differ")
            if batch > 4096:
                # past the grid cap: equal boards, equal logits (every sample is thereby held to one of the first `period`,
                # which are judged above), and a seeded subset again in batches of 1..16
                for h, out in enumerate(got):
                    assert ref.same_bits(out, out[index]), (case_id, batch, "equal boards, different logits")
                subset = rs.choice(batch, size=256, replace=False)
                subset[:3] = (0, batch - 1, cases.samples_per_round(shapes, kernel) % batch)
                at = 0
                while at < len(subset):
                    few = subset[at:at + int(rs.randint(1, 17))]
                    at += len(few)
                    picked = torch.from_numpy(few).cuda()
                    small = launch(lib, native, shapes, dparams, [x[picked].contiguous() for x in xs], len(few),
                                   cols_off=cols_off, monkeypatch=monkeypatch)
                    for h in range(len(shapes)):
                        assert ref.same_bits(small[h], got[h][few]), (case_id, batch, few, "not the logits of a small batch")
        if len({id(b) for b in boards}) == 1:                         # one tensor for all heads: the single-input entry as well
            xs = _boards(base_d, min(case["batches"]))
            again = launch(lib, native, shapes, dparams, xs, min(case["batches"]), cols_off=cols_off, single=True, monkeypatch=monkeypatch)
            assert all(ref.same_bits(a, b[:min(case["batches"])]) for a, b in zip(again, seen)), case_id


@pytest.mark.parametrize("case_id", ["H2", "H4", "H6", "H11", "H9d", "W2", "W4e", "W7"])
def test_a_nan_stays_in_its_own_sample(lib, native, monkeypatch, case_id):
    """The matrix-core kernels multiply padded operand lanes by zero and share a tile between 16 samples: a NaN in one
    board must reach every logit of that sample (every hidden unit reads the poisoned position) and no other sample."""
    case = cases.HEAD_CASES[case_id]
    shapes = case["shapes"]
    params, boards = cases.case_data(case_id, False)
    dparams, base_d = _device_params(params), _base_tensors(boards)
    batch, victim = 37, 21
    xs = [x.clone() for x in _boards(base_d, batch)]
    clean = launch(lib, native, shapes, dparams, xs, batch, cols_off=case["cols_off"], monkeypatch=monkeypatch)
    c, p = shapes[0][:2]
    for x in xs:
        x[victim, c - 1, p // 2] = float("nan")
    dirty = launch(lib, native, shapes, dparams, xs, batch, cols_off=case["cols_off"], monkeypatch=monkeypatch)
    others = np.arange(batch) != victim
    for a, b in zip(clean, dirty):
        assert np.isnan(b[victim]).all(), (case_id, "the NaN did not reach its own logits")
        assert ref.same_bits(a[others], b[others]), (case_id, "the NaN reached another sample")


def _filled_outs(shapes, batch):
    return [torch.full((batch + 1, s[4]), SENTINEL, device="cuda") for s in shapes]


def test_refusals_and_the_empty_batch(lib, native, monkeypatch):
    """R1 (no form fits 160 KB) returns MZMCTS_ERR_INVALID and leaves the outputs alone; so do an input pointer off 16
    bytes, heads that disagree on channels or plane (on the matrix-core and on the wave path) and 0 or 4 heads; an empty
    batch returns 0 and writes nothing, on every kernel's path."""
    monkeypatch.delenv("MZ_HEADS_COLS", raising=False)
    stream = torch.cuda.current_stream().cuda_stream

    def call(shapes, batch, x_offset=0, n_heads=None, single=False):
        params = [cases.head_params(s, 5, False) for s in shapes]
        dparams = _device_params(params)
        x = torch.zeros(max(batch, 1) * max(s[0] * s[1] for s in shapes) + 4, device="cuda")
        outs = _filled_outs(shapes, max(batch, 1))
        n = len(shapes)
        descs = (native.MzHeadDesc * n)(*[native.MzHeadDesc(*[q[k].data_ptr() for k in ref.KEYS], *s) for s, q in zip(shapes, dparams)])
        x_ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() + x_offset] * n)
        out_ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        if single:
            rc = lib.mzmcts_conv_heads(x.data_ptr() + x_offset, ctypes.addressof(descs), n if n_heads is None else n_heads,
                                       ctypes.addressof(out_ptrs), batch, stream)
        else:
            rc = lib.mzmcts_conv_heads_multi(ctypes.addressof(x_ptrs), ctypes.addressof(descs), n if n_heads is None else n_heads,
                                             ctypes.addressof(out_ptrs), batch, stream)
        torch.cuda.synchronize()
        if rc != 0 or batch == 0:
            assert all(bool((o == SENTINEL).all()) for o in outs), (shapes, batch, "a refused or empty launch wrote")
        else:
            assert all(bool((o[batch] == SENTINEL).all()) and bool(torch.isfinite(o[:batch]).all()) for o in outs)
        return rc

    r1 = cases.HEAD_CASES["R1"]["shapes"]
    assert cases.dispatch(r1) == "none" and call(r1, 3) == native.ERR_INVALID and call(r1, 0) == native.ERR_INVALID
    for case_id in ("H2", "H9c", "W2"):                                # an empty batch on each kernel's path
        assert call(cases.HEAD_CASES[case_id]["shapes"], 0) == 0
    for case_id in ("H2", "H9c", "W2"):
        shapes = cases.HEAD_CASES[case_id]["shapes"]
        assert call(shapes, 3, x_offset=4) == native.ERR_INVALID and call(shapes, 3, x_offset=8) == native.ERR_INVALID
        assert call(shapes[:1], 3, x_offset=4, single=True) == native.ERR_INVALID
    assert call([(17, 7, 3, 17, 17), (16, 7, 3, 17, 17)], 3) == native.ERR_INVALID         # channels, matrix-core path
    assert call([(17, 7, 3, 17, 17), (17, 6, 3, 17, 17)], 3) == native.ERR_INVALID         # plane
    assert call([(16, 9, 3, 8, 21), (16, 8, 3, 8, 21)], 3) == native.ERR_INVALID           # (the cols launch declines first)
    assert call([(4, 9, 17, 5, 3), (5, 9, 17, 5, 3)], 3) == native.ERR_INVALID             # channels, wave path
    assert call([(4, 9, 17, 5, 3), (4, 8, 17, 5, 3)], 3) == native.ERR_INVALID             # plane
    four = [(3, 5, 2, 5, 3)] * 4
    for single in (False, True):
        assert call(four, 3, n_heads=0, single=single) == native.ERR_INVALID
        assert call(four, 3, n_heads=4, single=single) == native.ERR_INVALID
    assert call(four[:3], 3) == 0 and call(four[:3], 3, single=True) == 0
    LAUNCHES["mfma"] += 2


def test_zz_report():
    """Last in the file: the measured worst error / bound per kernel and the launches the restated dispatch counted."""
    for kernel in ("mfma", "wave", "cols"):
        if kernel in WORST:
            print(f"{KERNEL_NAMES[kernel]}: worst error / bound over the float64-mode cases = {WORST[kernel]:.4f}; "
                  f"launches = {LAUNCHES[kernel]}")
            assert WORST[kernel] <= 1.0
