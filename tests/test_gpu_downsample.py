"""downsample_cnn_kernel (csrc/downsample_cnn.hip) driven through mzmcts_downsample_cnn directly (ctypes) and compared with a
yardstick that owes nothing to it (tests/downsample_reference.py; tests/test_net_head_reference.py holds it to account on
the CPU), over what the entry admits beyond the shipped shape: mid 4..10, cout 1..16, out_h and out_w 1..8 independently,
batches around the launch's grid of one workgroup per CU.  Three verdicts:

  exact         integer frames and weights, every partial sum below 2^24, pooling windows of 1, 2, 4, 8 or 16 elements:
                the integers (and their exact quotients), bit for bit;
  float64       seeded float frames and weights (both ReLUs cut a good share): every output within the bound the yardstick
                derives; the worst error / bound is printed by the last test of the file;
  independence  a frame's outputs are bit for bit those of the same frame in a batch of 1..16, wherever it sits in a large
                batch (first, second or last round of the persistent loop); a NaN in one frame reaches the outputs torch
                would hand it to, of that frame, and nothing else.

Frame b of a batch is frame b % 13 of thirteen seeded frames (13 is prime to every grid), so EVERY frame of every batch is
judged.  The output tensor is one frame longer than the batch and starts as NaN: the extra row holds a sentinel.
"""
import importlib

import numpy as np
import pytest
import torch

import downsample_reference as dref
import net_head_cases as cases
import net_head_reference as href

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
WORST = {"downsample_cnn_kernel": 0.0}
LAUNCHES = {"downsample_cnn_kernel": 0}
_frames, _wanted = {}, {}


@pytest.fixture(scope="module")
def lib(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native").load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def frames(integer):
    """(the thirteen base frames, their device copy), made once per kind."""
    if integer not in _frames:
        x = cases.down_frames(cases.FRAME_PERIOD, 77, integer)
        _frames[integer] = (x, torch.from_numpy(x).cuda())
    return _frames[integer]


def wanted(mid, cout, oh, ow, integer):
    """The yardstick's (outputs, bound) on the base frames; the six layers before the average once per (mid, cout, kind)."""
    key = (mid, cout, integer)
    if key not in _wanted:
        _wanted[key] = dref.downsample_features(frames(integer)[0], *cases.down_params(mid, cout, 10 * mid + cout, integer), exact=integer)
    return dref.adaptive_average(*_wanted[key], oh, ow, exact=integer)


def run(lib, x, params_d, mid, cout, oh, ow, batch=None, expect=0):
    batch = x.shape[0] if batch is None else batch
    out = torch.full((batch + 1, cout, oh, ow), float("nan"), device="cuda")
    out[batch] = SENTINEL
    w1, b1, w2, b2 = params_d
    rc = lib.mzmcts_downsample_cnn(x.data_ptr(), batch, 4, 84, 84, w1.data_ptr(), b1.data_ptr(), mid, 12, w2.data_ptr(), b2.data_ptr(),
                                   cout, oh, ow, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (mid, cout, oh, ow, batch, rc)
    assert bool((out[batch] == SENTINEL).all()), "the launch wrote past its last frame"
    if rc == 0 and batch > 0:
        LAUNCHES["downsample_cnn_kernel"] += 1
    return out[:batch].cpu().numpy()


def params_on_device(mid, cout, integer):
    return tuple(torch.from_numpy(a).cuda() for a in cases.down_params(mid, cout, 10 * mid + cout, integer))


def batch_of(base_d, batch):
    return base_d[torch.arange(batch, device="cuda") % base_d.shape[0]].contiguous()


def judge(lib, mid, cout, oh, ow, batch, integer, params_d=None):
    """One launch of `batch` frames, every frame held to the yardstick.  Returns the outputs."""
    params_d = params_d or params_on_device(mid, cout, integer)
    got = run(lib, batch_of(frames(integer)[1], batch), params_d, mid, cout, oh, ow)
    want, bound = wanted(mid, cout, oh, ow, integer)
    index = np.arange(batch) % cases.FRAME_PERIOD
    what = (f"mid {mid} cout {cout} out {oh} x {ow} batch {batch}", "integer" if integer else "float")
    if integer:
        wrong = np.argwhere(got.astype(np.float64) != want[index])
        assert len(wrong) == 0, (what, "first wrong (frame, channel, i, j)", wrong[0], got[tuple(wrong[0])], want[index][tuple(wrong[0])])
    else:
        ratio, where = href.judge(got, want[index], bound[index])
        print(what, f"worst error / bound {ratio:.4f} at", where)
        assert ratio <= 1.0, (what, ratio, where)
        WORST["downsample_cnn_kernel"] = max(WORST["downsample_cnn_kernel"], ratio)
    return got


@pytest.mark.parametrize("shape", cases.DOWN_SHAPES, ids=[f"mid{m}-cout{c}" for m, c in cases.DOWN_SHAPES])
def test_every_shape_at_three_frames_and_one_past_the_grid(lib, cus, shape):
    mid, cout = shape
    for integer in (True, False):
        params_d = params_on_device(mid, cout, integer)
        for oh, ow in cases.DOWN_OUTPUTS:
            few = judge(lib, mid, cout, oh, ow, 3, integer, params_d)
            many = judge(lib, mid, cout, oh, ow, cus + 1, integer, params_d)
            assert href.same_bits(few, many[:3]), (shape, oh, ow, "a frame's outputs depend on the batch")
            assert href.same_bits(many[cus], many[cus % cases.FRAME_PERIOD]), (shape, oh, ow, "the second round differs")


@pytest.mark.parametrize("shape", [((10, 16), (6, 6)), ((5, 3), (5, 3))], ids=["mid10-cout16-6x6", "mid5-cout3-5x3"])
def test_every_batch_around_the_grid_on_two_shapes(lib, cus, shape):
    (mid, cout), (oh, ow) = shape
    rs = np.random.RandomState(cus + mid)
    for integer in (True, False):
        params_d = params_on_device(mid, cout, integer)
        base_d = frames(integer)[1]
        # the thirteen frames in batches of 1..16 (the 16 wrap around): what every frame of every batch must equal, bit for bit
        alone = np.concatenate([run(lib, base_d[b:b + 1].contiguous(), params_d, mid, cout, oh, ow) for b in range(cases.FRAME_PERIOD)])
        for size in (2, 3, 5, 8, 13, 16):
            start = int(rs.randint(cases.FRAME_PERIOD))
            picked = (start + np.arange(size)) % cases.FRAME_PERIOD
            small = run(lib, base_d[torch.from_numpy(picked).cuda()].contiguous(), params_d, mid, cout, oh, ow)
            assert href.same_bits(small, alone[picked]), (shape, size, "a frame's outputs depend on the batch")
        for batch in cases.down_batches(cus):
            got = judge(lib, mid, cout, oh, ow, batch, integer, params_d)
            assert href.same_bits(got, alone[np.arange(batch) % cases.FRAME_PERIOD]), (shape, batch, "not the outputs of a batch of one")


@pytest.mark.parametrize("shape", [((7, 12), (6, 6)), ((4, 1), (1, 8)), ((10, 16), (3, 7))], ids=["mid7-cout12-6x6", "mid4-cout1-1x8", "mid10-cout16-3x7"])
def test_a_nan_stays_in_its_own_frame_and_goes_where_torch_takes_it(lib, cus, shape):
    (mid, cout), (oh, ow) = shape
    params = cases.down_params(mid, cout, 10 * mid + cout, False)
    params_d = params_on_device(mid, cout, False)
    batch = cus + 3
    x = batch_of(frames(False)[1], batch)
    clean = run(lib, x, params_d, mid, cout, oh, ow)
    victims = {1: (2, 3, 80), cus - 1: (0, 40, 41), cus + 1: (3, 83, 0)}         # first round, last workgroup, second round
    for b, (c, yy, xx) in victims.items():
        x[b, c, yy, xx] = float("nan")
    dirty = run(lib, x, params_d, mid, cout, oh, ow)
    others = np.array([b not in victims for b in range(batch)])
    assert href.same_bits(clean[others], dirty[others]), (shape, "a NaN reached another frame")
    want, bound = dref.downsample_reference(x[list(victims)].cpu().numpy(), *params, oh, ow)
    got = dirty[list(victims)]
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want)), (shape, "not torch's NaN pattern")
    sound = ~np.isnan(want)
    if sound.any():
        assert (np.abs(got - want)[sound] <= bound[sound]).all(), shape


def test_refusals_and_the_empty_batch(lib):
    """What tests/test_native_abi.py does not pin: an output height or width of 0, a width of 9, no output channel -- and
    that a refused or empty launch leaves the output alone (mid 3 / 11 and cout 17 once more, with real tensors)."""
    params_d = params_on_device(10, 16, False)
    x = frames(False)[1][:2].contiguous()

    def call(batch=2, mid=10, cout=16, oh=6, ow=6):
        out = torch.full((3, 16, 8, 8), SENTINEL, device="cuda")
        rc = lib.mzmcts_downsample_cnn(x.data_ptr(), batch, 4, 84, 84, params_d[0].data_ptr(), params_d[1].data_ptr(), mid, 12,
                                       params_d[2].data_ptr(), params_d[3].data_ptr(), cout, oh, ow, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), "a refused or empty launch wrote"
        return rc

    assert call(batch=0) == 0
    for refused in cases.DOWN_REFUSED + (dict(cout=0), dict(batch=-1)):
        assert call(**refused) == -1, refused


def test_zz_report():
    """Last in the file: the measured worst error / bound and the launches counted."""
    print(f"downsample_cnn_kernel: worst error / bound over the float64-mode cases = {WORST['downsample_cnn_kernel']:.4f}; "
          f"launches = {LAUNCHES['downsample_cnn_kernel']}")
    assert WORST["downsample_cnn_kernel"] <= 1.0
