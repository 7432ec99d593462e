"""Yardsticks, cases and argument builders for the backward of the hidden state's min-max rescale in training
(csrc/rescale_train.h, include/mztrain.h mztrain_rescale_*), shared by tests/test_rescale_train_cpu.py and
tests/test_gpu_rescale_train.py.

  run64      the rule in float64 throughout (numpy): what torch's float64 expression with autograd is held to, and what the
             training-step rule measures errors against
  run_rule   the rule as the header states it: minimum, maximum, span and y in float32, everything after in float64 with
             sequential sums -- the host entry's and the kernel's bits; `defect` breaks it in one of five ways
  run_torch  models._unit_rescale, the division and autograd in a dtype of torch's, on a device

A case is {"x": f32[rows, P], "g": f32[rows, P]}."""
import ctypes

import numpy as np
import torch

U = 2.0 ** -24
MAX_ROW_LEN, BLOCK, MIN_ROWS, SPREAD, LDS_BYTES = 128, 256, 16, 256, 160 * 1024


# ---- the plan, restated -------------------------------------------------------------------------------------------------------
def plan(rows, row_len):
    """(grid, block, rows per workgroup, row stride, LDS bytes) of csrc/rescale_train.h plan_rescale_backward."""
    stride = row_len | 1
    fit = LDS_BYTES // (2 * 4 * stride)
    per_group = min(max(-(-rows // SPREAD), MIN_ROWS), BLOCK, fit)
    return -(-rows // per_group), BLOCK, per_group, stride, 2 * 4 * per_group * stride


def library_plan(lib, rows, row_len):
    out = (ctypes.c_int64 * 5)()
    rc = lib.mztrain_rescale_backward_plan(rows, row_len, out)
    return rc, tuple(out)


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def _shapes():
    shapes = [(1, p) for p in (1, 2, 9, 36, 42, 121, 128)]
    for p in (9, 42, 128):                                  # around the rows per workgroup of a small launch
        per_group = plan(MIN_ROWS, p)[2]
        shapes += [(per_group - 1, p), (per_group, p), (per_group + 1, p)]
    shapes += [(2 * 16, 9), (2 * 64, 42), (2 * 128, 121)]   # the configs' hidden states at B = 2
    shapes += [(3 * 16 + 5, 2), (37, 1)]                    # several workgroups of the shortest rows
    return shapes


SHAPES = _shapes()
# where the plan's other two limits decide the rows per workgroup: the workgroup's 256 threads, and a CU's LDS at P = 128
LARGE_SHAPES = [(255 * SPREAD + 1, 9), (160 * SPREAD + 3, 128)]     # 256 rows of 9; 158 rows of 128, the last group partial
KINDS = ("normal", "relu", "constant", "span5e-6", "span2e-5")


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def make_case(shape, kind, seed):
    rows, p = shape
    rng = np.random.RandomState(seed)
    g = rng.standard_normal((rows, p)).astype(np.float32)
    if kind == "normal":
        x = rng.standard_normal((rows, p))
    elif kind == "relu":                                    # a plane's minimum is a run of zeros, as in the network
        x = np.maximum(rng.standard_normal((rows, p)), 0.0)
    elif kind == "constant":
        x = np.repeat(rng.standard_normal((rows, 1)), p, axis=1)
    elif kind in ("span5e-6", "span2e-5"):                  # either side of the 1e-5 branch; both extremes attained for P >= 2
        span = 5e-6 if kind == "span5e-6" else 2e-5
        unit = rng.rand(rows, p)
        if p >= 2:
            unit[:, 0], unit[:, -1] = 0.0, 1.0
        x = span * unit
    else:
        raise KeyError(kind)
    return {"x": np.ascontiguousarray(x, dtype=np.float32), "g": g}


INTEGER_SHAPES = [(1, 2), (5, 2), (7, 4), (33, 9), (17, 42), (3, 121), (18, 128)]


def integer_case(shape, seed):
    """Integer x with a span of 1, 2, 4 or 8 and 1, 2 or 4 positions at each extreme, small integer g: every quotient of the
    rule is dyadic and every value a multiple of 2^-8 well below 2^16, so float32, float64, any order of the sums and torch's
    own formulas all give the same numbers.  P >= 2."""
    rows, p = shape
    assert p >= 2
    rng = np.random.RandomState(seed)
    x = np.empty((rows, p), dtype=np.float32)
    for r in range(rows):
        pairs = [(a, b) for a in (1, 2, 4) for b in (1, 2, 4) if a + b <= p]
        n_lo, n_hi = pairs[rng.randint(len(pairs))]
        interior = p - n_lo - n_hi
        span = int(rng.choice((2, 4, 8) if interior else (1, 2, 4, 8)))
        lo = int(rng.randint(-4, 5))
        row = np.concatenate([np.full(n_lo, lo), np.full(n_hi, lo + span), rng.randint(lo + 1, lo + span, size=interior)
                              if interior else np.empty(0)])
        x[r] = rng.permutation(row)
        assert (x[r] == lo).sum() == n_lo and (x[r] == lo + span).sum() == n_hi and x[r].min() == lo and x[r].max() == lo + span
        assert span in (1, 2, 4, 8) and n_lo in (1, 2, 4) and n_hi in (1, 2, 4)
    g = rng.randint(-3, 4, size=(rows, p)).astype(np.float32)
    return {"x": x, "g": g}


def integer_bound(case):
    """An upper bound of |value| * 2^8 over every value the rule forms on an integer case (values are multiples of 2^-8):
    below 2^24 they are float32 numbers.  |g / s|, |S0|, |S1|, |dlo|, |dhi| <= sum |g|; |dx| <= max|g| + 2 sum |g|."""
    g = np.abs(case["g"].astype(np.float64))
    return 256.0 * float((g.max(axis=1) + 2.0 * g.sum(axis=1)).max())


def float32_sums_case():
    """One row on which float32 sums lose what float64 keeps: S0 = 2^24 + 1 + 1 - 2^24 is 2, and 0 when summed in float32
    (2^24 + 1 rounds back to 2^24 twice).  x = (0, 1, 1, 1/2), so y = x and S1 = 2 - 2^23 either way:
    dx_0 = g_0 + dlo = 2^24 - (S0 - S1) = 2^23; with S0 = 0 it is 2^23 + 2.  Every quotient is dyadic."""
    return {"x": np.array([[0, 1, 1, 0.5]], dtype=np.float32), "g": np.array([[2.0 ** 24, 1, 1, -2.0 ** 24]], dtype=np.float32)}


def directed_cases():
    zeros = np.array([[-0.0, 0.0, 3.0, 0.0, -0.0, 1.0]], dtype=np.float32)
    g6 = np.array([[1, -2, 3, 5, -7, 2]], dtype=np.float32)
    return {
        "a single position": {"x": np.array([[0.75], [-3.0]], dtype=np.float32), "g": np.array([[2.0], [-1.5]], dtype=np.float32)},
        "a constant plane": {"x": np.full((1, 9), 0.5, dtype=np.float32), "g": np.arange(1, 10, dtype=np.float32)[None] / 4},
        "every position at the minimum but one": {"x": np.array([[0, 0, 0, 0, 2.5, 0, 0, 0, 0]], dtype=np.float32),
                                                  "g": np.array([[1, 2, -3, 4, 5, -6, 7, 8, 9]], dtype=np.float32)},
        "both zeros as tied minima": {"x": zeros, "g": g6},
        "float32 sums lose": float32_sums_case(),
    }


# ---- the rule -----------------------------------------------------------------------------------------------------------------
DEFECTS = {"first index takes the tie": "relu", "no share for the maximum": "normal", "dlo without the span term": "normal",
           "sums in float32": "float32 sums lose", "no gradient through the 1e-5 branch": "span5e-6"}


def _backward(x, g, lo, hi, s, y, defect=None):
    """The rule's float64 part on float64 arrays; lo, hi, s are [rows, 1], y [rows, P]."""
    at_lo, at_hi = x == lo, x == hi
    if defect == "first index takes the tie":
        first = lambda mask: mask & (np.cumsum(mask, axis=1) == 1)
        at_lo, at_hi = first(at_lo), first(at_hi)
    n_lo, n_hi = at_lo.sum(axis=1, keepdims=True), at_hi.sum(axis=1, keepdims=True)
    if defect == "sums in float32":
        s0 = np.cumsum(g.astype(np.float32), axis=1, dtype=np.float32)[:, -1:].astype(np.float64)
        s1 = np.cumsum((g * y).astype(np.float32), axis=1, dtype=np.float32)[:, -1:].astype(np.float64)
    else:
        s0 = np.cumsum(g, axis=1)[:, -1:]                   # cumsum adds in ascending order, one term at a time
        s1 = np.cumsum(g * y, axis=1)[:, -1:]
    dlo = -(s0 - s1) / s
    dhi = -s1 / s
    if defect == "no share for the maximum":
        dhi = np.zeros_like(dhi)
    if defect == "dlo without the span term":
        dlo = -s0 / s
    if defect == "no gradient through the 1e-5 branch":     # the span as a constant wherever the branch was taken
        taken = (hi - lo) < 1e-5
        dlo, dhi = np.where(taken, -s0 / s, dlo), np.where(taken, 0.0, dhi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = g / s
        t = np.where(at_lo, t + dlo / n_lo, t)
        t = np.where(at_hi, t + dhi / n_hi, t)
    return t


def run64(case, defect=None):
    """dx in float64 throughout."""
    x, g = case["x"].astype(np.float64), case["g"].astype(np.float64)
    lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
    s = hi - lo
    s = np.where(s < 1e-5, s + 1e-5, s)
    return _backward(x, g, lo, hi, s, (x - lo) / s, defect)


def run_rule(case, defect=None):
    """dx as the header forms it: float32 up to y, float64 after, rounded once."""
    x32 = case["x"]
    lo, hi = x32.min(axis=1, keepdims=True), x32.max(axis=1, keepdims=True)      # (numpy's min and max let a NaN win, too)
    s = hi - lo
    s = np.where(s < np.float32(1e-5), s + np.float32(1e-5), s).astype(np.float32)
    y = ((x32 - lo) / s).astype(np.float32)
    f64 = lambda a: a.astype(np.float64)
    return _backward(f64(x32), f64(case["g"]), f64(lo), f64(hi), f64(s), f64(y), defect).astype(np.float32)


def terms(case):
    """max |g_p / s| over the tensor: the size of the terms dx is a sum of (they cancel; for P <= 2 down to zero)."""
    x, g = case["x"].astype(np.float64), case["g"].astype(np.float64)
    s = x.max(axis=1, keepdims=True) - x.min(axis=1, keepdims=True)
    s = np.where(s < 1e-5, s + 1e-5, s)
    return float(np.abs(g / s).max())


def run_torch(models, case, dtype, device="cpu"):
    """(y, dx) of the project's torch expression (models._unit_rescale, a division) with autograd."""
    x = torch.from_numpy(case["x"]).to(device=device, dtype=dtype).requires_grad_()
    shifted, span = models._unit_rescale(x, 1)
    y = shifted / span
    y.backward(torch.from_numpy(case["g"]).to(device=device, dtype=dtype))
    return y.detach().cpu().numpy(), x.grad.cpu().numpy()


# ---- the entries of include/mztrain.h -----------------------------------------------------------------------------------------
def backward_args(native, x, grad_out, grad_x, rows, row_len):
    """mztrain_rescale_backward_args from raw addresses (host or device; None stays a null pointer)."""
    return native.MzTrainRescaleBackwardArgs(x=x, grad_out=grad_out, grad_x=grad_x, rows=rows, row_len=row_len)


def run_host_entry(native, case):
    lib = native.load()
    x, g = np.ascontiguousarray(case["x"]), np.ascontiguousarray(case["g"])
    dx = np.full(x.shape, -1.0, dtype=np.float32)
    args = backward_args(native, x.ctypes.data, g.ctypes.data, dx.ctypes.data, x.shape[0], x.shape[1])
    rc = lib.mztrain_rescale_reference_backward(ctypes.byref(args))
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    return dx
