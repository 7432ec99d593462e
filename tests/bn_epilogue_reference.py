"""relu(batch_norm(x) [+ residual]) in training, forward and backward, in float64 numpy, restated from the formulas without
autograd: the yardstick the HIP training epilogue (csrc/bn_epilogue.h, include/mztrain.h mztrain_epilogue_*) is held to.
`defect` names a deliberate mistake, so that the tests can show which tensor each one pushes away."""
import ctypes

import numpy as np

U = 2.0 ** -24
EPS, MOMENTUM = 1e-5, 0.1
KEEP = 4096       # include/mztrain.h MZTRAIN_EPILOGUE_KEEP_VALUES: a channel of at most this many values stays in LDS
# [N, C, H, W]; what each covers
SHAPES = [
    (2, 1, 1, 1),        # M = 2, the smallest admitted
    (1, 3, 1, 2),        # the smallest multi-channel case
    (64, 16, 3, 3),      # TicTacToe
    (3, 15, 3, 3),       # 15 channels: the unaligned channel slices of the dynamics network
    (5, 4, 6, 7),        # Connect4's board
    (2, 2, 11, 11),      # Gomoku's board
    (255, 2, 1, 1), (256, 2, 1, 1), (257, 2, 1, 1),     # one value either side of the workgroup's thread count
    (256, 2, 4, 4),      # M = 4096 = KEEP: the largest channel kept in LDS between the passes
    (241, 2, 1, 17),     # M = 4097 = KEEP + 1: the smallest channel read again through L2
    (130, 2, 11, 11),    # 15 730 values per channel, past any LDS-resident form
]
assert 256 * 4 * 4 == KEEP and 241 * 17 == KEEP + 1
DEFECTS = {   # defect -> the tensor that shows it
    "biased_running_var": "running_var",
    "no_xhat_term": "dx",
    "mask_before_residual": "dx",
    "residual_gradient_unmasked": "dresidual",
    "m_minus_1_in_dx": "dx",
    "eps_outside_sqrt": "out",
}
OUTPUTS = ("out", "running_mean", "running_var", "dx", "dresidual", "dgamma", "dbeta")


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def make_case(shape, with_residual, seed=0, special=None):
    """float32 inputs of one epilogue: x with a different mean and spread per channel, gamma, beta, running statistics, an
    upstream gradient, [a residual].  special: "constant" (channel 0 is one constant: variance 0), "offset" (channel 0 has
    mean 1e4 and deviation 1), "zeros" (gamma = 1, beta = 0 and x = -x mirrored pairs with small integers in channel 0, so
    that batch-norm outputs are exactly 0 at some elements)."""
    n, c, h, w = shape
    rng = np.random.RandomState(7919 * seed + 31 * n + 17 * c + 5 * h + w + (1000 if with_residual else 0))
    x = rng.standard_normal(shape) * rng.uniform(0.25, 4.0, (1, c, 1, 1)) + rng.uniform(-3.0, 3.0, (1, c, 1, 1))
    gamma = rng.uniform(0.5, 1.5, c) * np.where(rng.random_sample(c) < 0.25, -1.0, 1.0)
    beta = rng.uniform(-0.5, 0.5, c)
    if special == "constant":
        x[:, 0] = 1.7
    elif special == "offset":
        x[:, 0] = 1e4 + rng.standard_normal((n, h, w))
    elif special == "zeros":
        m = n * h * w
        values = np.zeros(m)                         # mean 0 exactly; a third of the values are the mean itself
        half = m // 3
        values[:half] = rng.randint(1, 9, half)
        values[half:2 * half] = -values[:half]
        x[:, 0] = rng.permutation(values).reshape(n, h, w)
        gamma[0], beta[0] = 1.0, 0.0
    case = {"shape": shape, "x": x.astype(np.float32), "gamma": gamma.astype(np.float32), "beta": beta.astype(np.float32),
            "running_mean": rng.uniform(-1.0, 1.0, c).astype(np.float32),
            "running_var": rng.uniform(0.5, 2.0, c).astype(np.float32),
            "dy": (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 0, shape)).astype(np.float32),
            "residual": rng.standard_normal(shape).astype(np.float32) if with_residual else None}
    if special == "zeros" and with_residual:
        case["residual"][:, 0] = 0.0
    return case


def run64(case, eps=EPS, momentum=MOMENTUM, defect=None):
    """The rule in float64.  Returns every tensor of OUTPUTS (dresidual None without a residual) plus mean and invstd."""
    x = case["x"].astype(np.float64)
    n, c, h, w = x.shape
    m = n * h * w
    per = lambda v: np.asarray(v, dtype=np.float64).reshape(1, c, 1, 1)
    gamma, beta = per(case["gamma"]), per(case["beta"])
    mean = x.sum(axis=(0, 2, 3), keepdims=True) / m
    var = ((x - mean) ** 2).sum(axis=(0, 2, 3), keepdims=True) / m
    invstd = 1.0 / (np.sqrt(var) + eps) if defect == "eps_outside_sqrt" else 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * invstd
    bn = xhat * gamma + beta
    y = bn if case["residual"] is None else bn + case["residual"].astype(np.float64)
    out = np.maximum(y, 0.0)
    unbiased = var if defect == "biased_running_var" else var * m / (m - 1)
    running_mean = (1 - momentum) * case["running_mean"].astype(np.float64) + momentum * mean.reshape(c)
    running_var = (1 - momentum) * case["running_var"].astype(np.float64) + momentum * unbiased.reshape(c)
    dy = case["dy"].astype(np.float64)
    mask = (bn > 0) if defect == "mask_before_residual" else (out > 0)
    g = np.where(mask, dy, 0.0)
    dbeta = g.sum(axis=(0, 2, 3), keepdims=True)
    dgamma = (g * xhat).sum(axis=(0, 2, 3), keepdims=True)
    count = m - 1 if defect == "m_minus_1_in_dx" else m
    inner = g - dbeta / count
    if defect != "no_xhat_term":
        inner = inner - xhat * dgamma / count
    dx = gamma * invstd * inner
    dresidual = None
    if case["residual"] is not None:
        dresidual = dy.copy() if defect == "residual_gradient_unmasked" else g
    return {"out": out, "running_mean": running_mean, "running_var": running_var, "dx": dx, "dresidual": dresidual,
            "dgamma": dgamma.reshape(c), "dbeta": dbeta.reshape(c), "mean": mean.reshape(c), "invstd": invstd.reshape(c),
            "dx_terms": float(np.abs(gamma * invstd * g).max()), "m": m}


def run_torch(case, dtype, device="cpu", eps=EPS, momentum=MOMENTUM):
    """torch's own training expression, BatchNorm2d -> add -> relu with autograd, in `dtype` on `device`: the library of the
    rule (float32) and the check of the yardstick (float64).  Everything comes back as float64 numpy."""
    import torch
    c = case["shape"][1]
    to = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).to(device)
    bn = torch.nn.BatchNorm2d(c, eps=eps, momentum=momentum).to(dtype).to(device)
    with torch.no_grad():
        bn.weight.copy_(to(case["gamma"]))
        bn.bias.copy_(to(case["beta"]))
        bn.running_mean.copy_(to(case["running_mean"]))
        bn.running_var.copy_(to(case["running_var"]))
    bn.train()
    x = to(case["x"]).requires_grad_()
    residual = to(case["residual"]).requires_grad_() if case["residual"] is not None else None
    y = bn(x)
    if residual is not None:
        y = y + residual
    out = torch.relu(y)
    out.backward(to(case["dy"]))
    back = lambda t: t.detach().double().cpu().numpy().copy()
    return {"out": back(out), "running_mean": back(bn.running_mean), "running_var": back(bn.running_var), "dx": back(x.grad),
            "dresidual": back(residual.grad) if residual is not None else None, "dgamma": back(bn.weight.grad),
            "dbeta": back(bn.bias.grad)}


def ratio(native_value, library_value, exact, scale=None):
    """The project's rule for a training step: native error / (4 max(library error, 4 u max|exact|));
    0 / 0 = 0.  `scale` replaces max|exact| in the floor (see ratios)."""
    exact = np.asarray(exact, dtype=np.float64)
    scale = float(np.abs(exact).max()) if scale is None else float(scale)
    native_error = float(np.abs(np.asarray(native_value, dtype=np.float64) - exact).max())
    library_error = float(np.abs(np.asarray(library_value, dtype=np.float64) - exact).max())
    allowed = 4.0 * max(library_error, 4.0 * U * scale)
    value = native_error / allowed if allowed > 0 else (0.0 if native_error == 0 else float("inf"))
    return value, {"native": native_error, "library": library_error, "max_abs": scale, "ratio": value}


def ratios(got, library, exact):
    """ratio() per tensor of OUTPUTS that the case has: {name: (value, entry)}.

    One floor is not max|x64|.  With M = 2 values per channel xhat is (+a, -a), a^2 = var / (var + eps), and
    dx = gamma invstd (g - mean(g) - xhat mean(g xhat)) = gamma invstd (g1 - g2) / 2 * (1 - a^2) * (+1, -1): the three terms
    cancel down to eps / (var + eps), about 1e-6, of their own size.  max|dx64| then says nothing about the size of the
    numbers float32 rounds on the way, and a floor of 4 u max|dx64| would ask for a relative accuracy of 1e-13 in terms of
    the inputs, which no float32 expression has (torch's own is at 1e-11 or at 1e-9 depending on whether x1 + x2 happens to
    be a float).  For M = 2 the floor of dx is therefore 4 u max|gamma invstd g|, the size of the terms that cancel; every
    other tensor, and dx at every M >= 3, keeps max|x64|."""
    out = {}
    for key in OUTPUTS:
        if exact[key] is not None:
            scale = exact["dx_terms"] if key == "dx" and exact["m"] == 2 else None
            out[key] = ratio(got[key], library[key], exact[key], scale=scale)
    return out


# ---- the entries of include/mztrain.h ------------------------------------------------------------------------------------
def forward_args(native, shape, x, residual, gamma, beta, running_mean, running_var, out, save_mean, save_invstd, eps=EPS,
                 momentum=MOMENTUM):
    """mztrain_epilogue_forward_args from raw addresses (host or device; None stays a null pointer)."""
    n, c, h, w = shape
    return native.MzTrainEpilogueForwardArgs(x=x, residual=residual, gamma=gamma, beta=beta, running_mean=running_mean,
                                             running_var=running_var, out=out, save_mean=save_mean, save_invstd=save_invstd,
                                             batch=n, channels=c, hw=h * w, eps=eps, momentum=momentum)


def backward_args(native, shape, dy, x, out, gamma, save_mean, save_invstd, dx, dresidual, dgamma, dbeta):
    n, c, h, w = shape
    return native.MzTrainEpilogueBackwardArgs(dy=dy, x=x, out=out, gamma=gamma, save_mean=save_mean, save_invstd=save_invstd,
                                              dx=dx, dresidual=dresidual, dgamma=dgamma, dbeta=dbeta, batch=n, channels=c,
                                              hw=h * w)


def run_host_entry(native, case, eps=EPS, momentum=MOMENTUM):
    """Forward and backward through mztrain_epilogue_reference_* on host arrays (float32): every tensor of OUTPUTS plus
    "mean" and "invstd" as float32 arrays; the inputs are checked to come back unchanged."""
    lib = native.load()
    shape = case["shape"]
    c = shape[1]
    inputs = {k: np.ascontiguousarray(case[k]) for k in ("x", "gamma", "beta", "dy")}
    residual = np.ascontiguousarray(case["residual"]) if case["residual"] is not None else None
    kept = {k: v.copy() for k, v in inputs.items()}
    running_mean, running_var = case["running_mean"].copy(), case["running_var"].copy()
    out = np.full(shape, np.nan, dtype=np.float32)
    mean, invstd = np.full(c, np.nan, dtype=np.float32), np.full(c, np.nan, dtype=np.float32)
    address = lambda a: a.ctypes.data if a is not None else None
    args = forward_args(native, shape, address(inputs["x"]), address(residual), address(inputs["gamma"]),
                        address(inputs["beta"]), address(running_mean), address(running_var), address(out), address(mean),
                        address(invstd), eps=eps, momentum=momentum)
    rc = lib.mztrain_epilogue_reference_forward(ctypes.byref(args))
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    dx = np.full(shape, np.nan, dtype=np.float32)
    dresidual = np.full(shape, np.nan, dtype=np.float32) if residual is not None else None
    dgamma, dbeta = np.full(c, np.nan, dtype=np.float32), np.full(c, np.nan, dtype=np.float32)
    args = backward_args(native, shape, address(inputs["dy"]), address(inputs["x"]), address(out), address(inputs["gamma"]),
                         address(mean), address(invstd), address(dx), address(dresidual), address(dgamma), address(dbeta))
    rc = lib.mztrain_epilogue_reference_backward(ctypes.byref(args))
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    for key, value in inputs.items():
        assert np.array_equal(value.view(np.uint32), kept[key].view(np.uint32)), f"{key} was written"
    return {"out": out, "running_mean": running_mean, "running_var": running_var, "dx": dx, "dresidual": dresidual,
            "dgamma": dgamma, "dbeta": dbeta, "mean": mean, "invstd": invstd}
