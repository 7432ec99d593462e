"""The reward / value / policy heads of a residual network in training -- 1 x 1 convolution with bias, flatten (r * P + p),
Linear, ELU, Linear, forward and backward -- in float64 numpy, restated from the formulas without autograd: the yardstick the
HIP head launches (csrc/head_train.h, include/mztrain.h mztrain_heads_*) are held to.  `defect` names a deliberate mistake, so
that the tests can show which tensor each one pushes away.

A shape is (B, C, P, ((R, Hd, O), ...)): one or two heads reading one x [B, C, P].  A case is a dict of float32 arrays: "x",
and per head k "conv_w{k}" [R, C], "conv_b{k}", "fc1_w{k}" [Hd, R P], "fc1_b{k}", "fc2_w{k}" [O, Hd], "fc2_b{k}",
"dlogits{k}" [B, O].  Results carry per head "logits", "flat", "pre", "dpre", "dflat", "dconv_w", "dconv_b", "dfc1_w", "dfc1_b",
"dfc2_w", "dfc2_b" (each with the head's index appended) and one "dx"."""
import ctypes

import numpy as np

U = 2.0 ** -24
ELU_ULPS = 4          # include/mztrain.h MZTRAIN_HEADS_ELU_ULPS
LANES = 16            # csrc/head_train.h kReduceLanes: partial sums of a parameter gradient's entry
PARAMS = ("conv_w", "conv_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
PER_HEAD = ("logits", "flat", "pre", "dpre", "dflat") + tuple("d" + p for p in PARAMS)

TICTACTOE = ((16, 8, 21), (16, 8, 9))                 # value, policy; the reward head is the value head's shape
CONNECT4 = ((2, 64, 21), (4, 64, 7))
GOMOKU = ((2, 64, 21), (4, 64, 121))
SHAPES = [
    (64, 16, 9, TICTACTOE), (64, 16, 9, TICTACTOE[:1]),            # the TicTacToe config: value + policy, reward
    (64, 64, 42, CONNECT4), (64, 64, 42, CONNECT4[:1]),            # the Connect4 config
    (1, 16, 9, TICTACTOE),                                         # one sample: 15 of the 16 partial sums are empty
    (2, 5, 6, ((3, 5, 4),)),
    (15, 5, 6, ((3, 5, 4), (2, 3, 6))), (16, 5, 6, ((3, 5, 4),)), (17, 5, 6, ((3, 5, 4), (2, 3, 6))),   # either side of 16 partials
    (65, 5, 6, ((3, 5, 4),)),                                      # a fifth term in partial 0 only
    (3, 7, 1, ((2, 3, 5), (1, 2, 3))),                             # P = 1
    (4, 6, 4, ((1, 6, 3),)),                                       # R = 1
    (5, 4, 9, ((2, 1, 4),)),                                       # Hd = 1
    (5, 4, 9, ((3, 7, 5), (2, 6, 2))),                             # Hd no multiple of 4; R P = 27 and 18: ragged fc1 partial chains
    (3, 8, 9, ((2, 5, 1), (2, 5, 121))),                           # O = 1 and O = 121
    (4, 15, 9, ((4, 8, 9),)), (4, 17, 9, TICTACTOE),               # C = 15 and 17
    (3, 16, 36, ((8, 9, 5), (8, 9, 5))),                           # R P = 288: more flat entries than a workgroup has threads
    (2, 128, 121, GOMOKU[:1]), (17, 128, 121, GOMOKU),             # Gomoku's heads (its batch of 512 is not run)
]
DEFECTS = {   # defect -> the tensor that shows it
    "elu_slope_one": "dpre0",
    "flatten_position_major": "logits0",
    "conv_bias_without_positions": "dconv_b0",
    "fc1_gradient_transposed": "dfc1_w0",
    "dx_without_second_head": "dx",
}


def shape_id(shape):
    b, c, p, heads = shape
    return f"B{b}-C{c}-P{p}-" + "+".join("R{}H{}O{}".format(*h) for h in heads)


def _rng(shape, seed):
    b, c, p, heads = shape
    return np.random.RandomState(104729 * seed + 31 * b + 17 * c + 5 * p + 3 * len(heads) + sum(sum(h) for h in heads))


def normal_case(shape, seed, dlogits_scale=1e-3):
    """Magnitudes of a training step: x in [0, 1] (rescaled states), weights uniform within 1 / sqrt(fan-in) as torch
    initialises them, the gradient of the logits of order `dlogits_scale`."""
    b, c, p, heads = shape
    rng = _rng(shape, seed)
    case = {"shape": shape, "x": rng.uniform(0, 1, (b, c, p)).astype(np.float32)}
    for k, (r, hd, o) in enumerate(heads):
        for name, dims, fan in (("conv_w", (r, c), c), ("conv_b", (r,), c), ("fc1_w", (hd, r * p), r * p), ("fc1_b", (hd,), r * p),
                                ("fc2_w", (o, hd), hd), ("fc2_b", (o,), hd)):
            case[f"{name}{k}"] = rng.uniform(-1, 1, dims).astype(np.float32) / np.float32(np.sqrt(fan))
        case[f"fc1_w{k}"] *= np.float32(4)           # pre-activations of order 1 on both sides of zero
        case[f"dlogits{k}"] = (rng.standard_normal((b, o)) * dlogits_scale).astype(np.float32)
    return case


def integer_case(shape, seed):
    """Integers in [-1, 1] everywhere but fc1's bias, which is 1 + the largest |fc1 sum| of its unit over the batch: every fc1
    pre-activation is a positive integer, ELU is the identity, and every sum is exact in float32 (integer_bound checks)."""
    b, c, p, heads = shape
    rng = _rng(shape, seed)
    ints = lambda dims: rng.randint(-1, 2, dims).astype(np.float32)
    case = {"shape": shape, "x": ints((b, c, p))}
    for k, (r, hd, o) in enumerate(heads):
        case[f"conv_w{k}"], case[f"conv_b{k}"] = ints((r, c)), ints((r,))
        case[f"fc1_w{k}"], case[f"fc2_w{k}"], case[f"fc2_b{k}"] = ints((hd, r * p)), ints((o, hd)), ints((o,))
        case[f"dlogits{k}"] = ints((b, o))
        flat = (np.einsum("rc,bcp->brp", case[f"conv_w{k}"], case["x"]) + case[f"conv_b{k}"][None, :, None]).reshape(b, r * p)
        case[f"fc1_b{k}"] = (1 + np.abs(flat @ case[f"fc1_w{k}"].T).max(axis=0)).astype(np.float32)
    return case


def directed_case():
    """fc1 pre-activations at exactly -20, -1, -1e-4, 0 (from a bias of -0.0), 0, 1e-4 in every sample: the convolution is
    zero, so the flattened output is zero and a pre-activation is its bias (a sum that starts at +0 cannot end at -0: the
    bias -0.0 arrives as +0; the tests that feed `pre` to the backward launch directly put the -0.0 back)."""
    shape = (5, 4, 9, ((3, 6, 5), (2, 6, 4)))
    case = normal_case(shape, seed=77, dlogits_scale=1.0)
    for k in range(2):
        case[f"conv_w{k}"][:] = 0
        case[f"conv_b{k}"][:] = 0
        case[f"fc1_b{k}"] = np.array(DIRECTED_PRE, dtype=np.float32)
    return case


DIRECTED_PRE = (-20.0, -1.0, -1e-4, -0.0, 0.0, 1e-4)


def run64(case, defect=None, pre=None):
    """The rule in float64.  `pre`: {k: [B, Hd]} replaces the fc1 pre-activations the backward reads.  Besides the outputs:
    "h{k}", and the absolute-value sums ulp_bounds works with."""
    b, c, p, heads = case["shape"]
    x = case["x"].astype(np.float64)
    out = {"dx": np.zeros((b, c, p))}
    for k, (r, hd, o) in enumerate(heads):
        cw, cb, w1, b1, w2, b2, dl = (case[f"{n}{k}"].astype(np.float64) for n in PARAMS + ("dlogits",))
        conv = np.einsum("rc,bcp->brp", cw, x) + cb[None, :, None]
        flat = (conv.transpose(0, 2, 1) if defect == "flatten_position_major" else conv).reshape(b, r * p)
        a = flat @ w1.T + b1
        a_back = a if pre is None else pre[k].astype(np.float64)
        h = np.where(a_back > 0, a_back, np.expm1(np.minimum(a_back, 0)))
        logits = np.where(a > 0, a, np.expm1(np.minimum(a, 0))) @ w2.T + b2
        slope = np.ones_like(a_back) if defect == "elu_slope_one" else np.where(a_back > 0, 1.0, np.exp(np.minimum(a_back, 0)))
        dpre = (dl @ w2) * slope
        dflat = dpre @ w1
        dconv = dflat.reshape(b, r, p)
        if not (defect == "dx_without_second_head" and k == 1):
            out["dx"] += np.einsum("rc,brp->bcp", cw, dconv)
        dfc1_w = dpre.T @ flat
        if defect == "fc1_gradient_transposed":
            dfc1_w = (flat.T @ dpre).reshape(hd, r * p)
        got = {"logits": logits, "flat": flat, "pre": a, "dpre": dpre, "dflat": dflat,
               "dconv_w": np.einsum("brp,bcp->rc", dconv, x),
               "dconv_b": dconv[:, :, 0].sum(axis=0) if defect == "conv_bias_without_positions" else dconv.sum(axis=(0, 2)),
               "dfc1_w": dfc1_w, "dfc1_b": dpre.sum(axis=0), "dfc2_w": dl.T @ h, "dfc2_b": dl.sum(axis=0), "h": h}
        m_dflat = np.abs(dpre) @ np.abs(w1)
        got.update({"abs_logits": np.abs(h) @ np.abs(w2).T + np.abs(b2), "abs_dflat": m_dflat,
                    "abs_dfc2_w": np.abs(dl).T @ np.abs(h), "abs_dfc1_w": np.abs(dpre).T @ np.abs(flat),
                    "abs_dfc1_b": np.abs(dpre).sum(axis=0),
                    "abs_dconv_w": np.einsum("brp,bcp->rc", m_dflat.reshape(b, r, p), np.abs(x)),
                    "abs_dconv_b": m_dflat.reshape(b, r, p).sum(axis=(0, 2)),
                    "abs_dx": np.einsum("rc,brp->bcp", np.abs(cw), m_dflat.reshape(b, r, p))})
        out.update({f"{name}{k}": value for name, value in got.items()})
    out["abs_dx"] = sum(out.pop(f"abs_dx{k}") for k in range(len(heads)))
    return out


def outputs(shape, with_intermediates=True):
    names = [f"{n}{k}" for k in range(len(shape[3])) for n in PER_HEAD] + ["dx"]
    return names if with_intermediates else [n for n in names if not n.startswith(("flat", "pre", "dpre", "dflat"))]


def ulp_bounds(case, exact):
    """Per output, the largest |host entry - device| that csrc/head_train.h allows when pre-activations are negative: the ELU
    output h and its derivative each carry a relative difference of rho = ELU_ULPS * 2^-23; a float32 chain of n terms that
    reads differing inputs may also round differently at every step, u = 2^-24 of the absolute-value sum each; the float64
    reductions round once (2 u with the conversion of their inputs' differences).  flat, pre and dfc2_b see no ELU: 0."""
    b, c, p, heads = case["shape"]
    rho = ELU_ULPS * 2.0 ** -23
    total_r = sum(h[0] for h in heads)
    tol = {}
    for k, (r, hd, o) in enumerate(heads):
        g = lambda name: exact[f"{name}{k}"]
        rho_dpre = rho + U
        rho_dflat = rho_dpre + (hd + 1) * U
        tol[f"flat{k}"], tol[f"pre{k}"], tol[f"dfc2_b{k}"] = 0.0 * g("flat"), 0.0 * g("pre"), 0.0 * g("dfc2_b")
        tol[f"logits{k}"] = (rho + (hd + 1) * U) * g("abs_logits")
        tol[f"dpre{k}"] = rho_dpre * np.abs(g("dpre"))
        tol[f"dflat{k}"] = rho_dflat * g("abs_dflat")
        tol[f"dfc2_w{k}"] = (rho + 2 * U) * g("abs_dfc2_w")
        tol[f"dfc1_w{k}"] = (rho_dpre + 2 * U) * g("abs_dfc1_w")
        tol[f"dfc1_b{k}"] = (rho_dpre + 2 * U) * g("abs_dfc1_b")
        tol[f"dconv_w{k}"] = (rho_dflat + 2 * U) * g("abs_dconv_w")
        tol[f"dconv_b{k}"] = (rho_dflat + 2 * U) * g("abs_dconv_b")
    tol["dx"] = (rho + U + (max(h[1] for h in heads) + 1) * U + (total_r + 1) * U) * exact["abs_dx"]
    return tol


def integer_bound(case):
    """The largest sum of absolute values of the terms of any sum the launches form on `case` (an upper bound of every partial
    sum in any order), from the float64 restatement."""
    b, c, p, heads = case["shape"]
    exact = run64(case)
    x = np.abs(case["x"].astype(np.float64))
    worst = 0.0
    for k, (r, hd, o) in enumerate(heads):
        cw, cb, w1, b1, w2, b2, dl = (np.abs(case[f"{n}{k}"].astype(np.float64)) for n in PARAMS + ("dlogits",))
        flat_abs = (np.einsum("rc,bcp->brp", cw, x) + cb[None, :, None]).reshape(b, r * p)
        pre_abs = np.abs(exact[f"flat{k}"]) @ w1.T + b1
        dh_abs = dl @ w2
        worst = max(worst, flat_abs.max(), pre_abs.max(), dh_abs.max(),
                    *(exact[f"abs_{n}{k}"].max() for n in ("logits", "dflat", "dfc2_w", "dfc1_w", "dfc1_b", "dconv_w", "dconv_b")),
                    dl.sum(axis=0).max())
    return max(worst, exact["abs_dx"].max())


def run_torch(case, dtype, device="cpu"):
    """torch's own expression -- the 1 x 1 convolution as models.PointwiseConv2d evaluates it (one addmm over the (sample,
    position) rows), reshape, Linear, ELU, Linear -- with autograd, in `dtype` on `device`: the library of the rule (float32)
    and the check of the yardstick (float64).  Everything comes back as float64 numpy."""
    import torch
    b, c, p, heads = case["shape"]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)
    x = to(case["x"]).requires_grad_()
    kept, loss = {}, 0
    for k, (r, hd, o) in enumerate(heads):
        t = {n: to(case[f"{n}{k}"]).requires_grad_() for n in PARAMS}
        rows = x.view(b, c, p, 1).permute(0, 2, 3, 1).reshape(b * p, c)
        conv = torch.addmm(t["conv_b"], rows, t["conv_w"].t()).view(b, p, 1, r).permute(0, 3, 1, 2)
        flat = conv.reshape(-1, r * p)
        pre = torch.nn.functional.linear(flat, t["fc1_w"], t["fc1_b"])
        logits = torch.nn.functional.linear(torch.nn.functional.elu(pre), t["fc2_w"], t["fc2_b"])
        for v in (flat, pre):
            v.retain_grad()
        loss = loss + (logits * to(case[f"dlogits{k}"])).sum()
        kept[k] = (t, flat, pre, logits)
    loss.backward()
    back = lambda v: v.detach().double().cpu().numpy().copy()
    out = {"dx": back(x.grad)}
    for k, (t, flat, pre, logits) in kept.items():
        out.update({f"logits{k}": back(logits), f"flat{k}": back(flat), f"pre{k}": back(pre), f"dpre{k}": back(pre.grad),
                    f"dflat{k}": back(flat.grad)})
        out.update({f"d{n}{k}": back(t[n].grad) for n in PARAMS})
    return out


# ---- the entries of include/mztrain.h ------------------------------------------------------------------------------------------
def head_descs(native, shape, address):
    """mzmcts_head_desc per head from address(name) (host or device)."""
    b, c, p, heads = shape
    return [native.MzHeadDesc(*[address(f"{n}{k}") for n in PARAMS], c, p, r, hd, o) for k, (r, hd, o) in enumerate(heads)]


def forward_args(native, shape, address):
    args = native.MzTrainHeadsForwardArgs(x=address("x"), batch=shape[0], n_heads=len(shape[3]))
    for k, desc in enumerate(head_descs(native, shape, address)):
        args.heads[k] = desc
        args.logits[k], args.flat[k], args.pre[k] = address(f"logits{k}"), address(f"flat{k}"), address(f"pre{k}")
    return args


def backward_args(native, shape, address, want_dx=True, wanted=PARAMS):
    args = native.MzTrainHeadsBackwardArgs(x=address("x"), dx=address("dx") if want_dx else None, batch=shape[0],
                                           n_heads=len(shape[3]))
    for k, desc in enumerate(head_descs(native, shape, address)):
        args.heads[k] = desc
        for name in ("dlogits", "flat", "pre", "dpre", "dflat"):
            getattr(args, name)[k] = address(f"{name}{k}")
        for name in wanted:
            setattr(args.grads[k], name, address(f"d{name}{k}"))
    return args


def output_shapes(shape):
    b, c, p, heads = shape
    dims = {"dx": (b, c, p)}
    for k, (r, hd, o) in enumerate(heads):
        dims.update({f"logits{k}": (b, o), f"flat{k}": (b, r * p), f"pre{k}": (b, hd), f"dpre{k}": (b, hd), f"dflat{k}": (b, r * p),
                     f"dconv_w{k}": (r, c), f"dconv_b{k}": (r,), f"dfc1_w{k}": (hd, r * p), f"dfc1_b{k}": (hd,),
                     f"dfc2_w{k}": (o, hd), f"dfc2_b{k}": (o,)})
    return dims


def run_host_entry(native, case, pre=None):
    """Forward and backward through mztrain_heads_reference_* on host arrays: every output as float32, NaN-filled before the
    call; the inputs are checked to come back unchanged.  `pre`: as run64's."""
    lib = native.load()
    shape = case["shape"]
    arrays = {k: np.ascontiguousarray(v) for k, v in case.items() if k != "shape"}
    kept = {k: v.copy() for k, v in arrays.items()}
    arrays.update({k: np.full(dims, np.nan, dtype=np.float32) for k, dims in output_shapes(shape).items()})
    address = lambda name: arrays[name].ctypes.data
    args = forward_args(native, shape, address)
    rc = lib.mztrain_heads_reference_forward(ctypes.byref(args))
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    if pre is not None:
        for k, value in pre.items():
            arrays[f"pre{k}"][:] = value
    args = backward_args(native, shape, address)
    rc = lib.mztrain_heads_reference_backward(ctypes.byref(args))
    assert rc == 0, (rc, lib.mzmcts_last_error(None))
    for key, value in kept.items():
        assert np.array_equal(arrays[key].view(np.uint32), value.view(np.uint32)), f"{key} was written"
    return {k: arrays[k] for k in output_shapes(shape)}
