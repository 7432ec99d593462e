"""Adam and SGD in float64 numpy, restated from their formulas (Kingma & Ba's Algorithm 1 with L2 weight decay added to the
gradient; SGD with a momentum buffer, no dampening, no Nesterov): the yardstick the flat-buffer optimizer
(csrc/fc_optimizer.h, include/mztrain.h mztrain_opt_*) is held to.  `defect` names a deliberate mistake, so that the tests
can show which tensor each one pushes past their bound."""
import ctypes

import numpy as np

U = 2.0 ** -24
SIZES = (1, 3, 4, 5, 255, 256, 257, 1748, 70001)
STEPS = 5
KINDS = {"adam": dict(kind="Adam"), "sgd-m0": dict(kind="SGD", momentum=0.0), "sgd-m0.9": dict(kind="SGD", momentum=0.9)}
DECAYS = (0.0, 1e-4)
DEFECTS = ("no_weight_decay", "t_off_by_one", "bc2s_left_out")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def learning_rates(steps=STEPS, lr0=0.02, rate=0.8, decay_steps=2):
    """A learning rate that changes every step, as Trainer.update_lr's decay does."""
    return [lr0 * rate ** (k / decay_steps) for k in range(steps)]


def make_case(n, steps=STEPS, seed=0):
    """float32 weights, and per step a float32 gradient spread over six decades with exact zeros and a few 1e-30."""
    rng = np.random.RandomState(1000 * seed + n % 997)
    weights = (rng.standard_normal(n) * 0.5).astype(np.float32)
    grads = []
    for _ in range(steps):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)
        g[rng.random_sample(n) < 0.1] = 0.0
        g[rng.random_sample(n) < 0.03] = 1e-30
        grads.append(g.astype(np.float32))
    return weights, grads


def run64(kind, weights, grads, lrs, weight_decay=0.0, momentum=0.0, beta1=BETA1, beta2=BETA2, eps=EPS, defect=None):
    """The steps in float64.  Returns {"weights", "moment1", "moment2"} (moment2 only for Adam; SGD's moment1 is its
    momentum buffer, zeros for momentum 0)."""
    w = np.asarray(weights, dtype=np.float64).copy()
    m = np.zeros_like(w)
    v = np.zeros_like(w)
    for index, (g, lr) in enumerate(zip(grads, lrs)):
        t = index + 1
        g = np.asarray(g, dtype=np.float64)
        if weight_decay != 0.0 and defect != "no_weight_decay":
            g = g + weight_decay * w
        if kind == "Adam":
            if defect == "t_off_by_one":
                t += 1
            m = beta1 * m + (1.0 - beta1) * g
            v = beta2 * v + (1.0 - beta2) * g * g
            m_hat = m / (1.0 - beta1 ** t)
            v_hat = v if defect == "bc2s_left_out" else v / (1.0 - beta2 ** t)
            w = w - lr * m_hat / (np.sqrt(v_hat) + eps)
        else:
            if momentum != 0.0:
                m = momentum * m + g
                g = m
            w = w - lr * g
    out = {"weights": w, "moment1": m}
    if kind == "Adam":
        out["moment2"] = v
    return out


def ratio(native_value, library_value, exact):
    """The project's rule for a training step: native error / (4 max(library error, 4 u max|exact|));
    0 / 0 = 0."""
    exact = np.asarray(exact, dtype=np.float64)
    scale = float(np.abs(exact).max())
    native_error = float(np.abs(np.asarray(native_value, dtype=np.float64) - exact).max())
    library_error = float(np.abs(np.asarray(library_value, dtype=np.float64) - exact).max())
    allowed = 4.0 * max(library_error, 4.0 * U * scale)
    value = native_error / allowed if allowed > 0 else (0.0 if native_error == 0 else float("inf"))
    return value, {"native": native_error, "library": library_error, "max_abs": scale, "ratio": value}


def run_torch(kind, weights, grads, lrs, dtype, weight_decay=0.0, momentum=0.0):
    """torch.optim on the CPU in `dtype`: the library of the rule (float32) and the check of the yardstick (float64)."""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(weights)).to(dtype).clone())
    if kind == "Adam":
        opt = torch.optim.Adam([p], lr=lrs[0], betas=(BETA1, BETA2), eps=EPS, weight_decay=weight_decay)
    else:
        opt = torch.optim.SGD([p], lr=lrs[0], momentum=momentum, weight_decay=weight_decay)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = torch.from_numpy(np.asarray(g)).to(dtype).clone()
        opt.step()
    state = opt.state[p]
    zeros = np.zeros(p.numel())
    out = {"weights": p.detach().double().numpy().copy()}
    if kind == "Adam":
        out["moment1"] = state["exp_avg"].double().numpy().copy()
        out["moment2"] = state["exp_avg_sq"].double().numpy().copy()
    else:
        buf = state.get("momentum_buffer")
        out["moment1"] = buf.double().numpy().copy() if buf is not None else zeros
    return out


def opt_args(native, kind, n, weights, grads, moment1, moment2, lr, steps_done, weight_decay=0.0, momentum=0.0,
             beta1=BETA1, beta2=BETA2, eps=EPS):
    """mztrain_opt_args from raw addresses (host or device; None stays a null pointer)."""
    return native.MzTrainOptArgs(kind=native.OPT_ADAM if kind == "Adam" else native.OPT_SGD, n=n, weights=weights, grads=grads,
                                 moment1=moment1, moment2=moment2, lr=lr, steps_done=steps_done, beta1=beta1, beta2=beta2,
                                 eps=eps, weight_decay=weight_decay, momentum=momentum)


def run_host_entry(native, kind, weights, grads, lrs, weight_decay=0.0, momentum=0.0, start=0):
    """The steps through mztrain_opt_reference on host arrays (float32).  Returns the tensors as float32 arrays plus
    "steps_done"; the gradient arrays are checked to come back unchanged."""
    lib = native.load()
    n = len(weights)
    w = np.ascontiguousarray(weights, dtype=np.float32).copy()
    adam = kind == "Adam"
    m = np.zeros(n, dtype=np.float32) if adam or momentum != 0.0 else None
    v = np.zeros(n, dtype=np.float32) if adam else None
    lr = np.zeros(1, dtype=np.float64)
    done = np.full(1, start, dtype=np.int64)
    address = lambda a: a.ctypes.data if a is not None else None
    for g, rate in zip(grads, lrs):
        g = np.ascontiguousarray(g, dtype=np.float32)
        kept = g.copy()
        lr[0] = rate
        args = opt_args(native, kind, n, address(w), address(g), address(m), address(v), address(lr), address(done),
                        weight_decay=weight_decay, momentum=momentum)
        rc = lib.mztrain_opt_reference(ctypes.byref(args))
        assert rc == 0, (rc, lib.mzmcts_last_error(None))
        assert np.array_equal(g.view(np.uint32), kept.view(np.uint32)), "the gradient was written"
    out = {"weights": w, "moment1": m if m is not None else np.zeros(n, dtype=np.float32), "steps_done": int(done[0])}
    if adam:
        out["moment2"] = v
    return out
