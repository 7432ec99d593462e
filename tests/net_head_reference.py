"""The float64 yardstick of one reward / value / policy head of the residual networks (reference models.py:467-480,
500-522), in plain numpy: it owes nothing to csrc/net_kernels.hip, csrc/board_conv.hip or torch.

    y[r, p]  = sum_c Wc[r, c] x[c, p] + bc[r]          the 1x1 convolution, flattened as r * P + p
    h        = elu(W1 y + b1)
    logits   = W2 h + b2

head_reference returns the logits with parity_helpers.head_rounding_bound's per-logit bound on a float32 evaluation
(the argument for it is in dot_layer_rounding_bound's docstring).  exact=True is for integer cases: it refuses data that
is not integral, a hidden pre-activation that is not positive (ELU must be the identity) and any sum of magnitudes
sum |w| |x| + |b| of 2^24 or more -- every partial sum of every order is bounded by it, so the float32 result IS the
integer, whatever the kernel's order.  tests/test_net_head_reference.py holds all of this to account on the CPU.

A head's parameters are a dict of float32 arrays: conv_w [R, C], conv_b [R], w1 [Hd, R P], b1 [Hd], w2 [O, Hd], b2 [O];
boards are [B, C, P].
"""
import numpy as np

from parity_helpers import head_rounding_bound

KEYS = ("conv_w", "conv_b", "w1", "b1", "w2", "b2")


def elu64(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))


def head_layers(x, p):
    """(y [B, R P], pre-activations [B, Hd], logits [B, O]) in float64."""
    x = np.asarray(x, dtype=np.float64)
    conv_w, conv_b, w1, b1, w2, b2 = (np.asarray(p[k], dtype=np.float64) for k in KEYS)
    batch = x.shape[0]
    y = np.einsum("rc,bcp->brp", conv_w, x) + conv_b[None, :, None]
    flat = y.reshape(batch, -1)
    pre = flat @ w1.T + b1
    return flat, pre, elu64(pre) @ w2.T + b2


def head_reference(x, p, exact=False):
    """(logits float64 [B, O], bound [B, O]); exact: see the module docstring (the bound is then zero)."""
    flat, pre, logits = head_layers(x, p)
    if exact:
        x64 = np.asarray(x, dtype=np.float64)
        for a in (x64,) + tuple(np.asarray(p[k], dtype=np.float64) for k in KEYS):
            assert np.array_equal(a, np.rint(a)), "exact mode is for integer data"
        assert bool((pre > 0).all()), "exact mode needs every hidden pre-activation positive (ELU = identity)"
        a_w, a_b, a_w1, a_b1, a_w2, a_b2 = (np.abs(np.asarray(p[k], dtype=np.float64)) for k in KEYS)
        m_y = np.einsum("rc,bcp->brp", a_w, np.abs(x64)) + a_b[None, :, None]
        m_pre = np.abs(flat) @ a_w1.T + a_b1
        m_out = np.abs(pre) @ a_w2.T + a_b2
        for name, m in (("1x1 convolution", m_y), ("Linear-1", m_pre), ("Linear-2", m_out)):
            assert float(m.max()) < 2.0 ** 24, f"{name}: a partial sum may reach 2^24 ({m.max():.0f})"
        return logits, np.zeros_like(logits)
    return logits, head_rounding_bound(x, *[p[k] for k in KEYS])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def judge(got, want, bound):
    """(worst error / bound, index of the worst element or of the first element that is not finite).  An element whose
    bound is zero must be equal; one that is not a finite number has ratio inf."""
    got = np.asarray(got, dtype=np.float64)
    error = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, error / bound, np.where(error == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[worst]), tuple(int(i) for i in worst)
