"""The float64 yardstick of models.DownsampleCNN's seven layers (reference models.py:278-297) in plain numpy; it owes
nothing to csrc/downsample_cnn.hip or torch:

    conv 12 x 12, stride 4, pad 2 -> ReLU -> max-pool (3, 2) -> conv 5 x 5, pad 2 -> ReLU -> max-pool (3, 2)
    -> adaptive average with torch's windows [floor(i Q / h), ceil((i + 1) Q / h))

A NaN is kept by ReLU and by the maximum, as torch keeps it.  Both convolutions are rows of patches times the weight
matrix in torch's k order (c, ky, kx), so parity_helpers.dot_layer_rounding_bound carries the float32 bound through them
(K = 576 and K = 25 mid; products with the zero padding are not counted: they add an exact zero); ReLU is 1-Lipschitz, a
maximum moves by at most the largest bound in its window, the average by window_mean_rounding_bound.

exact=True is for integer cases: integral data, every sum of magnitudes below 2^24 (so every partial sum of every
order is exact in float32), the 16-term pooling sum included, and windows of 1, 2, 4, 8 or 16 elements (an exact
division).  Frames are [B, 4, 84, 84]; w1 [mid, 4, 12, 12], b1 [mid], w2 [cout, mid, 5, 5], b2 [cout].
"""
import numpy as np

from parity_helpers import dot_layer_rounding_bound, window_mean_rounding_bound


def patches(x, k, stride, pad):
    """[B, C, H, W] -> ([B, oh ow, C k k] rows in (c, ky, kx) order, oh, ow), zero padding."""
    b, c, h, w = x.shape
    padded = np.zeros((b, c, h + 2 * pad, w + 2 * pad), dtype=x.dtype)
    padded[:, :, pad:pad + h, pad:pad + w] = x
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    rows = np.empty((b, oh, ow, c, k, k), dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            rows[:, :, :, :, ky, kx] = padded[:, :, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride].transpose(0, 2, 3, 1)
    return rows.reshape(b, oh * ow, c * k * k), oh, ow


def relu_keep_nan(v):
    return np.where(v < 0, 0.0, v)


def max_pool_3_2(v):
    """[B, C, H, W] -> [B, C, (H - 3) / 2 + 1, ...]; np.maximum hands a NaN on."""
    oh, ow = (v.shape[2] - 3) // 2 + 1, (v.shape[3] - 3) // 2 + 1
    out = None
    for dy in range(3):
        for dx in range(3):
            part = v[:, :, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2]
            out = part if out is None else np.maximum(out, part)
    return out


def windows(q, n):
    """torch's adaptive windows of n outputs over q inputs."""
    return [((i * q) // n, -((-(i + 1) * q) // n)) for i in range(n)]


def _conv(x, e, weight, bias, k, stride, pad):
    rows, oh, ow = patches(x, k, stride, pad)
    e_rows, _, _ = patches(e, k, stride, pad)
    b, n, kk = rows.shape
    cout = weight.shape[0]
    y, e_out = dot_layer_rounding_bound(rows.reshape(b * n, kk), e_rows.reshape(b * n, kk), weight.reshape(cout, kk), bias)
    magnitude = np.abs(rows.reshape(b * n, kk)) @ np.abs(np.asarray(weight, dtype=np.float64).reshape(cout, kk)).T + np.abs(bias)
    shape = lambda a: a.reshape(b, oh, ow, cout).transpose(0, 3, 1, 2)
    return shape(y), shape(e_out), float(np.nanmax(magnitude))


def downsample_features(x, w1, b1, w2, b2, exact=False):
    """The six layers before the average: (pooled maps float64 [B, cout, 4, 4], the bound they carry)."""
    x, w1, b1, w2, b2 = (np.asarray(a, dtype=np.float64) for a in (x, w1, b1, w2, b2))
    with np.errstate(invalid="ignore"):
        c1, e, m1 = _conv(x, np.zeros_like(x), w1, b1, 12, 4, 2)
        p1, e = max_pool_3_2(relu_keep_nan(c1)), max_pool_3_2(e)
        c2, e, m2 = _conv(p1, e, w2, b2, 5, 1, 2)
        p2, e = max_pool_3_2(relu_keep_nan(c2)), max_pool_3_2(e)
    if exact:
        for a in (x, w1, b1, w2, b2):
            assert np.array_equal(a, np.rint(a)), "exact mode is for integer data"
        assert m1 < 2.0 ** 24 and m2 < 2.0 ** 24, f"a partial sum may reach 2^24 ({m1:.0f}, {m2:.0f})"
    return p2, e


def adaptive_average(p2, e, out_h, out_w, exact=False):
    """torch's AdaptiveAvgPool2d on the pooled maps, with window_mean_rounding_bound."""
    q = p2.shape[2]
    out = np.empty(p2.shape[:2] + (out_h, out_w))
    bound = np.empty_like(out)
    sizes = set()
    with np.errstate(invalid="ignore"):
        for i, (y0, y1) in enumerate(windows(q, out_h)):
            for j, (x0, x1) in enumerate(windows(q, out_w)):
                values = p2[:, :, y0:y1, x0:x1].reshape(p2.shape[:2] + (-1,))
                sizes.add(values.shape[-1])
                out[:, :, i, j] = values.mean(axis=-1)
                bound[:, :, i, j] = window_mean_rounding_bound(values, e[:, :, y0:y1, x0:x1].reshape(values.shape))
                if exact:
                    assert float(np.abs(values).sum(axis=-1).max()) < 2.0 ** 24, "a pooling sum may reach 2^24"
    if exact:
        assert q == 4 and sizes <= {1, 2, 4, 8, 16}, sizes
        bound = np.zeros_like(out)
    return out, bound


def downsample_reference(x, w1, b1, w2, b2, out_h, out_w, exact=False):
    """(out float64 [B, cout, out_h, out_w], bound of the same shape).  The bound of an output that a NaN reaches is
    meaningless; such outputs are judged on the NaN pattern."""
    p2, e = downsample_features(x, w1, b1, w2, b2, exact=exact)
    return adaptive_average(p2, e, out_h, out_w, exact=exact)
