"""A float64 numpy restatement of the training convolutions of include/mztrain.h (mztrain_conv_*): the padded, stride-1
3 x 3 convolution, its data gradient for the input's first `dx_planes` planes and its weight gradient, sliced as
csrc/conv_train.h slices it.  On data whose products and partial sums are exact in float32 (small integers) it gives the
bits of the host entries and of the kernels; on any data it is the float64 answer they are held to.

`defect` switches ONE deliberate mistake on, so that the tests can show each is seen:
    "taps_not_flipped"          the data gradient convolves with the unflipped taps
    "channels_not_transposed"   the data gradient does not swap the weight's two channel axes (needs cin == cout)
    "border_wraps"              a border tap reads the opposite edge instead of a zero
    "fold_in_float32"           the weight gradient adds its slice sums in float32
    "action_plane_in_dx"        the data gradient covers every input plane, the one beyond dx_planes included
"""
import ctypes

import numpy

DEFECTS = ("taps_not_flipped", "channels_not_transposed", "border_wraps", "fold_in_float32", "action_plane_in_dx")

# (B, cin, cout, H, W, dx_planes): the smallest shapes that reach every form.  sb = samples per workgroup of the forward
# plan: 32 (3 x 3, 16), 16 (3 x 3, 64), 16 (6 x 6, 16), 4 (6 x 7, 64); a data gradient of 16 planes under 64 output channels is
# the convolution 64 -> 16, which fits LDS on 6 x 7 boards only; slice edges for MZTRAIN_CONV_SLICE = 64: the largest B
# with B * P <= 64, that + 1, and a B of three slices (B * P in (128, 192]).
SHAPES = [
    # 3 x 3, cout 16 (sb 32; slices: 7 | 8 | 15..21)
    (1, 1, 16, 3, 3, 0), (31, 3, 16, 3, 3, 0), (32, 16, 16, 3, 3, 16), (33, 17, 16, 3, 3, 16),
    (7, 16, 16, 3, 3, 16), (8, 17, 16, 3, 3, 16), (15, 16, 16, 3, 3, 0),
    # 3 x 3, cout 64 (sb 16)
    (1, 3, 64, 3, 3, 0), (15, 64, 64, 3, 3, 64), (16, 65, 64, 3, 3, 64), (17, 80, 64, 3, 3, 64), (7, 64, 64, 3, 3, 64),
    (8, 65, 64, 3, 3, 0), (21, 64, 64, 3, 3, 0),
    # 6 x 6, cout 16 (sb 16; slices: 1 | 2 | 4, 5)
    (1, 1, 16, 6, 6, 0), (15, 3, 16, 6, 6, 0), (16, 16, 16, 6, 6, 16), (17, 17, 16, 6, 6, 16), (2, 16, 16, 6, 6, 16),
    (4, 17, 16, 6, 6, 16),
    # 6 x 7, cout 64 (sb 4; slices: 1 | 2 | 4)
    (1, 3, 64, 6, 7, 0), (3, 64, 64, 6, 7, 64), (4, 65, 64, 6, 7, 64), (5, 80, 64, 6, 7, 64), (2, 64, 64, 6, 7, 16),
]


def patches(x, wrap=False):
    """[B, cin, 9, H, W]: tap (ky, kx) of xpad, zeros (or, the defect, the opposite edge) outside the board."""
    x = numpy.asarray(x, dtype=numpy.float64)
    b, c, h, w = x.shape
    out = numpy.zeros((b, c, 9, h, w))
    if wrap:
        for ky in range(3):
            for kx in range(3):
                out[:, :, ky * 3 + kx] = numpy.roll(x, (1 - ky, 1 - kx), axis=(2, 3))
        return out
    padded = numpy.zeros((b, c, h + 2, w + 2))
    padded[:, :, 1:-1, 1:-1] = x
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky * 3 + kx] = padded[:, :, ky:ky + h, kx:kx + w]
    return out


def forward(x, weight, defect=None):
    """y [B, cout, H, W] in float64."""
    weight = numpy.asarray(weight, dtype=numpy.float64)
    cout, cin = weight.shape[:2]
    return numpy.einsum("nct,bcthw->bnhw", weight.reshape(cout, cin, 9), patches(x, wrap=defect == "border_wraps"))


def virtual_weight(weight, dx_planes, defect=None):
    """w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], ci < dx_planes: the weight the data gradient convolves dy with."""
    weight = numpy.asarray(weight)
    planes = weight.shape[1] if defect == "action_plane_in_dx" else dx_planes
    w = weight if defect == "channels_not_transposed" else weight.transpose(1, 0, 2, 3)
    if defect != "taps_not_flipped":
        w = w[:, :, ::-1, ::-1]
    return numpy.ascontiguousarray(w[:planes])


def dgrad(dy, weight, dx_planes, defect=None):
    """dx [B, dx_planes, H, W] in float64: the gradient of the input's first dx_planes planes."""
    return forward(dy, virtual_weight(weight, dx_planes, defect), defect=defect)


def wgrad(x, dy, slice_length, defect=None):
    """dw [cout, cin, 3, 3]: slice sums over k = b * P + p in float64, folded in ascending order in float64 (or, the
    defect, in float32), rounded to float32 once -- returned as float64 for comparison."""
    dy = numpy.asarray(dy, dtype=numpy.float64)
    b, cout, h, w = dy.shape
    cin = x.shape[1]
    cols = patches(x, wrap=defect == "border_wraps").transpose(0, 3, 4, 1, 2).reshape(b * h * w, cin * 9)
    rows = dy.transpose(0, 2, 3, 1).reshape(b * h * w, cout)
    fold = numpy.float32 if defect == "fold_in_float32" else numpy.float64
    total = numpy.zeros((cout, cin * 9), dtype=fold)
    for k0 in range(0, b * h * w, slice_length):
        part = rows[k0:k0 + slice_length].T @ cols[k0:k0 + slice_length]
        total = (total + part.astype(numpy.float32).astype(fold)).astype(fold)
    return total.astype(numpy.float32).astype(numpy.float64).reshape(cout, cin, 3, 3)


def wgrad_exact(x, dy):
    """dw in float64 with no slicing: the answer on any data."""
    b, cout, h, w = dy.shape
    return numpy.einsum("bnhw,bcthw->nct", numpy.asarray(dy, dtype=numpy.float64), patches(x)).reshape(cout, -1, 3, 3)


def integer_case(shape, seed):
    """(x, w, dy) as float32 arrays of small integers: x in [-3, 3], w and dy in [-2, 2] -- every partial sum is below
    9 * 80 * 6 (forward, data gradient) or B * P * 6 (weight gradient), far below 2^24."""
    b, cin, cout, h, w, _ = shape
    rng = numpy.random.default_rng(seed)
    return (rng.integers(-3, 4, (b, cin, h, w)).astype(numpy.float32),
            rng.integers(-2, 3, (cout, cin, 3, 3)).astype(numpy.float32),
            rng.integers(-2, 3, (b, cout, h, w)).astype(numpy.float32))


def normal_case(shape, seed, x_scale=1.0, w_scale=0.1, dy_scale=1e-3):
    b, cin, cout, h, w, _ = shape
    rng = numpy.random.default_rng(seed)
    return ((rng.standard_normal((b, cin, h, w)) * x_scale).astype(numpy.float32),
            (rng.standard_normal((cout, cin, 3, 3)) * w_scale).astype(numpy.float32),
            (rng.standard_normal((b, cout, h, w)) * dy_scale).astype(numpy.float32))


# ---- the host entries (mztrain_conv_reference_*) on numpy arrays ---------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_forward(native, lib, x, weight):
    b, cin, h, w = x.shape
    x, weight = numpy.ascontiguousarray(x, numpy.float32), numpy.ascontiguousarray(weight, numpy.float32)
    y = numpy.full((b, weight.shape[0], h, w), numpy.nan, dtype=numpy.float32)
    args = native.MzTrainConvForwardArgs(x=_ptr(x), weight=_ptr(weight), y=_ptr(y), batch=b, cin=cin, cout=weight.shape[0],
                                         height=h, width=w)
    native.check_train(lib, lib.mztrain_conv_reference_forward(ctypes.byref(args)), "mztrain_conv_reference_forward")
    return y


def host_dgrad(native, lib, dy, weight, dx_planes):
    b, cout, h, w = dy.shape
    dy, weight = numpy.ascontiguousarray(dy, numpy.float32), numpy.ascontiguousarray(weight, numpy.float32)
    dx = numpy.full((b, dx_planes, h, w), numpy.nan, dtype=numpy.float32)
    args = native.MzTrainConvDgradArgs(dy=_ptr(dy), weight=_ptr(weight), dx=_ptr(dx), batch=b, cin=weight.shape[1], cout=cout,
                                       height=h, width=w, dx_planes=dx_planes)
    native.check_train(lib, lib.mztrain_conv_reference_dgrad(ctypes.byref(args)), "mztrain_conv_reference_dgrad")
    return dx


def host_wgrad(native, lib, x, dy):
    b, cin, h, w = x.shape
    x, dy = numpy.ascontiguousarray(x, numpy.float32), numpy.ascontiguousarray(dy, numpy.float32)
    dw = numpy.full((dy.shape[1], cin, 3, 3), numpy.nan, dtype=numpy.float32)
    args = native.MzTrainConvWgradArgs(x=_ptr(x), dy=_ptr(dy), dw=_ptr(dw), batch=b, cin=cin, cout=dy.shape[1], height=h,
                                       width=w)
    native.check_train(lib, lib.mztrain_conv_reference_wgrad(ctypes.byref(args)), "mztrain_conv_reference_wgrad")
    return dw


def host_pack(native, lib, weight, dx_planes):
    """(forward packing, data-gradient packing or None, affine) of mztrain_conv_reference_pack."""
    weight = numpy.ascontiguousarray(weight, numpy.float32)
    cout, cin = weight.shape[:2]
    packed = numpy.full(lib.mzmcts_board_conv_packed_floats(cin, cout), numpy.nan, dtype=numpy.float32)
    packed_dx = (numpy.full(lib.mzmcts_board_conv_packed_floats(cout, dx_planes), numpy.nan, dtype=numpy.float32)
                 if dx_planes else None)
    affine = numpy.full(2 * native.CONV_AFFINE, numpy.nan, dtype=numpy.float32)
    args = native.MzTrainConvPackArgs(weight=_ptr(weight), packed=_ptr(packed),
                                      packed_dx=_ptr(packed_dx) if dx_planes else None, affine=_ptr(affine), cin=cin,
                                      cout=cout, dx_planes=dx_planes)
    native.check_train(lib, lib.mztrain_conv_reference_pack(ctypes.byref(args)), "mztrain_conv_reference_pack")
    return packed, packed_dx, affine
