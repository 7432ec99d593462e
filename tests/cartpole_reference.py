"""The yardstick for CartPole's step (csrc/env_kernels.hip, games/cartpole.py), written from the published classic-control
equations (Barto, Sutton & Anderson 1983; Euler integration):

    temp      = (force + m_p l theta_dot^2 sin theta) / (m_c + m_p)
    theta_acc = (g sin theta - cos theta temp) / (l (4/3 - m_p cos^2 theta / (m_c + m_p)))
    x_acc     = temp - m_p l theta_acc cos theta / (m_c + m_p)
    x' = x + tau x_dot,  x_dot' = x_dot + tau x_acc,  theta' = theta + tau theta_dot,  theta_dot' = theta_dot + tau theta_acc
    the pole has fallen when |x'| > 2.4 or |theta'| > 12 degrees; a game lasts 500 plies at most

Three statements of that step:

    step_f64    numpy float64, one numpy operation per arithmetic operation, sin and cos handed in.  Every operation is
                one correctly rounded IEEE + - * /, so with the device's own sin / cos the device's next state must equal
                this one BIT FOR BIT.
    step_exact  the same step in mpmath at 256 bits with mpmath's own sin and cos: the equations themselves.
    step_bound  a running error bound per component for step_f64 against step_exact, when sin and cos are within L ulps.

Every number a test rests on is derived here or has its measurement written beside it.
"""
import math

import mpmath
import numpy as np

GRAVITY = 9.8
MASS_POLE = 0.1
HALF_LENGTH = 0.5
FORCE_MAG = 10.0
TAU = 0.02
TOTAL_MASS = 1.0 + 0.1                  # the Python doubles, rounded as written: step_exact takes them as given
POLE_ML = 0.1 * 0.5
FOUR_THIRDS = 4.0 / 3.0
THETA_LIMIT = 12 * 2 * math.pi / 360
X_LIMIT = 2.4
MAX_STEPS = 500

U = 2.0 ** -53                          # unit roundoff of float64: |fl(r) - r| <= U |fl(r)| for a normal result
TINY = 2.0 ** -1074                     # ... and at most half of this for a subnormal one (charged in full)
EXACT_BITS = 256

# The device library's fp64 sin and cos, as env_step_one calls them, against numpy.longdouble (64-bit mantissa, itself
# within 2^-11 double ulps of the truth) on 2^20 seeded doubles |theta| <= 0.5 plus the edge thetas of cartpole_cases:
# MEASURED on an MI355X (tests/test_gpu_cartpole.py::test_device_sin_cos_within_l_ulps prints it): worst distance from
# the true value sin 0.5972 ulps (at theta = -0.4948988888260628), cos 0.5605 ulps (at theta = -0.43755126657263854),
# "ulps" = spacing of the doubles at the true value (0.5 is the best any double can promise).  Of the 1048595 arguments
# 10922 sines and 14421 cosines differ from glibc's bits, which is why the host plugin cannot be the device's yardstick.
# L is the worst value rounded up to the next integer.
SINCOS_ULPS_L = 1


def step_f64(state, action, sin_t, cos_t):
    """state f64 [N, 4] (x, x_dot, theta, theta_dot), action int [N] (1 pushes right, anything else left), sin_t / cos_t
    f64 [N].  Returns (next state f64 [N, 4], done_own bool [N]); done_own is the game's own "fallen" rule, without the
    500-ply cap (done_after adds it)."""
    state = np.asarray(state, np.float64)
    sin_t, cos_t = np.asarray(sin_t, np.float64), np.asarray(cos_t, np.float64)
    x, x_dot, theta, theta_dot = state[:, 0], state[:, 1], state[:, 2], state[:, 3]
    with np.errstate(all="ignore"):
        force = np.where(np.asarray(action) == 1, FORCE_MAG, -FORCE_MAG)
        td2 = theta_dot * theta_dot
        centrifugal = POLE_ML * td2
        centrifugal = centrifugal * sin_t
        pushed = force + centrifugal
        temp = pushed / TOTAL_MASS
        weight = GRAVITY * sin_t
        reaction = cos_t * temp
        numerator = weight - reaction
        cos2 = cos_t * cos_t
        inertia = MASS_POLE * cos2
        inertia = inertia / TOTAL_MASS
        inertia = FOUR_THIRDS - inertia
        denominator = HALF_LENGTH * inertia
        theta_acc = numerator / denominator
        back = POLE_ML * theta_acc
        back = back * cos_t
        back = back / TOTAL_MASS
        x_acc = temp - back
        dx = TAU * x_dot
        dx_dot = TAU * x_acc
        dtheta = TAU * theta_dot
        dtheta_dot = TAU * theta_acc
        nxt = np.stack([x + dx, x_dot + dx_dot, theta + dtheta, theta_dot + dtheta_dot], axis=1)
        done_own = (np.abs(nxt[:, 0]) > X_LIMIT) | (np.abs(nxt[:, 2]) > THETA_LIMIT)      # (a NaN compares false)
    return nxt, done_own


def done_after(done_own, steps_after, max_moves=0):
    """The done flag of a ply that brought the counter to steps_after: fallen, or the 500th ply, or the move limit."""
    steps_after = np.asarray(steps_after)
    done = np.asarray(done_own, bool) | (steps_after >= MAX_STEPS)
    if max_moves > 0:
        done = done | (steps_after >= max_moves)
    return done


def host_sin_cos(theta):
    """math.sin / math.cos (the host plugin's calls) of every theta."""
    theta = np.asarray(theta, np.float64)
    return (np.array([math.sin(t) for t in theta], np.float64), np.array([math.cos(t) for t in theta], np.float64))


def step_exact(state, action):
    """The equations in mpmath at EXACT_BITS bits: a list of N rows of four mpf.  Finite states only."""
    rows = []
    with mpmath.workprec(EXACT_BITS):
        m = mpmath.mpf
        total_mass, pole_ml, four_thirds = m(TOTAL_MASS), m(POLE_ML), m(FOUR_THIRDS)
        gravity, mass_pole, half_length, tau = m(GRAVITY), m(MASS_POLE), m(HALF_LENGTH), m(TAU)
        for (x, x_dot, theta, theta_dot), a in zip(np.asarray(state, np.float64).tolist(), np.asarray(action).tolist()):
            x, x_dot, theta, theta_dot = m(x), m(x_dot), m(theta), m(theta_dot)
            force = m(FORCE_MAG) if a == 1 else -m(FORCE_MAG)
            sin_t, cos_t = mpmath.sin(theta), mpmath.cos(theta)
            temp = (force + pole_ml * theta_dot * theta_dot * sin_t) / total_mass
            theta_acc = (gravity * sin_t - cos_t * temp) / (half_length * (four_thirds - mass_pole * cos_t * cos_t / total_mass))
            x_acc = temp - pole_ml * theta_acc * cos_t / total_mass
            rows.append([x + tau * x_dot, x_dot + tau * x_acc, theta + tau * theta_dot, theta_dot + tau * theta_acc])
    return rows


class _Run:
    """A float64 value per state with a bound on its distance from the exact value (running error analysis)."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def _of(other):
        return other if isinstance(other, _Run) else _Run(other)

    def _rounded(self, v, e):
        return _Run(v, e + U * np.abs(v) + TINY)          # every operation adds 2^-53 |result| (one rounding)

    def __add__(self, other):
        other = self._of(other)
        return self._rounded(self.v + other.v, self.e + other.e)

    def __sub__(self, other):
        other = self._of(other)
        return self._rounded(self.v - other.v, self.e + other.e)

    def __mul__(self, other):
        other = self._of(other)
        return self._rounded(self.v * other.v, np.abs(self.v) * other.e + np.abs(other.v) * self.e + self.e * other.e)

    def __truediv__(self, other):
        other = self._of(other)                             # |n/d - n'/d'| <= (e_n + |q| e_d) / (|d| - e_d), q = n/d
        q = self.v / other.v
        return self._rounded(q, (self.e + np.abs(q) * other.e) / (np.abs(other.v) - other.e))


def step_bound(state, action, L, sin_t=None, cos_t=None):
    """Per component, a bound on |step_f64(state, action, sin_t, cos_t) - step_exact(state, action)| when sin_t and cos_t
    are within L ulps of the true values (default: numpy's own).  f64 [N, 4].  The magnitudes are those of the float64
    computation, so the bound is first order in 2^-53 with the second-order terms carried along (e_a e_b, |d| - e_d)."""
    state = np.asarray(state, np.float64)
    x, x_dot, theta, theta_dot = (_Run(state[:, i]) for i in range(4))
    sin_v = np.sin(state[:, 2]) if sin_t is None else np.asarray(sin_t, np.float64)
    cos_v = np.cos(state[:, 2]) if cos_t is None else np.asarray(cos_t, np.float64)
    with np.errstate(all="ignore"):
        sin_r = _Run(sin_v, L * U * np.abs(sin_v) + TINY)   # the library calls add L 2^-53 |result|
        cos_r = _Run(cos_v, L * U * np.abs(cos_v))
        force = _Run(np.where(np.asarray(action) == 1, FORCE_MAG, -FORCE_MAG))
        temp = (force + _Run(POLE_ML) * (theta_dot * theta_dot) * sin_r) / TOTAL_MASS
        theta_acc = (_Run(GRAVITY) * sin_r - cos_r * temp) / (_Run(HALF_LENGTH) * (_Run(FOUR_THIRDS) - _Run(MASS_POLE) * (cos_r * cos_r) / TOTAL_MASS))
        x_acc = temp - _Run(POLE_ML) * theta_acc * cos_r / TOTAL_MASS
        tau = _Run(TAU)
        out = [x + tau * x_dot, x_dot + tau * x_acc, theta + tau * theta_dot, theta_dot + tau * theta_acc]
    return np.stack([r.e for r in out], axis=1)


def error_over_bound(got, exact, bound):
    """max over states and components of |got - exact| / bound, with the (row, component) where it is attained.
    got f64 [N, 4], exact from step_exact, bound from step_bound.  The subtraction is done in mpmath."""
    worst, where = 0.0, None
    got, bound = np.asarray(got, np.float64), np.asarray(bound, np.float64)
    with mpmath.workprec(EXACT_BITS):
        for n, row in enumerate(exact):
            for i in range(4):
                err = abs(mpmath.mpf(float(got[n, i])) - row[i])
                ratio = float(err / mpmath.mpf(float(bound[n, i]))) if bound[n, i] > 0 else (0.0 if err == 0 else math.inf)
                if not ratio <= worst:
                    worst, where = ratio, (n, i)
    return worst, where


def reset_states(seed, k):
    """The state after the k-th reset (k = 0: the first) of Game(seed): draws 4k .. 4k + 3 of
    numpy.random.RandomState(seed).uniform(-0.05, 0.05, size=4), taken from numpy itself."""
    rs = np.random.RandomState(int(seed))
    for _ in range(k):
        rs.uniform(-0.05, 0.05, size=4)
    return rs.uniform(-0.05, 0.05, size=4)


def reset_table(seeds, count):
    """reset_states(seed, k) for every seed and k < count: f64 [len(seeds), count, 4]."""
    out = np.empty((len(seeds), count, 4), np.float64)
    for i, seed in enumerate(seeds):
        rs = np.random.RandomState(int(seed))
        for k in range(count):
            out[i, k] = rs.uniform(-0.05, 0.05, size=4)
    return out


def same_bits(a, b):
    """Elementwise: equal as uint64 views, or both NaN (a NaN's sign and payload are not part of the contract)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def ulps_from(got, true_ld):
    """|got - true| in spacings of the doubles at the true value; true_ld is numpy.longdouble.  f64 array."""
    assert np.finfo(np.longdouble).nmant >= 63
    got_ld = np.asarray(got, np.float64).astype(np.longdouble)
    nearest = true_ld.astype(np.float64)
    spacing = np.spacing(np.abs(nearest)).astype(np.longdouble)
    return (np.abs(got_ld - true_ld) / spacing).astype(np.float64)
