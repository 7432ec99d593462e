"""The states CartPole's step is judged on, shared by tests/test_cartpole_reference.py (CPU) and
tests/test_gpu_cartpole.py (device).  Every set is (name, state f64 [N, 4], action int32 [N]); the order of a state is
x, x_dot, theta, theta_dot."""
import numpy as np

from cartpole_reference import THETA_LIMIT, X_LIMIT

SWEEP = 4096                             # states per launch of the device sweep


def interior(n=SWEEP, seed=20240):
    """Seeded states over everything a game can reach and a little beyond: |x| <= 2.6, |x_dot| <= 4, |theta| <= 0.25,
    |theta_dot| <= 5; one state in seven scaled down by up to 1e-8 (the neighbourhood of the upright rest, where the
    terms of the equations differ most in size).  Actions alternate."""
    rs = np.random.RandomState(seed)
    state = rs.uniform(-1.0, 1.0, size=(n, 4)) * np.array([2.6, 4.0, 0.25, 5.0])
    scale = 10.0 ** -rs.uniform(0.0, 8.0, size=n)
    small = np.arange(n) % 7 == 3
    state[small] *= scale[small, None]
    return state, (np.arange(n) & 1).astype(np.int32)


def _both_actions(rows):
    state = np.array(rows, np.float64).reshape(-1, 4)
    return np.concatenate([state, state]), np.concatenate([np.zeros(len(state), np.int32), np.ones(len(state), np.int32)])


def theta_limit_states():
    """theta_dot = 0, so theta' = theta exactly: theta on +-limit (not fallen: the rule is >) and on both neighbours
    (the next double beyond has fallen).  Returns (state, action, fallen)."""
    rows, fallen = [], []
    for sign in (1.0, -1.0):
        for theta, f in ((THETA_LIMIT, False), (np.nextafter(THETA_LIMIT, 1.0), True), (np.nextafter(THETA_LIMIT, 0.0), False)):
            rows.append([0.01, 0.0, sign * theta, 0.0])
            fallen.append(f)
    state, action = _both_actions(rows)
    return state, action, np.array(fallen + fallen)


def x_limit_states():
    """x_dot = 0, so x' = x + tau * 0 = x exactly: x on +-2.4 (not fallen), the next double beyond (fallen) and the one
    before (not fallen).  Returns (state, action, fallen)."""
    rows, fallen = [], []
    for sign in (1.0, -1.0):
        for x, f in ((X_LIMIT, False), (np.nextafter(X_LIMIT, 3.0), True), (np.nextafter(X_LIMIT, 0.0), False)):
            rows.append([sign * x, 0.0, 0.01, 0.0])
            fallen.append(f)
    state, action = _both_actions(rows)
    return state, action, np.array(fallen + fallen)


def balanced_states(n):
    """States far from both limits: whatever the action, the next state has not fallen."""
    rs = np.random.RandomState(7)
    return rs.uniform(-0.05, 0.05, size=(n, 4))


EDGE_THETAS = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060, -2.0 ** -1060, 2.0 ** -1022, THETA_LIMIT, -THETA_LIMIT,
                        np.nextafter(THETA_LIMIT, 1.0), np.nextafter(THETA_LIMIT, 0.0), 0.25, -0.25, 0.5, -0.5, 2.0 ** -27,
                        2.0 ** -26, 1e-5, 0.1])


def edges():
    """Signed zeros, subnormal thetas, both limits and their neighbours, velocities whose square overflows, and inf / NaN
    in each component; every state with both actions."""
    rows = []
    for bits in range(16):                                   # zeros and signed zeros
        rows.append([-0.0 if bits >> i & 1 else 0.0 for i in range(4)])
    for theta in (5e-324, -5e-324, 2.0 ** -1060, -2.0 ** -1060, 2.0 ** -1022, 3e-310):   # subnormal theta
        for theta_dot in (0.0, 1.0, -5e-324, 2.0 ** -1030):
            rows.append([0.0, 0.0, theta, theta_dot])
            rows.append([1.0, -0.5, theta, theta_dot])
    rows += theta_limit_states()[0][:6].tolist() + x_limit_states()[0][:6].tolist()
    for v in (1e150, -1e150, 1.3e154, 1.35e154, 1e200, -1e300, 1.7e308):   # v * v overflows from 1.35e154 on
        rows.append([0.0, 0.0, 0.1, v])
        rows.append([0.0, v, -0.1, 0.0])
        rows.append([0.5, v, 0.05, -v])
        rows.append([0.0, 0.0, 0.0, v])
    for bad in (np.inf, -np.inf, np.nan):                    # inf and NaN in each component
        for i in range(4):
            row = [0.5, -0.25, 0.03, 0.125]
            row[i] = bad
            rows.append(row)
    rows.append([np.nan] * 4)
    rows.append([np.inf, np.inf, -np.inf, np.inf])
    return _both_actions(rows)


def finite_steps(state, action):
    """Rows of a set whose state is finite and small enough that no operation of the step overflows."""
    state = np.asarray(state, np.float64)
    return np.isfinite(state).all(axis=1) & (np.abs(state) < 1e150).all(axis=1)


def cast_edges():
    """Doubles on and around float32 ties, at 1 and in float32's subnormal range, and doubles beyond float32's range."""
    values = []
    for tie in (1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -127 + 2.0 ** -150, 2.0 ** -127 + 3 * 2.0 ** -150,
                2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5, 2.0 ** -126 - 2.0 ** -150):
        values += [tie, np.nextafter(tie, 0.0), np.nextafter(tie, 2.0)]
    big = float(np.finfo(np.float32).max)
    values += [big, big + 2.0 ** 102, np.nextafter(big + 2.0 ** 102, 0.0), 2.0 ** 128, 1e39, 1e300, np.inf, np.nan, 0.0, 5e-324]
    values = np.array(values, np.float64)
    return np.concatenate([values, -values])
