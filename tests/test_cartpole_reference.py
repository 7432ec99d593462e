"""CartPole's yardstick (tests/cartpole_reference.py) held to itself on the CPU: the float64 restatement against the
equations in mpmath, against the host plugin bit for bit, against closed forms -- and the case set
(tests/cartpole_cases.py) shown to bite: each one-line defect of a numpy copy of the step breaks a named case."""
import importlib
import math

import mpmath
import numpy as np
import pytest

import cartpole_cases as cases
import cartpole_reference as ref


@pytest.fixture(scope="module")
def plugin(pkg):
    return importlib.import_module("muzero-hypermodel_amd.games.cartpole")


@pytest.fixture(scope="module")
def interior():
    """The seeded interior with the reference's answers, computed once: state, action, step_f64 with the host's sin / cos,
    the exact step and the L = 1 bound (glibc's sin and cos are within one ulp)."""
    state, action = cases.interior()
    sin_t, cos_t = ref.host_sin_cos(state[:, 2])
    nxt, done = ref.step_f64(state, action, sin_t, cos_t)
    return dict(state=state, action=action, sin=sin_t, cos=cos_t, next=nxt, done=done,
                exact=ref.step_exact(state, action), bound=ref.step_bound(state, action, 1, sin_t, cos_t))


def plugin_step(plugin, state, action, steps=0):
    env = plugin.CartPolePhysics(0)
    out, done = np.empty((len(state), 4)), np.empty(len(state), bool)
    for n in range(len(state)):
        env.state, env.steps = np.array(state[n]), steps
        _, reward, done[n] = env.step(int(action[n]))
        assert reward == 1.0
        out[n] = env.state
    return out, done


def test_f64_step_within_bound_of_the_equations(interior):
    worst, where = ref.error_over_bound(interior["next"], interior["exact"], interior["bound"])
    print(f"interior: worst error / bound {worst:.3f} at (state, component) {where}")
    assert worst <= 1.0
    # (the bound is tight, not loose: x + tau * x_dot is two roundings and nearly attains its two half-ulps)
    assert worst > 0.5


def test_f64_step_within_bound_on_the_finite_edges():
    state, action = cases.edges()
    keep = cases.finite_steps(state, action)
    state, action = state[keep], action[keep]
    assert len(state) >= 100
    sin_t, cos_t = ref.host_sin_cos(state[:, 2])
    nxt, _ = ref.step_f64(state, action, sin_t, cos_t)
    worst, where = ref.error_over_bound(nxt, ref.step_exact(state, action), ref.step_bound(state, action, 1, sin_t, cos_t))
    print(f"finite edges: worst error / bound {worst:.3f} at {where}")
    assert worst <= 1.0


def test_host_plugin_equals_f64_step_bit_for_bit(plugin, interior):
    got, done = plugin_step(plugin, interior["state"], interior["action"])
    same = ref.same_bits(got, interior["next"])
    assert same.all(), f"{(~same).sum()} components differ, first at {np.argwhere(~same)[0]}"
    assert np.array_equal(done, interior["done"])
    state, action = cases.edges()
    sin_t, cos_t = ref.host_sin_cos(np.where(np.isfinite(state[:, 2]), state[:, 2], 0.0))
    bad = ~np.isfinite(state[:, 2])                 # (math.sin raises on inf where IEEE answers NaN)
    sin_t[bad], cos_t[bad] = np.nan, np.nan
    keep = ~bad
    with np.errstate(all="ignore"):
        got, done = plugin_step(plugin, state[keep], action[keep])
    want, want_done = ref.step_f64(state[keep], action[keep], sin_t[keep], cos_t[keep])
    same = ref.same_bits(got, want)
    assert same.all(), f"{(~same).sum()} components differ, first at {np.argwhere(~same)[0]}"
    assert np.array_equal(done, want_done)


def test_closed_form_upright_acceleration():
    """At theta = theta_dot = 0: sin = 0 and cos = 1 exactly, so theta_acc = -force / (total_mass * 0.5 * (4/3 - 0.1/1.1))
    in rationals.  theta_dot' = tau * theta_acc.  Beyond the step's own bound the constants' roundings count: total_mass
    = fl(1 + fl(0.1)) is within 2 u, 4/3 within u (weight (4/3) / 1.2424 = 1.07), 0.1 / 1.1 within 3 u (weight 0.07), tau
    = fl(0.02) within u: less than 5 u relative in all."""
    state = np.array([[0.0, 0.0, 0.0, 0.0], [1.5, -2.0, 0.0, 0.0], [-2.0, 3.0, -0.0, 0.0]])
    for a in (0, 1):
        action = np.full(len(state), a)
        sin_t, cos_t = ref.host_sin_cos(state[:, 2])
        nxt, _ = ref.step_f64(state, action, sin_t, cos_t)
        bound = ref.step_bound(state, action, 1, sin_t, cos_t)
        exact = ref.step_exact(state, action)
        with mpmath.workprec(ref.EXACT_BITS):
            r = lambda p, q: mpmath.mpf(p) / mpmath.mpf(q)
            force = mpmath.mpf(10 if a == 1 else -10)
            want = r(1, 50) * -force / (r(11, 10) * r(1, 2) * (r(4, 3) - r(1, 10) / r(11, 10)))
            for n in range(len(state)):
                allowed = mpmath.mpf(float(bound[n, 3])) + 5 * ref.U * abs(want)
                assert abs(mpmath.mpf(float(nxt[n, 3])) - want) <= allowed
                assert abs(exact[n][3] - want) <= 5 * ref.U * abs(want)
                assert nxt[n, 2] == 0.0


def test_step_is_odd_under_reflection(plugin, interior):
    """Mirroring the track -- every component negated and the push reversed -- negates the next state: exactly, in all
    three statements (IEEE operations and glibc's sin / cos are symmetric in sign)."""
    state, action = interior["state"][:512], interior["action"][:512]
    mirrored, _ = ref.step_f64(-state, 1 - action, -interior["sin"][:512], interior["cos"][:512])
    assert (np.ascontiguousarray(-mirrored).view(np.uint64) == np.ascontiguousarray(interior["next"][:512]).view(np.uint64)).all()
    got, _ = plugin_step(plugin, -state, 1 - action)
    assert (np.ascontiguousarray(-got).view(np.uint64) == np.ascontiguousarray(interior["next"][:512]).view(np.uint64)).all()
    for row, back in zip(interior["exact"][:64], ref.step_exact(-state[:64], 1 - action[:64])):
        assert all(a + b == 0 for a, b in zip(row, back))     # (a sum of opposites is exact at any working precision)


def test_reset_states_are_the_plugins(plugin):
    for seed in (0, 1, 2 ** 31, 2 ** 32 - 1):
        game = plugin.Game(seed)
        table = ref.reset_table([seed], 5)[0]
        for k in range(5):
            obs = game.reset()
            assert np.array_equal(game.env.state, ref.reset_states(seed, k)) and np.array_equal(game.env.state, table[k])
            assert np.array_equal(obs[0, 0], table[k].astype(np.float32))


# ---- the case set bites ------------------------------------------------------------------------------------------------
def copy_step(state, action, steps, defect=None):
    """A numpy copy of the step with one line changed per defect; returns (next state, done)."""
    x, x_dot, theta, theta_dot = (np.array(state[:, i]) for i in range(4))
    tau = 0.2 if defect == "tau 0.2" else 0.02
    force = np.where(action == 1, 10.0, -10.0)
    if defect == "force sign":
        force = -force
    total_mass = 1.0 + 0.1
    pole_ml = 0.1 * (1.0 if defect == "full length in pole_ml" else 0.5)
    sin_t, cos_t = ref.host_sin_cos(theta)
    td2 = theta_dot if defect == "theta_dot not squared" else theta_dot * theta_dot
    temp = (force + pole_ml * td2 * sin_t) / total_mass
    cos2 = 1.0 if defect == "no cos^2" else cos_t * cos_t
    four_thirds = 1.33 if defect == "4/3 as 1.33" else 4.0 / 3.0
    theta_acc = (9.8 * sin_t - cos_t * temp) / (0.5 * (four_thirds - 0.1 * cos2 / total_mass))
    x_acc = temp - pole_ml * theta_acc * cos_t / total_mass
    new_x_dot, new_theta_dot = x_dot + tau * x_acc, theta_dot + tau * theta_acc
    if defect == "semi-implicit Euler":
        new_x, new_theta = x + tau * new_x_dot, theta + tau * new_theta_dot
    elif defect == "fma":
        with mpmath.workprec(ref.EXACT_BITS):               # x + tau * x_dot rounded once
            new_x = np.array([float(mpmath.mpf(a) + mpmath.mpf(tau) * mpmath.mpf(b)) for a, b in zip(x.tolist(), x_dot.tolist())])
        new_theta = theta + tau * theta_dot
    else:
        new_x, new_theta = x + tau * x_dot, theta + tau * theta_dot
    nxt = np.stack([new_x, new_x_dot, new_theta, new_theta_dot], axis=1)
    if defect == "float32 state":
        nxt = nxt.astype(np.float32).astype(np.float64)
    limit = {"limit 24 degrees": 24 * 2 * math.pi / 360, "limit in degrees": 12.0}.get(defect, 12 * 2 * math.pi / 360)
    if defect == ">= at the limits":
        fell = (np.abs(nxt[:, 0]) >= 2.4) | (np.abs(nxt[:, 2]) >= limit)
    else:
        fell = (np.abs(nxt[:, 0]) > 2.4) | (np.abs(nxt[:, 2]) > limit)
    cap = {"cap at 499": 499, "cap at 501": 501}.get(defect, 500)
    return nxt, fell | (steps + 1 >= cap)


def flag_cases():
    """name -> (state, action, counter before the ply, the done flag the rules give)."""
    out = {}
    state, action, fallen = cases.theta_limit_states()
    out["theta limit"] = (state, action, np.zeros(len(state), int), fallen)
    state, action, fallen = cases.x_limit_states()
    out["x limit"] = (state, action, np.zeros(len(state), int), fallen)
    state = cases.balanced_states(4)
    steps = np.array([497, 498, 499, 500])
    out["cap"] = (state, np.array([0, 1, 0, 1]), steps, np.array([False, False, True, True]))
    return out


BOUND_DEFECTS = ["force sign", "theta_dot not squared", "no cos^2", "4/3 as 1.33", "full length in pole_ml",
                 "semi-implicit Euler", "tau 0.2", "float32 state"]
FLAG_DEFECTS = {">= at the limits": ("theta limit", "x limit"), "limit 24 degrees": ("theta limit",),
                "limit in degrees": ("theta limit",), "cap at 499": ("cap",), "cap at 501": ("cap",)}


def test_the_copy_itself_passes_every_case(interior):
    nxt, done = copy_step(interior["state"], interior["action"], np.zeros(cases.SWEEP, int))
    assert ref.same_bits(nxt, interior["next"]).all() and np.array_equal(done, interior["done"])
    for name, (state, action, steps, want) in flag_cases().items():
        assert np.array_equal(copy_step(state, action, steps)[1], want), name
        sin_t, cos_t = ref.host_sin_cos(state[:, 2])
        assert np.array_equal(ref.done_after(ref.step_f64(state, action, sin_t, cos_t)[1], steps + 1), want), name


@pytest.mark.parametrize("defect", BOUND_DEFECTS)
def test_arithmetic_defect_leaves_the_bound(interior, defect):
    nxt, _ = copy_step(interior["state"], interior["action"], np.zeros(cases.SWEEP, int), defect)
    worst, where = ref.error_over_bound(nxt[:1024], interior["exact"][:1024], interior["bound"][:1024])
    print(f"{defect}: misses the bound of case 'interior' by a factor {worst:.3g} at {where}")
    assert worst > 1.0
    assert not ref.same_bits(nxt, interior["next"]).all()


def test_fma_defect_breaks_the_bit_identity(interior):
    """An fma rounds x + tau * x_dot once instead of twice: it is CLOSER to the exact value, so no error bound can refuse
    it.  What refuses it is the bit identity with step_f64, which is the check the device is held to."""
    nxt, _ = copy_step(interior["state"], interior["action"], np.zeros(cases.SWEEP, int), "fma")
    differ = ~ref.same_bits(nxt, interior["next"]).all(axis=1)
    worst, _ = ref.error_over_bound(nxt[:1024], interior["exact"][:1024], interior["bound"][:1024])
    print(f"fma: {differ.sum()} of {cases.SWEEP} states of case 'interior' differ in bits; error / bound {worst:.3f}")
    # (how often: the product's rounding error, half an ulp of ~0.05, moves a sum of size ~2 across a rounding boundary
    # about once in 2^5 states; the small states, where x and tau * x_dot are of one size, differ far more often)
    assert differ.sum() >= cases.SWEEP // 64 and worst <= 1.0


@pytest.mark.parametrize("defect", sorted(FLAG_DEFECTS))
def test_flag_defect_gives_a_wrong_done(defect):
    table = flag_cases()
    for name in FLAG_DEFECTS[defect]:
        state, action, steps, want = table[name]
        got = copy_step(state, action, steps, defect)[1]
        print(f"{defect}: {(got != want).sum()} of {len(want)} flags of case '{name}' wrong")
        assert (got != want).any(), name
