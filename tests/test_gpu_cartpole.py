"""CartPole on the device (csrc/env_kernels.hip) held to its equations.  With the device's own sin(theta) and cos(theta)
handed to the reference, every other operation of a step is one correctly rounded + - * / in a fixed order, so the next
state read back must equal tests/cartpole_reference.py::step_f64 BIT FOR BIT, from the state read before the ply: nothing
compounds.  `done` is then an exact function of those bits and of the ply counter.  The two library calls are measured
on their own and bounded (SINCOS_ULPS_L), which ties the device to the equations (step_exact) and not only to a copy of
its own text."""
import importlib

import mpmath
import numpy as np
import pytest
import torch

import cartpole_cases as cases
import cartpole_reference as ref

pytestmark = pytest.mark.gpu

L = ref.SINCOS_ULPS_L


@pytest.fixture(scope="module")
def dev(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd.games.device")


@pytest.fixture(scope="module")
def native(pkg):
    return importlib.import_module("muzero-hypermodel_amd._native")


def device_sin_cos(native, theta):
    theta = np.ascontiguousarray(theta, np.float64)
    sin_t, cos_t = np.empty_like(theta), np.empty_like(theta)
    P = native.c_f64_p
    assert native.load().mzmcts_device_sincos(native.ptr(theta, P), theta.size, native.ptr(sin_t, P), native.ptr(cos_t, P)) == 0
    return sin_t, cos_t


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (bits32(a) == bits32(b)) | (np.isnan(a) & np.isnan(b))


def cast(state):
    with np.errstate(all="ignore"):
        return np.asarray(state, np.float64).astype(np.float32)


def assert_step(native, before, steps_before, action, after, steps_after, reward, done, max_moves=0, what=""):
    """One ply of every env judged on the device's own input: before / after are the fp64 states read around it."""
    played = action >= 0
    sin_t, cos_t = device_sin_cos(native, before[:, 2])
    want, own = ref.step_f64(before, action, sin_t, cos_t)
    same = ref.same_bits(after, want).all(axis=1)
    assert same[played].all(), f"{what}: {(~same[played]).sum()} states differ from step_f64, first env {np.flatnonzero(played & ~same)[:4]}"
    assert np.array_equal(steps_after[played], steps_before[played] + 1), what
    assert np.array_equal(done[played], ref.done_after(own, steps_before + 1, max_moves)[played]), what
    assert (reward[played] == 1.0).all(), what
    # an env with action < 0 keeps its state bits (NaN payloads included) and its counter; its reward and done read 0
    idle = ~played
    assert (after[idle].view(np.uint64) == before[idle].view(np.uint64)).all(), what
    assert np.array_equal(steps_after[idle], steps_before[idle]) and not done[idle].any() and (reward[idle] == 0.0).all(), what
    return want, own, sin_t, cos_t


def one_step(envs, state, steps, action):
    envs.set_state(state, steps)
    reward, done = envs.step(action)
    reward, done = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
    after, steps_after = envs.get_state()
    return after, steps_after, reward, done


@pytest.fixture(scope="module")
def sweep_envs(dev):
    envs = dev.DeviceEnvs("cartpole", cases.SWEEP, seeds=np.arange(cases.SWEEP))
    yield envs
    envs.close()


@pytest.mark.parametrize("launch", ["interior", "interior, other action", "edges"])
def test_one_step_sweep_is_bit_exact(native, sweep_envs, launch):
    """4096 states per launch through mzenv_step; the two interior launches give every state both actions, the third
    tiles the edge set (signed zeros, subnormal theta, both limits and their neighbours, overflowing squares, inf and NaN in
    each component).  One env in 17 sits the launch out (action -1)."""
    E = cases.SWEEP
    if launch == "edges":
        state, action = cases.edges()
        rows = np.arange(E) % len(state)
        state, action = state[rows], action[rows]
        idle = np.arange(E) % 17 == 16                        # (17 and the edge count share no factor: every edge is played)
    else:
        state, action = cases.interior()
        if launch != "interior":
            action = 1 - action
        idle = np.arange(E) % 17 == (16 if launch == "interior" else 3)
    action = np.where(idle, -1, action).astype(np.int32)
    steps = (np.arange(E) % 400).astype(np.int32)
    after, steps_after, reward, done = one_step(sweep_envs, state, steps, action)
    want, own, sin_t, cos_t = assert_step(native, state, steps, action, after, steps_after, reward, done, what=launch)
    if launch == "edges":
        # the thresholds on those bits: on the limit is not fallen, the next double beyond is; a NaN compares false
        for limit_state, _, fallen in (cases.theta_limit_states(), cases.x_limit_states()):
            for row, f in zip(limit_state, fallen):
                hit = (state.view(np.uint64) == row.view(np.uint64)).all(axis=1) & ~idle
                assert hit.any() and (done[hit] == f).all()
        nan_next = np.isnan(after[:, 0]) & np.isnan(after[:, 2]) & ~idle
        assert nan_next.any() and not done[nan_next].any()
    else:
        # ... and the equations themselves: with sin / cos within L ulps the device's state lies within the running
        # error bound of the mpmath step
        keep = ~idle
        worst, where = ref.error_over_bound(after[keep], ref.step_exact(state[keep], action[keep]),
                                            ref.step_bound(state[keep], action[keep], L, sin_t[keep], cos_t[keep]))
        print(f"{launch}: worst error / bound(L = {L}) against the mpmath step {worst:.3f} at {where}")
        assert worst <= 1.0


@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_ragged_grids_touch_nothing_past_the_last_env(dev, native, E):
    """One thread per env, 256 per block: first and last env are right and the row past E of every output keeps its
    sentinel, through step, observe and advance."""
    envs = dev.DeviceEnvs("cartpole", E, seeds=np.arange(E) + 100)
    state = cases.interior(E, seed=E)[0]
    action = (np.arange(E) % 2).astype(np.int32)
    reward = torch.full((E + 1,), -3.0, dtype=torch.float32, device="cuda")
    done = torch.full((E + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    obs = torch.full((E + 1, 1, 1, 4), -3.0, dtype=torch.float32, device="cuda")
    obs_after, obs_next = obs.clone(), obs.clone()
    actions = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    actions[:E] = torch.from_numpy(action).cuda()
    envs.legal = torch.full((E + 1, 2), -7, dtype=torch.int32, device="cuda")
    envs.num_legal = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    envs.to_play = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")

    def check_sentinels():
        assert reward[E].item() == -3.0 and done[E].item() == 0xAB
        for t in (obs, obs_after, obs_next):
            assert (t[E] == -3.0).all()
        assert (envs.legal[E] == -7).all() and envs.num_legal[E].item() == -7 and envs.to_play[E].item() == -7

    steps = np.zeros(E, np.int32)
    envs.set_state(state, steps)
    envs.step(actions, reward=reward, done=done)
    after, steps_after = envs.get_state()
    assert_step(native, state, steps, action, after, steps_after, reward[:E].cpu().numpy(), done[:E].cpu().numpy().astype(bool))
    envs.observe(obs)
    assert same_bits32(obs[:E].cpu().numpy().reshape(E, 4), cast(after)).all()
    assert (envs.legal[:E].cpu().numpy() == [0, 1]).all() and (envs.num_legal[:E] == 2).all() and (envs.to_play[:E] == 0).all()
    check_sentinels()
    envs.set_state(state, steps)
    envs.advance(actions, reward, done, obs_after, obs_next)
    after, steps_after = envs.get_state()
    d = done[:E].cpu().numpy().astype(bool)
    want, own = ref.step_f64(state, action, *device_sin_cos(native, state[:, 2]))
    assert np.array_equal(d, own) and (reward[:E] == 1.0).all()
    assert ref.same_bits(after[~d], want[~d]).all() and np.array_equal(steps_after, np.where(d, 0, 1))
    assert ref.same_bits(after[d], ref.reset_table(np.arange(E)[d] + 100, 2)[:, 1]).all()     # (the finished envs' next draw)
    assert same_bits32(obs_after[:E].cpu().numpy().reshape(E, 4), cast(want)).all()
    assert same_bits32(obs_next[:E].cpu().numpy().reshape(E, 4), cast(after)).all()
    check_sentinels()
    envs.close()


def test_device_sin_cos_within_l_ulps(native):
    """The two inexact operations of a step, measured: the device library's sin and cos against numpy.longdouble on 2^20
    seeded doubles |theta| <= 0.5 plus the edge thetas, a subset against mpmath.  L (cartpole_reference.SINCOS_ULPS_L) is
    the worst distance measured this way, rounded up to the next integer."""
    assert np.finfo(np.longdouble).nmant >= 63
    theta = np.concatenate([np.random.RandomState(11).uniform(-0.5, 0.5, size=1 << 20), cases.EDGE_THETAS])
    sin_t, cos_t = device_sin_cos(native, theta)
    wide = theta.astype(np.longdouble)
    true_sin, true_cos = np.sin(wide), np.cos(wide)
    sin_ulps, cos_ulps = ref.ulps_from(sin_t, true_sin), ref.ulps_from(cos_t, true_cos)
    glibc_sin, glibc_cos = ref.host_sin_cos(theta)
    print(f"device sin: worst {sin_ulps.max():.4f} ulps at theta = {theta[sin_ulps.argmax()]!r}; "
          f"cos: worst {cos_ulps.max():.4f} ulps at theta = {theta[cos_ulps.argmax()]!r}; "
          f"differ from glibc's bits: sin {(sin_t != glibc_sin).sum()}, cos {(cos_t != glibc_cos).sum()} of {theta.size}")
    assert sin_ulps.max() <= L and cos_ulps.max() <= L
    # the long-double values themselves, and the device, against mpmath on a subset: sinl / cosl are within one
    # long-double ulp = 2^-11 double ulps, so the yardstick is good to 2^-10 of the unit it measures in
    subset = np.concatenate([np.arange(2048), np.arange(theta.size - len(cases.EDGE_THETAS), theta.size)])
    with mpmath.workprec(ref.EXACT_BITS):
        for i in subset.tolist():
            for got, true_ld, fn in ((sin_t[i], true_sin[i], mpmath.sin), (cos_t[i], true_cos[i], mpmath.cos)):
                exact = fn(mpmath.mpf(float(theta[i])))
                spacing = mpmath.mpf(float(np.spacing(abs(float(true_ld)))))
                hi, lo = float(true_ld), float(true_ld - np.longdouble(float(true_ld)))
                assert abs(mpmath.mpf(hi) + mpmath.mpf(lo) - exact) <= spacing * 2.0 ** -10
                assert abs(mpmath.mpf(float(got)) - exact) <= spacing * L


def test_cap_and_move_limit_end_the_game_on_the_ply_the_header_says(dev, native):
    """The ply counter handed in with set_state is what CartPole's 500 cap and mzenv_set_max_moves read: done arrives on
    the ply that brings it to 500 (or to the limit, or beyond a limit lowered in mid-game) and on no other, with reward 1;
    mzenv_game_moves agrees; a reset zeroes the counter."""
    E = 12
    seeds = np.arange(E) + 7
    table = ref.reset_table(seeds, 5)
    state = cases.balanced_states(E)
    action = (np.arange(E) % 2).astype(np.int32)
    for path in ("step", "advance"):
        envs = dev.DeviceEnvs("cartpole", E, seeds=seeds)
        resets = np.zeros(E, int)
        for max_moves, steps, want_done in (
                (0, [497, 498, 499, 0, 1, 2, 498, 499, 497, 6, 5, 499], [0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1]),
                (600, [497, 498, 499, 0, 1, 2, 498, 499, 497, 6, 5, 499], [0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1]),
                (7, [5, 6, 5, 6, 0, 4, 5, 6, 3, 6, 5, 1], [0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0]),
                (10, [20, 9, 8, 20, 0, 400, 8, 9, 10, 11, 7, 499], [1, 1, 0, 1, 0, 1, 0, 1, 1, 1, 0, 1])):   # lowered mid-game
            steps, want_done = np.array(steps, np.int32), np.array(want_done, bool)
            envs.set_max_moves(0)
            envs.set_state(state, steps)
            envs.set_max_moves(max_moves)
            if path == "step":
                reward, done = envs.step(action)
                reward, done = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
                after, steps_after = envs.get_state()
                assert np.array_equal(envs.game_moves().cpu().numpy(), steps + 1)
                _, own, _, _ = assert_step(native, state, steps, action, after, steps_after, reward, done, max_moves, what=(path, max_moves))
                assert not own.any() and np.array_equal(done, want_done), (path, max_moves)
                envs.reset(torch.from_numpy(done.astype(np.uint8)).cuda())
                resets += done
                after_reset, steps_reset = envs.get_state()
                assert np.array_equal(steps_reset, np.where(done, 0, steps + 1))
                assert np.array_equal(envs.game_moves().cpu().numpy(), steps_reset)
                assert (after_reset[~done].view(np.uint64) == after[~done].view(np.uint64)).all()
            else:
                reward = torch.zeros(E, dtype=torch.float32, device="cuda")
                done_t = torch.zeros(E, dtype=torch.uint8, device="cuda")
                obs_after = torch.zeros((E, 1, 1, 4), dtype=torch.float32, device="cuda")
                obs_next = torch.zeros_like(obs_after)
                envs.advance(torch.from_numpy(action).cuda(), reward, done_t, obs_after, obs_next)
                done = done_t.cpu().numpy().astype(bool)
                assert np.array_equal(done, want_done), (path, max_moves)
                assert (reward.cpu().numpy() == 1.0).all()
                resets += done
                after_reset, steps_reset = envs.get_state()
                assert np.array_equal(steps_reset, np.where(done, 0, steps + 1))
                assert np.array_equal(envs.game_moves().cpu().numpy(), steps_reset)
                want, _ = ref.step_f64(state, action, *device_sin_cos(native, state[:, 2]))
                assert same_bits32(obs_after.cpu().numpy().reshape(E, 4), cast(want)).all()
                assert ref.same_bits(after_reset[~done], want[~done]).all()
            # a finished env's fresh state is the next draw of its own stream: set_state left the stream alone
            assert ref.same_bits(after_reset[done], table[np.flatnonzero(done), resets[done]]).all(), (path, max_moves)
        envs.close()


def pd_action(obs):
    """A fixed PD rule on the device's own observation (balances every seed tried on the CPU to the cap)."""
    x, x_dot, theta, theta_dot = (obs[:, i].astype(np.float64) for i in range(4))
    return (theta + 0.5 * theta_dot + 0.02 * x + 0.1 * x_dot > 0).astype(np.int32)


def test_whole_games_judged_ply_by_ply(dev, native):
    """64 envs play closed loop for 500 plies, envs 0..31 through mzenv_step + mzenv_reset and envs 32..63 through
    mzenv_advance; every ply is held to the bit-exact identity from the state read before it, so nothing compounds (a
    trajectory comparison cannot do this: one ulp in a sine grows by e^(3.9 t)).  At least 48 of the 64 first games must
    reach ply 500, so that the cap is reached by play and not only by a counter handed in."""
    E, plies = 32, 500
    capped = 0
    for path, seeds in (("step", np.arange(E)), ("advance", np.arange(E) + E)):
        table = ref.reset_table(seeds, 40)
        envs = dev.DeviceEnvs("cartpole", E, seeds=seeds)
        resets = np.zeros(E, int)
        before, steps_before = envs.get_state()
        assert ref.same_bits(before, table[:, 0]).all() and not steps_before.any()
        reward_t = torch.zeros(E, dtype=torch.float32, device="cuda")
        done_t = torch.zeros(E, dtype=torch.uint8, device="cuda")
        obs_after = torch.zeros((E, 1, 1, 4), dtype=torch.float32, device="cuda")
        obs_next = torch.zeros_like(obs_after)
        obs = envs.observe()[0].cpu().numpy().reshape(E, 4)
        for ply in range(plies):
            assert (bits32(obs) == bits32(cast(before))).all(), (path, ply)
            action = pd_action(obs)
            if path == "step":
                reward, done = envs.step(action)
                reward, done = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
                after, steps_after = envs.get_state()
                _, own, _, _ = assert_step(native, before, steps_before, action, after, steps_after, reward, done, what=(path, ply))
                if done.any():
                    envs.reset(torch.from_numpy(done.astype(np.uint8)).cuda())
                    after, steps_after = envs.get_state()
                obs = envs.observe()[0].cpu().numpy().reshape(E, 4)
            else:
                envs.advance(torch.from_numpy(action).cuda(), reward_t, done_t, obs_after, obs_next)
                reward, done = reward_t.cpu().numpy(), done_t.cpu().numpy().astype(bool)
                after, steps_after = envs.get_state()
                want, own = ref.step_f64(before, action, *device_sin_cos(native, before[:, 2]))
                assert (bits32(obs_after.cpu().numpy().reshape(E, 4)) == bits32(cast(want))).all(), (path, ply)
                assert ref.same_bits(after[~done], want[~done]).all(), (path, ply)
                assert np.array_equal(done, ref.done_after(own, steps_before + 1)) and (reward == 1.0).all(), (path, ply)
                assert np.array_equal(steps_after[~done], steps_before[~done] + 1), (path, ply)
                obs = obs_next.cpu().numpy().reshape(E, 4)
            if done.any():
                capped += int((done & ~own & (steps_before + 1 == ref.MAX_STEPS) & (resets == 0)).sum())
                resets += done
                assert ref.same_bits(after[done], table[np.flatnonzero(done), resets[done]]).all(), (path, ply)
                assert not steps_after[done].any(), (path, ply)
            before, steps_before = after, steps_after
        envs.close()
    print(f"{capped} of 64 first games reached ply 500")
    assert capped >= 48


@pytest.mark.parametrize("base", [0, 1, 2 ** 31, 2 ** 32 - 1])
def test_first_five_resets_and_the_observation_cast(dev, native, base):
    """Env e is Game((base + e) mod 2^32): its first five resets equal numpy's own draws bit for bit, through mzenv_reset
    and through mzenv_advance's own reset (the first from mzenv_create + reset, the later ones after a forced done: two
    envs in three are put beyond the track each round).  The observation is the fp64 state's astype(float32): obs_after of
    a finishing ply is the terminal state's cast, obs_next the fresh state's."""
    E = 257
    seeds = (base + np.arange(E)) & 0xFFFFFFFF
    table = ref.reset_table(seeds, 5)
    for path in ("reset", "advance"):
        envs = dev.DeviceEnvs("cartpole", E, seeds=seeds)
        resets = np.zeros(E, int)
        reward_t = torch.zeros(E, dtype=torch.float32, device="cuda")
        done_t = torch.zeros(E, dtype=torch.uint8, device="cuda")
        obs_after = torch.zeros((E, 1, 1, 4), dtype=torch.float32, device="cuda")
        obs_next = torch.zeros_like(obs_after)
        state, steps = envs.get_state()
        assert ref.same_bits(state, table[:, 0]).all() and not steps.any()
        assert (bits32(envs.observe()[0].cpu().numpy().reshape(E, 4)) == bits32(cast(state))).all()
        action = (np.arange(E) % 2).astype(np.int32)
        for k in range(6):
            fall = (np.arange(E) + k) % 3 != 0
            state[fall, 0] = np.where(np.arange(E)[fall] % 2 == 0, 3.0, -2.5)
            envs.set_state(state)
            want, own = ref.step_f64(state, action, *device_sin_cos(native, state[:, 2]))
            assert np.array_equal(own, fall)
            if path == "reset":
                reward, done = envs.step(action)
                done = done.cpu().numpy().astype(bool)
                assert (bits32(envs.observe()[0].cpu().numpy().reshape(E, 4)) == bits32(cast(want))).all()
                envs.reset(torch.from_numpy(done.astype(np.uint8)).cuda())
                fresh = envs.observe()[0].cpu().numpy().reshape(E, 4)
            else:
                envs.advance(torch.from_numpy(action).cuda(), reward_t, done_t, obs_after, obs_next)
                done = done_t.cpu().numpy().astype(bool)
                assert (bits32(obs_after.cpu().numpy().reshape(E, 4)) == bits32(cast(want))).all()
                fresh = obs_next.cpu().numpy().reshape(E, 4)
            assert np.array_equal(done, fall)
            resets += done
            state, steps = envs.get_state()
            assert ref.same_bits(state[done], table[np.flatnonzero(done), resets[done]]).all(), (path, k)
            assert ref.same_bits(state[~done], want[~done]).all() and not steps[done].any()
            assert (bits32(fresh) == bits32(cast(state))).all()
        assert (resets == 4).all()
        envs.close()


def test_observation_cast_at_float32_ties_and_beyond_its_range(dev):
    """States set by hand on float32 ties (1 + 2^-24 and the like, their neighbours, the same in float32's subnormal
    range) and beyond float32's range: the observation is round-to-nearest-even, subnormals kept, inf beyond the range."""
    values = cases.cast_edges()
    E = len(values)
    state = np.stack([np.roll(values, -i) for i in range(4)], axis=1)
    envs = dev.DeviceEnvs("cartpole", E, seeds=np.arange(E))
    envs.set_state(state)
    obs = envs.observe()[0].cpu().numpy().reshape(E, 4)
    want = cast(state)
    same = same_bits32(obs, want)
    assert same.all(), f"{(~same).sum()} casts differ: {state[~same][:4]!r} -> {obs[~same][:4]!r}, want {want[~same][:4]!r}"
    assert np.isinf(want).any() and (want == np.float32(1.0)).any() and ((want != 0) & (np.abs(want) < 2.0 ** -126)).any()
    envs.close()


def test_state_entries_refuse_and_round_trip(dev, native):
    lib = native.load()
    other = dev.DeviceEnvs("tictactoe", 4)
    state, steps = np.zeros((4, 4)), np.zeros(4, np.int32)
    assert lib.mzenv_get_state(other._h, state.ctypes.data, steps.ctypes.data) == -1
    assert b"only cartpole" in lib.mzenv_last_error(other._h)
    assert lib.mzenv_set_state(other._h, state.ctypes.data, steps.ctypes.data) == -1
    assert b"only cartpole" in lib.mzenv_last_error(other._h)
    with pytest.raises(RuntimeError, match="only cartpole"):
        other.get_state()
    with pytest.raises(RuntimeError, match="only cartpole"):
        other.set_state(state)
    other.close()

    E = 300
    envs = dev.DeviceEnvs("cartpole", E, seeds=np.arange(E))
    first, _ = envs.get_state()
    pattern = np.random.RandomState(3).randint(0, 2 ** 63, size=(E, 4)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    pattern[0] = [0x7FF0000000000001, 0xFFF8DEADBEEF0001, 0x7FF8000000000000, 0xFFF0000000000000]   # NaN payloads, -inf
    pattern[1] = [0x8000000000000000, 0x0000000000000001, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000]
    state = pattern.view(np.float64)
    steps = (np.arange(E) * 7 % 501).astype(np.int32)
    envs.set_state(state, steps)
    got, got_steps = envs.get_state()
    assert (got.view(np.uint64) == pattern).all() and np.array_equal(got_steps, steps)
    assert np.array_equal(envs.game_moves().cpu().numpy(), steps)
    # null arguments and negative counters are refused and change nothing; steps = None leaves the counters
    assert lib.mzenv_set_state(envs._h, None, steps.ctypes.data) == -1 and b"null argument" in lib.mzenv_last_error(envs._h)
    assert lib.mzenv_get_state(envs._h, None, steps.ctypes.data) == -1 and b"null argument" in lib.mzenv_last_error(envs._h)
    bad = steps.copy()
    bad[E - 1] = -1
    with pytest.raises(RuntimeError, match="step count"):
        envs.set_state(first, bad)
    got, got_steps = envs.get_state()
    assert (got.view(np.uint64) == pattern).all() and np.array_equal(got_steps, steps)
    envs.set_state(first)
    got, got_steps = envs.get_state()
    assert (got.view(np.uint64) == first.view(np.uint64)).all() and np.array_equal(got_steps, steps)
    alone = np.empty((E, 4))
    assert lib.mzenv_get_state(envs._h, alone.ctypes.data, None) == 0 and (alone.view(np.uint64) == first.view(np.uint64)).all()
    envs.close()
