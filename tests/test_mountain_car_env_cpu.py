"""MountainCar (discrete and continuous) as a device env, the parts that need
no GPU: the fp32 twin (``garage_amd.envs.MountainCarEnv``, the arithmetic
``include/garage_amd.h`` fixes) against a float64 restatement of gym 0.17's
``MountainCar-v0`` and ``MountainCarContinuous-v0`` steps, the exact invariants
(the box, the wall), the "push the way you move" script reaching the goal on
both and episode semantics.

What every kind states the same way (reset draws against a
pure-Python Philox, the ctypes mirror of its struct, the argument errors of the
entry points) is in ``test_state_envs_cpu.py``, rows ``mountain_car`` and
``mountain_car_continuous``.

The bounds on |twin - float64| are 4x the worst error measured when the
arithmetic was fixed (the restatement is the yardstick; the factor leaves room
for another sample).  Measured, position / speed, one step from 300 000 states
of the whole box (the step is discontinuous at the wall, where a car that
touches it stops: the states whose float64 position before the clip is within
1e-6 of -1.2 are compared in position only):
  discrete, classes 0, 1, 2 and out of range     6.4e-8 / 4.3e-9
  continuous, forces in [-1.5, 1.5]              6.4e-8 / 4.3e-9"""
import numpy as np
import pytest


# 4x the measured worst (module docstring)
STEP_X, STEP_V = 4 * 6.4e-8, 4 * 4.3e-9


def step_f64(state, action, continuous):
    """gym 0.17's step in float64, vectorised: the new state, the reward, done
    and the position before its clip."""
    x, v = (np.asarray(state, dtype=np.float64)[..., j] for j in range(2))
    if continuous:
        a = np.asarray(action, dtype=np.float64)
        force = np.minimum(np.maximum(a, -1.0), 1.0)
        v = v + force * 0.0015 - 0.0025 * np.cos(3 * x)
    else:
        k = np.asarray(action)
        k = np.where((k == 0) | (k == 2), k, 1)  # anything else coasts
        v = v + (k - 1) * 0.001 + np.cos(3 * x) * (-0.0025)
    v = np.clip(v, -0.07, 0.07)
    raw = x + v
    x = np.clip(raw, -1.2, 0.6)
    v = np.where((x == -1.2) & (v < 0), 0.0, v)
    done = (x >= (0.45 if continuous else 0.5)) & (v >= 0)
    if continuous:
        reward = np.where(done, 100.0, 0.0) - a * a * 0.1
    else:
        reward = np.full(np.shape(x), -1.0)
    return np.stack([x, v], axis=-1), reward, done, raw


def _box_states(m, rng):
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    st = np.stack([rng.uniform(-1.2, 0.6, m), rng.uniform(-0.07, 0.07, m)],
                  axis=-1).astype(f)
    # the faces of the box: both walls, both speed clips
    st[:m // 50, 0] = MountainCarEnv.MIN_X
    st[m // 50:m // 25, 0] = MountainCarEnv.MAX_X
    st[m // 25:m // 20, 1] = MountainCarEnv.MAX_V
    st[m // 20:m // 16, 1] = -MountainCarEnv.MAX_V
    lo = np.asarray([MountainCarEnv.MIN_X, -MountainCarEnv.MAX_V], dtype=f)
    hi = np.asarray([MountainCarEnv.MAX_X, MountainCarEnv.MAX_V], dtype=f)
    return np.clip(st, lo, hi)


@pytest.mark.parametrize('continuous', [False, True],
                         ids=['discrete', 'continuous'])
def test_twin_against_float64_one_step_over_the_whole_box(continuous):
    from garage_amd.envs import MountainCarEnv
    rng = np.random.RandomState(2 + continuous)
    m = 300_000
    st = _box_states(m, rng)
    if continuous:
        act = rng.uniform(-1.5, 1.5, m).astype(np.float32)
        act[::40] = 0
    else:
        act = rng.randint(0, 3, m)
        act[::50], act[1::50] = 3, -1
    new, obs, rew, done = MountainCarEnv.advance(st, act, continuous)
    ref, want_rew, want_done, raw = step_f64(st, act, continuous)
    assert new.dtype == obs.dtype == rew.dtype == np.float32
    assert new.shape == obs.shape == (m, 2)
    assert rew.shape == done.shape == (m, ) and done.dtype == np.bool_
    assert obs.tobytes() == new.tobytes()
    at_wall = np.abs(raw + 1.2) <= 1e-6
    ex = np.abs(new[:, 0] - ref[:, 0]).max()
    ev = np.abs(new[:, 1] - ref[:, 1])[~at_wall].max()
    print('one step, {} states, max |twin - float64|: x {:.3e} v {:.3e}; '
          '{} states within 1e-6 of the wall'.format(m, ex, ev, at_wall.sum()))
    assert ex <= STEP_X and ev <= STEP_V
    # termination wherever the restatement is clear of both thresholds
    goal = 0.45 if continuous else 0.5
    clear = ((np.abs(ref[:, 0] - goal) > 1e-5) &
             ((np.abs(ref[:, 1]) > 1e-5) | (ref[:, 1] == 0)) & ~at_wall)
    left_out = 1.0 - clear.mean()
    print('done left uncompared: {:.4%}; done in {:.2%}'.format(
        left_out, done.mean()))
    assert left_out < 0.01
    assert np.array_equal(done[clear], want_done[clear])
    assert done.any() and not done.all()
    if continuous:
        # the reward's cost is of the UNCLIPPED force; 100 on the goal step
        cost = np.float32(0.1) * (act * act)
        assert np.array_equal(rew, np.where(done, np.float32(100), 0) - cost)
        assert np.abs(rew[clear] - want_rew[clear]).max() <= 4e-6
        assert rew[done].min() > 99 and rew[~done].max() <= 0
        # forces past +-1 step as +-1 do
        for sign in (-1, 1):
            sel = act * sign > 1
            assert sel.sum() > 1000
            as_one, _, _, _ = MountainCarEnv.advance(
                st[sel], np.full(sel.sum(), sign, np.float32), True)
            assert as_one.tobytes() == new[sel].tobytes()
    else:
        assert (rew == -1).all()
        # out-of-range classes coast: 3 and -1 step as 1 does
        for k in (3, -1):
            sel = act == k
            assert sel.sum() > 1000
            as_one, _, _, _ = MountainCarEnv.advance(
                st[sel], np.ones(sel.sum(), int), False)
            assert as_one.tobytes() == new[sel].tobytes()

    # exact invariants: the state stays inside the declared Box, every face of
    # it is reached, and the wall zeroes a negative speed
    box = MountainCarEnv(continuous=continuous).spec.observation_space
    assert box.low.tolist() == [float(np.float32(-1.2)),
                                float(np.float32(-0.07))]
    assert box.high.tolist() == [float(np.float32(0.6)),
                                 float(np.float32(0.07))]
    assert (obs >= box.low).all() and (obs <= box.high).all()
    for j in range(2):
        assert (new[:, j] == box.low[j]).any()
        assert (new[:, j] == box.high[j]).any()
    on_wall = new[:, 0] == MountainCarEnv.MIN_X
    assert on_wall.sum() > 1000 and (new[on_wall, 1] >= 0).all()
    # (some got there moving left and were stopped; a car put on the wall that
    # moves right keeps its speed)
    assert (new[on_wall, 1] == 0).any()
    came = st[on_wall]
    assert ((came[:, 1] < -0.01) & (came[:, 0] > MountainCarEnv.MIN_X)).any()
    assert (new[:, 1] < 0).any()


def _script(v, continuous):
    """Push the way you move (right from rest)."""
    if continuous:
        return np.where(v >= 0, 1.0, -1.0).astype(np.float32)
    return np.where(v >= 0, 2, 0)


@pytest.mark.parametrize('continuous', [False, True],
                         ids=['discrete', 'continuous'])
def test_pushing_the_way_you_move_reaches_the_goal(continuous):
    """From 1000 reset draws the script reaches the goal on the restatement and
    on the twin, in the same number of steps except where the restatement's
    last position is within 1e-5 of the goal line (at most 1 % of the draws)."""
    from garage_amd.envs import MountainCarEnv, mountain_car_reset_draw
    m = 1000
    s32 = np.stack([mountain_car_reset_draw(6, i, i % 4) for i in range(m)])
    assert (s32[:, 0] >= np.float32(-0.6)).all()
    assert (s32[:, 0] <= np.float32(-0.4)).all() and (s32[:, 1] == 0).all()
    s64 = s32.astype(np.float64)
    goal = 0.45 if continuous else 0.5
    len32, len64 = np.zeros(m, int), np.zeros(m, int)
    last_x = np.zeros(m)
    total32 = np.zeros(m)
    for t in range(MountainCarEnv(continuous=continuous).max_episode_length):
        run32, run64 = len32 == 0, len64 == 0
        if not (run32.any() or run64.any()):
            break
        new, _, rew, done = MountainCarEnv.advance(
            s32, _script(s32[:, 1], continuous), continuous)
        s32 = np.where(run32[:, None], new, s32)
        total32 += np.where(run32, rew, 0)
        len32[run32 & done] = t + 1
        ref, _, done64, _ = step_f64(s64, _script(s64[:, 1], continuous),
                                     continuous)
        s64 = np.where(run64[:, None], ref, s64)
        last_x[run64 & done64] = ref[run64 & done64, 0]
        len64[run64 & done64] = t + 1
    print('steps to the goal: float64 {} .. {}, twin {} .. {}'.format(
        len64.min(), len64.max(), len32.min(), len32.max()))
    limit = 200 if not continuous else 999
    assert (len64 > 0).all() and (len32 > 0).all()
    assert len64.max() < limit and len32.max() < limit
    clear = np.abs(last_x - goal) > 1e-5
    print('episodes left uncompared: {}'.format((~clear).sum()))
    assert (~clear).mean() <= 0.01
    assert np.array_equal(len32[clear], len64[clear])
    if continuous:  # +100 once, minus 0.1 per full push
        assert np.allclose(total32, 100 - 0.1 * len32, atol=1e-3)
    else:
        assert np.array_equal(total32, -len32)


def test_twin_episode_semantics():
    from garage_amd._dtypes import Box, Discrete, StepType
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    # one step from each goal line, moving right
    near = {False: np.asarray([0.499, 0.03], dtype=f),
            True: np.asarray([0.449, 0.03], dtype=f)}
    right = {False: 2, True: np.asarray([1.7], dtype=f)}
    coast = {False: 1, True: np.asarray([0.0], dtype=f)}
    assert MountainCarEnv().max_episode_length == 200
    assert MountainCarEnv(continuous=True).max_episode_length == 999
    assert isinstance(MountainCarEnv().spec.action_space, Discrete)
    assert MountainCarEnv().spec.action_space.n == 3
    box = MountainCarEnv(continuous=True).spec.action_space
    assert isinstance(box, Box) and box.low.tolist() == [-1.0]
    assert box.high.tolist() == [1.0]
    for continuous in (False, True):
        env = MountainCarEnv(seed=3, env_id=4, continuous=continuous,
                             max_episode_length=7)
        assert env.spec.observation_space.flat_dim == 2
        assert env.spec.max_episode_length == 7
        obs, info = env.reset()
        assert info == {} and obs.dtype == np.float32 and obs.shape == (2, )
        types = []
        for t in range(7):
            es = env.step(coast[continuous])
            assert es.observation.dtype == np.float32
            assert isinstance(es.reward, np.float32) and es.env_info == {}
            assert es.reward == (0 if continuous else -1)
            types.append(es.step_type)
        assert types == ([StepType.FIRST] + [StepType.MID] * 5 +
                         [StepType.TIMEOUT])
        # the goal step: TERMINAL (it wins over FIRST); -1, or +100 minus the
        # cost of the unclipped 1.7
        env = MountainCarEnv(continuous=continuous, max_episode_length=5)
        env.reset()
        env.state = near[continuous].copy()
        es = env.step(right[continuous])
        assert es.step_type == StepType.TERMINAL
        want = f(100) - f(0.1) * (f(1.7) * f(1.7)) if continuous else f(-1)
        assert es.reward == want
        # max_episode_length 1: TIMEOUT wins over TERMINAL, the reward stays
        env = MountainCarEnv(continuous=continuous, max_episode_length=1)
        env.reset()
        assert env.step(coast[continuous]).step_type == StepType.TIMEOUT
        env.reset()
        env.state = near[continuous].copy()
        es = env.step(right[continuous])
        assert es.step_type == StepType.TIMEOUT and es.reward == want
        # max_episode_length 2: FIRST then TIMEOUT; TERMINAL on the first step
        env = MountainCarEnv(continuous=continuous, max_episode_length=2)
        env.reset()
        assert env.step(coast[continuous]).step_type == StepType.FIRST
        env.state = near[continuous].copy()
        assert env.step(right[continuous]).step_type == StepType.TIMEOUT
        env.reset()
        env.state = near[continuous].copy()
        assert env.step(right[continuous]).step_type == StepType.TERMINAL
        assert env.resets == 2
    # the two goal lines differ: 0.46 ends the continuous task only
    between = np.asarray([[0.455, 0.01]], dtype=f)
    assert MountainCarEnv.advance(between, np.full(1, 1.0, f), True)[3][0]
    assert not MountainCarEnv.advance(between, np.full(1, 2), False)[3][0]
    # ... and neither ends while the car moves left
    back = np.asarray([[0.55, -0.02]], dtype=f)
    assert not MountainCarEnv.advance(back, np.full(1, -1.0, f), True)[3][0]
    assert not MountainCarEnv.advance(back, np.full(1, 0), False)[3][0]
