"""Acrobot as a device env, the parts that need no GPU: the fp32 twin
(``garage_amd.envs.AcrobotEnv``, the arithmetic ``include/garage_amd.h`` fixes)
against a float64 restatement of gym 0.17's equations (the "book" dynamics with
``np.sin`` / ``np.cos``, one true RK4 step of 0.2, ``((x + pi) mod 2 pi) - pi``
and the speed bounds), the range of the RK4 stage angles and the reduction that
is trusted on it, the exact invariants of the state and episode semantics.

What every kind states the same way (reset draws against a
pure-Python Philox, the ctypes mirror of its struct, the argument errors of the
entry points) is in ``test_state_envs_cpu.py``, row ``acrobot``.

The bounds on |twin - float64| are 4x the worst error measured when the
arithmetic was fixed (the restatement is the yardstick; the factor leaves room
for another sample).  The accelerations reach thousands at the speed bounds and
one step multiplies a rounding error of a stage angle by hundreds there, so the
worst case over the whole state box is far above the typical one.  Measured
(angles on the circle / speeds):
  one step from 300 000 states of the whole box, all classes
                                    6.2e-5 / 4.4e-2  (medians 1.5e-7 / 3.5e-7)
  ten steps from 4096 reset states under each constant torque
                                    2.1e-7 / 4.0e-7
  reduce + sincos over |th| <= 34 (sin / cos)       2.2e-7 / 2.5e-7
  largest |stage angle| over the box and the torques, float64: 33.32"""
import numpy as np
import pytest

PI = np.pi
BOX = np.array([PI, PI, 4 * PI, 9 * PI])

# 4x the measured worst (module docstring)
ONE_STEP_ANGLE, ONE_STEP_SPEED = 4 * 6.2e-5, 4 * 4.4e-2
TEN_STEPS_ANGLE, TEN_STEPS_SPEED = 4 * 2.1e-7, 4 * 4.0e-7
REDUCED_SIN, REDUCED_COS = 4 * 2.2e-7, 4 * 2.5e-7
# the range reduce is trusted on (the header states 33.32 and trusts 34)
STAGE_RANGE = 34.0


def dsdt_f64(y, a):
    """gym 0.17 ``AcrobotEnv._dsdt`` ("book"): m1 = m2 = l1 = 1, lc1 = lc2 =
    0.5, I1 = I2 = 1, g = 9.8."""
    th1, th2, w1, w2 = y
    d1 = 0.25 + (1 + 0.25 + 2 * 0.5 * np.cos(th2)) + 1 + 1
    d2 = (0.25 + 0.5 * np.cos(th2)) + 1
    phi2 = 0.5 * 9.8 * np.cos(th1 + th2 - PI / 2)
    phi1 = (-0.5 * w2**2 * np.sin(th2) - 2 * 0.5 * w2 * w1 * np.sin(th2) +
            1.5 * 9.8 * np.cos(th1 - PI / 2) + phi2)
    acc2 = (a + d2 / d1 * phi1 - 0.5 * w1**2 * np.sin(th2) - phi2) / (
        0.25 + 1 - d2**2 / d1)
    acc1 = -(d2 * acc2 + phi1) / d1
    return np.stack([w1, w2, acc1, acc2])


def step_f64(state, torque):
    """One env step in float64, vectorised over the leading axis: the new
    state, the height expression ``-cos th1 - cos(th1 + th2)`` of it and the
    largest |angle| any RK4 stage (the unwrapped new angle included) saw."""
    y = np.asarray(state, dtype=np.float64).T
    a = np.asarray(torque, dtype=np.float64)
    k1 = dsdt_f64(y, a)
    y2 = y + 0.1 * k1
    k2 = dsdt_f64(y2, a)
    y3 = y + 0.1 * k2
    k3 = dsdt_f64(y3, a)
    y4 = y + 0.2 * k3
    k4 = dsdt_f64(y4, a)
    yn = y + 0.2 / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    stage = np.abs(np.stack([y2[:2], y3[:2], y4[:2], yn[:2]])).max(axis=(0, 1))
    th = ((yn[:2] + PI) % (2 * PI)) - PI
    new = np.stack([th[0], th[1], np.clip(yn[2], -4 * PI, 4 * PI),
                    np.clip(yn[3], -9 * PI, 9 * PI)], axis=-1)
    height = -np.cos(th[0]) - np.cos(th[1] + th[0])
    return new, height, stage


def on_circle(a, b):
    return np.abs(((a - b + PI) % (2 * PI)) - PI)


def _box_states(m, rng):
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    st = (rng.uniform(-1, 1, (m, 4)) * BOX).astype(f)
    # a share on the faces of the speed box, where the stage angles peak
    st[:m // 8, 2] = np.where(st[:m // 8, 2] < 0, -1, 1) * AcrobotEnv.MAX_VEL_1
    st[:m // 4, 3] = np.where(st[:m // 4, 3] < 0, -1, 1) * AcrobotEnv.MAX_VEL_2
    hi = np.asarray([AcrobotEnv.PI, AcrobotEnv.PI, AcrobotEnv.MAX_VEL_1,
                     AcrobotEnv.MAX_VEL_2], dtype=f)
    return np.clip(st, -hi, hi)


_cache = {}


def _one_step_sample():
    """300 000 states of the whole box with classes 0, 1, 2 and, for some, the
    out-of-range indices 3 and -1 (no torque), stepped once by both."""
    if not _cache:
        from garage_amd.envs import AcrobotEnv
        rng = np.random.RandomState(0)
        m = 300_000
        st = _box_states(m, rng)
        act = rng.randint(0, 3, m)
        act[::50] = 3
        act[1::50] = -1
        tq = np.where(act == 0, -1.0, np.where(act == 2, 1.0, 0.0))
        _cache.update(state=st, action=act,
                      twin=AcrobotEnv.advance(st, act),
                      ref=step_f64(st, tq))
    return _cache


def test_twin_against_float64_one_step_over_the_whole_box():
    from garage_amd.envs import AcrobotEnv
    c = _one_step_sample()
    new, obs, rew, done = c['twin']
    ref, height, _ = c['ref']
    m = len(c['action'])
    assert new.dtype == obs.dtype == rew.dtype == np.float32
    assert new.shape == (m, 4) and obs.shape == (m, 6)
    assert rew.shape == done.shape == (m, ) and done.dtype == np.bool_
    ea = on_circle(new[:, :2].astype(np.float64), ref[:, :2])
    es = np.abs(new[:, 2:] - ref[:, 2:])
    print('one step, {} states, max |twin - float64|: angle {:.3e} (median '
          '{:.3e}) speed {:.3e} (median {:.3e})'.format(
              m, ea.max(), np.median(ea), es.max(), np.median(es)))
    assert ea.max() <= ONE_STEP_ANGLE and es.max() <= ONE_STEP_SPEED
    # the observation is that of the new state
    assert obs.tobytes() == AcrobotEnv.observe(new).tobytes()
    # termination wherever the restatement is clear of its threshold
    clear = np.abs(height - 1) > 1e-5
    left_out = 1.0 - clear.mean()
    print('done left uncompared: {:.4%}; done in {:.1%}'.format(
        left_out, done.mean()))
    assert left_out < 0.01
    assert np.array_equal(done[clear], (height > 1)[clear])
    assert done.any() and not done.all()
    assert np.array_equal(rew, np.where(done, 0, -1).astype(np.float32))
    # out-of-range classes are no torque: classes 3 and -1 step as 1 does
    st, act = c['state'], c['action']
    for k in (3, -1):
        sel = act == k
        assert sel.sum() > 1000
        as_one, _, _, _ = AcrobotEnv.advance(st[sel], np.ones(sel.sum(), int))
        assert as_one.tobytes() == new[sel].tobytes()
    assert np.array_equal(AcrobotEnv.torque([0, 1, 2, 3, -1, 7]),
                          np.asarray([-1, 0, 1, 0, 0, 0], dtype=np.float32))


def test_exact_invariants_of_the_state_and_the_observation():
    from garage_amd.envs import AcrobotEnv
    c = _one_step_sample()
    new, obs, _, _ = c['twin']
    assert np.isfinite(new).all()
    assert (np.abs(new[:, :2]) <= AcrobotEnv.PI).all()
    assert (np.abs(new[:, 2]) <= AcrobotEnv.MAX_VEL_1).all()
    assert (np.abs(new[:, 3]) <= AcrobotEnv.MAX_VEL_2).all()
    # both clips are reached, either way
    for j, b in ((2, AcrobotEnv.MAX_VEL_1), (3, AcrobotEnv.MAX_VEL_2)):
        assert (new[:, j] == b).any() and (new[:, j] == -b).any()
    box = AcrobotEnv().spec.observation_space
    assert box.low.dtype == np.float32 and box.shape == (6, )
    assert box.high.tolist() == [1, 1, 1, 1, float(np.float32(4 * PI)),
                                 float(np.float32(9 * PI))]
    assert (box.low == -box.high).all()
    assert (obs >= box.low).all() and (obs <= box.high).all()
    assert AcrobotEnv().spec.action_space.n == 3
    assert AcrobotEnv.MAX_VEL_1 == np.float32(4 * PI)
    assert AcrobotEnv.MAX_VEL_2 == np.float32(9 * PI)
    assert AcrobotEnv.H6 == np.float32(0.2 / 6.0)


def _reset_states(m, seed=4):
    from garage_amd.envs import acrobot_reset_draw
    return np.stack([acrobot_reset_draw(seed, i, i % 3) for i in range(m)])


def test_twin_against_float64_ten_steps_from_reset_states():
    from garage_amd.envs import AcrobotEnv
    m = 4096
    worst_a = worst_s = 0.0
    for k, tq in ((0, -1.0), (1, 0.0), (2, 1.0)):
        state = _reset_states(m)
        s64 = state.astype(np.float64)
        act = np.full(m, k)
        for t in range(10):
            state, obs, rew, done = AcrobotEnv.advance(state, act)
            s64, height, _ = step_f64(s64, np.full(m, tq))
            worst_a = max(worst_a, on_circle(state[:, :2].astype(np.float64),
                                             s64[:, :2]).max())
            worst_s = max(worst_s, np.abs(state[:, 2:] - s64[:, 2:]).max())
            # nothing swings up within ten steps of such a start
            assert not done.any() and (height < 1 - 1e-5).all()
            assert (rew == -1).all()
    print('ten steps, max |twin - float64|: angle {:.3e} speed {:.3e}'.format(
        worst_a, worst_s))
    assert worst_a <= TEN_STEPS_ANGLE and worst_s <= TEN_STEPS_SPEED


def test_stage_angle_range_and_reduce_with_sincos_on_it():
    """The largest |stage angle| from the whole state box under the three
    torques, by a random search over the float64 restatement with a local
    refinement around the best; then ``reduce`` + ``sincos`` against float64
    over the range the header trusts them on."""
    from garage_amd.envs import AcrobotEnv, PendulumEnv
    c = _one_step_sample()
    stage = c['ref'][2]
    rng = np.random.RandomState(1)
    cand = c['state'][np.argsort(stage)[-50:]].astype(np.float64)
    best = stage.max()
    for it in range(12):
        loc = np.repeat(cand, 200, axis=0)
        loc = np.clip(loc + rng.normal(0, 0.05 * 0.6**it, loc.shape) * BOX,
                      -BOX, BOX)
        _, _, s = step_f64(loc, rng.randint(0, 3, len(loc)) - 1.0)
        cand = loc[np.argsort(s)[-50:]]
        best = max(best, s.max())
    print('largest |stage angle|: {:.4f} at {}'.format(best, cand[-1]))
    assert 33.0 < best < 33.4 < STAGE_RANGE  # the header: 33.32
    # it is reached at both speed bounds
    assert np.allclose(np.abs(cand[-1, 2:]), BOX[2:])

    th = np.concatenate([
        rng.uniform(-STAGE_RANGE, STAGE_RANGE, 1_000_000),
        np.linspace(-STAGE_RANGE, STAGE_RANGE, 1_000_001),
        # next to every multiple of pi and of pi / 2: the wrap and the folds
        (np.arange(-22, 23)[:, None] * (PI / 2) +
         np.linspace(-1e-5, 1e-5, 201)[None]).reshape(-1)]).astype(np.float32)
    r = AcrobotEnv.reduce(th)
    assert r.dtype == np.float32
    assert (np.abs(r) <= AcrobotEnv.PI).all()
    sn, cs = PendulumEnv.sincos(r)
    t64 = th.astype(np.float64)
    e_sin = np.abs(sn - np.sin(t64)).max()
    e_cos = np.abs(cs - np.cos(t64)).max()
    print('reduce + sincos over |th| <= {}: sin {:.3e} cos {:.3e}'.format(
        STAGE_RANGE, e_sin, e_cos))
    assert e_sin <= REDUCED_SIN and e_cos <= REDUCED_COS
    # inside [-PI, PI) reduce changes nothing but the wrap of exactly PI's
    # neighbourhood, so the states the twin keeps are fixed points of it
    inside = np.abs(th) < np.float32(3.1415)
    assert r[inside].tobytes() == th[inside].tobytes()
    assert AcrobotEnv.R_HI == np.float32(6.28125)
    assert float(AcrobotEnv.R_HI) + float(AcrobotEnv.R_LO) == pytest.approx(
        2 * PI, abs=1e-9)
    # k * R_HI is exact for every k the range needs
    k = np.arange(-6, 7).astype(np.float32)
    assert ((k * AcrobotEnv.R_HI).astype(np.float64) == k * 6.28125).all()


def test_hanging_arm_at_rest_is_a_fixed_point_bit_for_bit():
    from garage_amd.envs import AcrobotEnv
    rest = np.zeros((1, 4), dtype=np.float32)
    s = rest
    for _ in range(3):
        s, obs, rew, done = AcrobotEnv.advance(s, np.ones(1, dtype=int))
        assert s.tobytes() == rest.tobytes()  # +0 everywhere
        assert obs.tolist() == [[1, 0, 1, 0, 0, 0]]
        assert rew[0] == -1 and not done[0]
    new, height, _ = step_f64(np.zeros((1, 4)), np.zeros(1))
    # (gym's cos(th - pi / 2) leaves 6e-17 where the sine is 0)
    assert (np.abs(new) < 1e-15).all() and height[0] == -2
    # a torque moves it, and opposite torques mirror each other exactly
    a, _, _, _ = AcrobotEnv.advance(rest, np.zeros(1, dtype=int))
    b, _, _, _ = AcrobotEnv.advance(rest, np.full(1, 2))
    assert (a != 0).all() and np.array_equal(a, -b)


def test_restatement_swings_up_under_a_pumping_torque():
    """The restatement is Acrobot: torque with the sign of the second joint's
    speed pumps energy in and the tip passes the line; the twin, stepped with
    the same script, ends on the same step."""
    from garage_amd.envs import AcrobotEnv
    s64 = np.asarray([[0.05, -0.03, 0.0, 0.0]])
    s32 = s64.astype(np.float32)
    ended = [None, None]
    for t in range(500):
        if ended[0] is None:
            tq = np.where(s64[:, 3] >= 0, 1.0, -1.0)
            s64, height, _ = step_f64(s64, tq)
            if height[0] > 1:
                ended[0] = t + 1
        if ended[1] is None:
            k = np.where(s32[:, 3] >= 0, 2, 0)
            s32, _, rew, done = AcrobotEnv.advance(s32, k)
            if done[0]:
                assert rew[0] == 0
                ended[1] = t + 1
    print('pumping swings up after (float64, twin) steps:', ended)
    assert ended[0] is not None and ended[0] < 200
    assert ended[1] is not None and ended[1] < 200


def _goal_state():
    """A state whose next step under class 2 swings the tip over the line
    (found on the twin: an arm pointing almost straight up, moving up)."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    th1 = np.linspace(2.0, 3.0, 201).astype(f)
    st = np.stack([th1, np.zeros_like(th1), np.full_like(th1, 2.0),
                   np.zeros_like(th1)], axis=-1)
    _, _, _, before = AcrobotEnv.advance(st, np.full(len(st), 2))
    hgt = -np.cos(th1.astype(np.float64)) - np.cos(th1.astype(np.float64))
    ok = np.nonzero(before & (hgt < 0.99))[0]
    assert len(ok)
    return st[ok[0]]


def test_twin_episode_semantics():
    from garage_amd._dtypes import StepType
    from garage_amd.envs import AcrobotEnv
    goal = _goal_state()
    env = AcrobotEnv(seed=3, env_id=4, max_episode_length=7)
    assert env.spec.observation_space.flat_dim == 6
    assert env.spec.max_episode_length == 7
    assert AcrobotEnv().max_episode_length == 500
    # seven steps from a reset: FIRST, MID ..., TIMEOUT, reward -1 throughout
    obs, info = env.reset()
    assert info == {} and obs.dtype == np.float32 and obs.shape == (6, )
    types = []
    for t in range(7):
        es = env.step(t % 3)
        assert es.observation.dtype == np.float32
        assert isinstance(es.reward, np.float32) and es.env_info == {}
        assert es.reward == -1
        types.append(es.step_type)
    assert types == ([StepType.FIRST] + [StepType.MID] * 5 +
                     [StepType.TIMEOUT])
    # the terminating step: TERMINAL with reward 0, and it wins over FIRST
    env = AcrobotEnv(max_episode_length=5)
    env.reset()
    env.state = goal.copy()
    es = env.step(2)
    assert es.step_type == StepType.TERMINAL and es.reward == 0
    # an array action, as HostVecEnv never passes but garage's workers do
    env.state = goal.copy()
    env._t = 0
    assert env.step(np.asarray([2])).step_type == StepType.TERMINAL
    # max_episode_length 1: every step is a TIMEOUT, at the goal or not; the
    # reward is the step's own
    env = AcrobotEnv(max_episode_length=1)
    env.reset()
    es = env.step(1)
    assert es.step_type == StepType.TIMEOUT and es.reward == -1
    env.reset()
    env.state = goal.copy()
    es = env.step(2)
    assert es.step_type == StepType.TIMEOUT and es.reward == 0  # over TERMINAL
    # max_episode_length 2: FIRST then TIMEOUT; TERMINAL on the first step
    env = AcrobotEnv(max_episode_length=2)
    env.reset()
    assert env.step(1).step_type == StepType.FIRST
    env.state = goal.copy()
    assert env.step(2).step_type == StepType.TIMEOUT
    env.reset()
    env.state = goal.copy()
    assert env.step(2).step_type == StepType.TERMINAL
    assert env.resets == 2
