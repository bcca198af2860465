"""Pendulum as a device env, the parts that need no GPU: the fp32 twin
(``garage_amd.envs.PendulumEnv``, the arithmetic ``include/garage_amd.h`` fixes)
against the float64 equations of gym 0.17's ``pendulum.py``.

What every kind states the same way (reset draws against a
pure-Python Philox, the ctypes mirror of its struct, the argument errors of the
entry points) is in ``test_state_envs_cpu.py``, row ``pendulum``.

The bounds are the errors measured when the arithmetic was fixed, with a margin
of 2.5x to 5x for another sample: sincos 1.6e-7 / 2.0e-7 -> 5e-7; one step
4.3e-7 (observation) and 2.3e-6 (reward) -> 2e-6 and 1e-5; twenty steps 4.1e-6
and 7.5e-6 -> 2e-5 and 4e-5."""
import numpy as np


G, M, L, DT, MAX_SPEED, MAX_TORQUE = 10.0, 1.0, 1.0, 0.05, 8.0, 2.0


def angle_normalize(x):
    return ((x + np.pi) % (2 * np.pi)) - np.pi


def step_f64(th, thdot, action):
    """gym 0.17.2's ``PendulumEnv.step`` in float64, vectorised; the angle is
    left unwrapped: new th, new thdot, observation, reward."""
    u = np.clip(action, -MAX_TORQUE, MAX_TORQUE)
    costs = angle_normalize(th)**2 + .1 * thdot**2 + .001 * (u**2)
    newthdot = thdot + (-3 * G / (2 * L) * np.sin(th + np.pi) +
                        3. / (M * L**2) * u) * DT
    newth = th + newthdot * DT
    newthdot = np.clip(newthdot, -MAX_SPEED, MAX_SPEED)
    obs = np.stack([np.cos(newth), np.sin(newth), newthdot], axis=-1)
    return newth, newthdot, obs, -costs


def test_twin_sincos_against_float64():
    from garage_amd.envs import PendulumEnv
    pi, half = PendulumEnv.PI, PendulumEnv.HALF_PI
    assert float(PendulumEnv.TWO_PI) == 2.0 * float(pi)
    th = np.linspace(-float(pi), float(pi), 2000001).astype(np.float32)
    th[0], th[-1] = -pi, pi
    th = np.concatenate([th, [half, -half, np.nextafter(half, np.float32(9)),
                              np.nextafter(-half, np.float32(-9)),
                              np.float32(0)]]).astype(np.float32)
    assert np.abs(th).max() == pi
    sn, cs = PendulumEnv.sincos(th)
    assert sn.dtype == cs.dtype == np.float32
    t64 = th.astype(np.float64)
    es = float(np.abs(sn - np.sin(t64)).max())
    ec = float(np.abs(cs - np.cos(t64)).max())
    print('max |twin - float64|: sin {:.3e} cos {:.3e}'.format(es, ec))
    assert es <= 5e-7 and ec <= 5e-7
    assert (np.abs(sn) <= 1).all() and (np.abs(cs) <= 1).all()
    # a scalar goes the same way
    s1, c1 = PendulumEnv.sincos(th[12345])
    assert np.float32(s1) == sn[12345] and np.float32(c1) == cs[12345]


def _sample(rng, m, speed):
    from garage_amd.envs import PendulumEnv
    pi = PendulumEnv.PI
    th = np.clip(rng.uniform(-np.pi, np.pi, m).astype(np.float32), -pi, pi)
    thd = rng.uniform(-speed, speed, m).astype(np.float32)
    return th, thd


def test_twin_step_against_the_float64_equations():
    from garage_amd.envs import PendulumEnv
    rng = np.random.RandomState(0)
    m = 200000
    th, thd = _sample(rng, m, 8.0)
    a = rng.uniform(-3, 3, m).astype(np.float32)
    new, obs, rew = PendulumEnv.advance(np.stack([th, thd], axis=-1), a)
    assert new.dtype == obs.dtype == rew.dtype == np.float32
    assert new.shape == (m, 2) and obs.shape == (m, 3) and rew.shape == (m, )
    th64, thd64, a64 = (x.astype(np.float64) for x in (th, thd, a))
    nth, nthd, want_obs, want_rew = step_f64(th64, thd64, a64)
    eo = float(np.abs(obs - want_obs).max())
    er = float(np.abs(rew - want_rew).max())
    print('one step, max |twin - float64|: obs {:.3e} reward {:.3e}'.format(
        eo, er))
    assert eo <= 2e-6
    assert er <= 1e-5
    # the state stays in its box, exactly
    assert (np.abs(new[:, 0]) <= PendulumEnv.PI).all()
    assert (np.abs(new[:, 1]) <= np.float32(8.0)).all()
    # the wrapped angle is the float64 one modulo 2 pi (compared on the circle)
    d = angle_normalize(new[:, 0].astype(np.float64) - nth)
    assert np.abs(d).max() <= 2e-6
    # every branch is in the sample
    v = thd64 + (15.0 * np.sin(th64) + 3.0 * np.clip(a64, -2, 2)) * DT
    branches = {
        'wrap down': nth >= np.pi, 'wrap up': nth < -np.pi,
        'speed clipped low': v < -8, 'speed clipped high': v > 8,
        'torque clipped low': a < -2, 'torque clipped high': a > 2,
        'sine folded high': th > PendulumEnv.HALF_PI,
        'sine folded low': th < -PendulumEnv.HALF_PI,
    }
    for name, hit in branches.items():
        assert int(hit.sum()) >= 100, (name, int(hit.sum()))
    assert (new[v < -8, 1] == -8).all() and (new[v > 8, 1] == 8).all()


def test_twin_twenty_steps_against_float64():
    """From the reset range, the same actions on both sides.  Not longer: the
    upright equilibrium amplifies a difference by e^(sqrt(15) t)."""
    from garage_amd.envs import PendulumEnv
    rng = np.random.RandomState(1)
    m, T = 100000, 20
    th, thd = _sample(rng, m, 1.0)
    state = np.stack([th, thd], axis=-1)
    th64, thd64 = th.astype(np.float64), thd.astype(np.float64)
    eo = er = 0.0
    for t in range(T):
        a = rng.uniform(-3, 3, m).astype(np.float32)
        state, obs, rew = PendulumEnv.advance(state, a)
        th64, thd64, want_obs, want_rew = step_f64(th64, thd64,
                                                   a.astype(np.float64))
        eo = max(eo, float(np.abs(obs - want_obs).max()))
        er = max(er, float(np.abs(rew - want_rew).max()))
        assert (np.abs(state[:, 0]) <= PendulumEnv.PI).all()
        assert (np.abs(state[:, 1]) <= np.float32(8.0)).all()
    print('20 steps, max |twin - float64|: obs {:.3e} reward {:.3e}'.format(
        eo, er))
    assert eo <= 2e-5
    assert er <= 4e-5


def test_twin_episode_is_all_timeouts_and_in_the_declared_boxes():
    from garage_amd._dtypes import StepType
    from garage_amd.envs import PendulumEnv
    env = PendulumEnv(seed=3, env_id=4, max_episode_length=7)
    assert env.spec.action_space.low.tolist() == [-2.0]
    assert env.spec.action_space.high.tolist() == [2.0]
    assert env.spec.observation_space.high.tolist() == [1.0, 1.0, 8.0]
    assert env.spec.observation_space.low.tolist() == [-1.0, -1.0, -8.0]
    rng = np.random.RandomState(2)
    for ep in range(3):
        obs, info = env.reset()
        assert info == {} and obs.dtype == np.float32 and obs.shape == (3, )
        for t in range(7):
            es = env.step(rng.uniform(-3, 3, 1).astype(np.float32))
            assert es.observation.dtype == np.float32
            assert env.spec.observation_space.contains(es.observation)
            assert es.reward <= 0 and isinstance(es.reward, np.float32)
            want = (StepType.TIMEOUT if t == 6 else
                    StepType.FIRST if t == 0 else StepType.MID)
            assert es.step_type == want
    assert env.resets == 3
