"""The inverted double pendulum on a cart as a device env, the parts that need
no GPU: the fp32 twin (``garage_amd.envs.DoublePendulumEnv``, the arithmetic
``include/garage_amd.h`` fixes) against a float64 restatement of the same scheme
(same substeps, clips and wraps; ``np.sin``, ``np.cos``, ``np.linalg.solve``),
the physics of that restatement and episode semantics.

What every kind states the same way (reset draws against a
pure-Python Philox, the ctypes mirror of its struct, the argument errors of the
entry points) is in ``test_state_envs_cpu.py``, row ``double_pendulum``.

The bounds on |twin - float64| are 4x the worst error measured when the
arithmetic was fixed (the restatement is the yardstick; the factor covers states
the samples miss -- the dynamics are unstable, so this is not a tight
constant).  Measured, observation / reward:
  one step from 4096 reset states, zero action    3.7e-7 / 1.2e-6
  five steps from them                            2.1e-6 / 1.2e-6
  one step from the grid of 225 000 states        1.6e-5 / 9.8e-6"""
import numpy as np


M0, M1, M2, L1, L2, G = 10.5, 4.2, 4.2, 0.6, 0.6, 9.81
D1 = M0 + M1 + M2
D2 = (M1 / 2 + M2) * L1
D3 = M2 * L2 / 2
D4 = (M1 / 3 + M2) * L1**2
D5 = M2 * L1 * L2 / 2
D6 = M2 * L2**2 / 3
F1 = (M1 / 2 + M2) * L1 * G
F2 = M2 * L2 * G / 2
H, SUBSTEPS = 0.01, 5

# 4x the measured worst (module docstring)
ONE_STEP_OBS, ONE_STEP_REW = 4 * 3.7e-7, 4 * 1.2e-6
FIVE_STEPS_OBS, FIVE_STEPS_REW = 4 * 2.1e-6, 4 * 1.2e-6
GRID_OBS, GRID_REW = 4 * 1.6e-5, 4 * 9.8e-6


def mass_matrix(th1, th2):
    c1, c2, cd = np.cos(th1), np.cos(th2), np.cos(th1 - th2)
    d = np.empty(np.shape(th1) + (3, 3))
    d[..., 0, 0], d[..., 1, 1], d[..., 2, 2] = D1, D4, D6
    d[..., 0, 1] = d[..., 1, 0] = D2 * c1
    d[..., 0, 2] = d[..., 2, 0] = D3 * c2
    d[..., 1, 2] = d[..., 2, 1] = D5 * cd
    return d


def wrap64(th):
    return np.where(th >= np.pi, th - 2 * np.pi,
                    np.where(th < -np.pi, th + 2 * np.pi, th))


def step_f64(state, action):
    """One env step of the scheme in float64, vectorised over the leading axis:
    new state, observation, reward, y_tip."""
    x, th1, th2, xd, th1d, th2d = (state[..., j].astype(np.float64)
                                   for j in range(6))
    force = 500.0 * np.clip(np.asarray(action, dtype=np.float64), -1, 1)
    for _ in range(SUBSTEPS):
        s1, s2, sd = np.sin(th1), np.sin(th2), np.sin(th1 - th2)
        r = np.stack([force + D2 * s1 * th1d**2 + D3 * s2 * th2d**2,
                      F1 * s1 - D5 * sd * th2d**2,
                      F2 * s2 + D5 * sd * th1d**2], axis=-1)
        qdd = np.linalg.solve(mass_matrix(th1, th2), r[..., None])[..., 0]
        xd = np.clip(xd + H * qdd[..., 0], -100, 100)
        th1d = np.clip(th1d + H * qdd[..., 1], -100, 100)
        th2d = np.clip(th2d + H * qdd[..., 2], -100, 100)
        x = x + H * xd
        th1 = wrap64(th1 + H * th1d)
        th2 = wrap64(th2 + H * th2d)
    x_tip = x + L1 * np.sin(th1) + L2 * np.sin(th2)
    y_tip = L1 * np.cos(th1) + L2 * np.cos(th2)
    w1, w2 = th1d, th2d - th1d
    reward = (10 - (0.01 * x_tip**2 + (y_tip - 2)**2) -
              (0.001 * w1**2 + 0.005 * w2**2))
    zero = np.zeros_like(x)
    obs = np.stack([x, np.sin(th1), np.sin(th2 - th1), np.cos(th1),
                    np.cos(th2 - th1), np.clip(xd, -10, 10),
                    np.clip(w1, -10, 10), np.clip(w2, -10, 10), zero, zero,
                    zero], axis=-1)
    new = np.stack([x, th1, th2, xd, th1d, th2d], axis=-1)
    return new, obs, reward, y_tip


def energy(state):
    v = state[..., 3:]
    d = mass_matrix(state[..., 1], state[..., 2])
    return (0.5 * np.einsum('...i,...ij,...j', v, d, v) +
            F1 * np.cos(state[..., 1]) + F2 * np.cos(state[..., 2]))


def _reset_states(m, seed=4):
    from garage_amd.envs import double_pendulum_reset_draw
    return np.stack([double_pendulum_reset_draw(seed, i, i % 3)
                     for i in range(m)])


def _errors(obs, rew, want_obs, want_rew):
    return (float(np.abs(obs - want_obs).max()),
            float(np.abs(rew - want_rew).max()))


def _done_share(done, y_tip):
    """Compares ``done`` wherever the restatement is clear of the threshold;
    returns the share of cases left out."""
    clear = np.abs(y_tip - 1) > 1e-4
    assert np.array_equal(done[clear], (y_tip <= 1)[clear])
    return 1.0 - float(clear.mean())


def test_twin_against_float64_from_reset_states_under_zero_action():
    from garage_amd.envs import DoublePendulumEnv
    m = 4096
    state = _reset_states(m)
    s64 = state.astype(np.float64)
    zero = np.zeros(m, dtype=np.float32)
    worst = []
    for t in range(5):
        state, obs, rew, done = DoublePendulumEnv.advance(state, zero)
        assert state.dtype == obs.dtype == rew.dtype == np.float32
        assert state.shape == (m, 6) and obs.shape == (m, 11)
        assert rew.shape == done.shape == (m, ) and done.dtype == np.bool_
        s64, want_obs, want_rew, y_tip = step_f64(s64, zero)
        worst.append(_errors(obs, rew, want_obs, want_rew))
        # five is safe: nothing falls within five steps of such a start
        assert not done.any() and (y_tip > 1 + 1e-4).all()
        assert (obs[:, 8:] == 0).all()
    one = worst[0]
    five = (max(w[0] for w in worst), max(w[1] for w in worst))
    print('one step, max |twin - float64|: obs {:.3e} reward {:.3e}'.format(
        *one))
    print('five steps, max |twin - float64|: obs {:.3e} reward {:.3e}'.format(
        *five))
    assert one[0] <= ONE_STEP_OBS and one[1] <= ONE_STEP_REW
    assert five[0] <= FIVE_STEPS_OBS and five[1] <= FIVE_STEPS_REW


def _grid():
    from garage_amd.envs import PendulumEnv
    f = np.float32
    pi, half = float(PendulumEnv.PI), float(PendulumEnv.HALF_PI)
    e = 5e-4
    ang = np.asarray([-pi, -pi + e, -2.0, -half - e, -half + e, -0.7, -0.05,
                      0.0, 0.03, 0.9, half - e, half + e, 2.5, pi - e, pi],
                     dtype=f)
    ang = np.clip(ang, -PendulumEnv.PI, PendulumEnv.PI)
    x = np.asarray([0.0, 0.7], dtype=f)
    xd = np.asarray([-12.0, -3.0, 0.0, 10.5], dtype=f)
    th1d = np.asarray([-12.0, -1.0, 0.0, 4.0, 12.0], dtype=f)
    th2d = np.asarray([-12.0, -2.0, 0.0, 5.0, 12.0], dtype=f)
    act = np.asarray([-1.5, -1.0, 0.0, 0.3, 1.0], dtype=f)
    g = np.meshgrid(x, ang, ang, xd, th1d, th2d, act, indexing='ij')
    cols = [c.reshape(-1) for c in g]
    return np.stack(cols[:6], axis=-1).astype(f), cols[6].astype(f)


def test_twin_against_float64_on_a_grid():
    from garage_amd.envs import DoublePendulumEnv, PendulumEnv
    state, act = _grid()
    assert (np.abs(state[:, 1:3]) <= PendulumEnv.PI).all()
    new, obs, rew, done = DoublePendulumEnv.advance(state, act)
    n64, want_obs, want_rew, y_tip = step_f64(state.astype(np.float64), act)
    eo, er = _errors(obs, rew, want_obs, want_rew)
    print('grid of {} states, max |twin - float64|: obs {:.3e} reward {:.3e}'
          .format(len(act), eo, er))
    left_out = _done_share(done, y_tip)
    print('done left uncompared: {:.4%}; done in {:.1%}'.format(
        left_out, done.mean()))
    assert eo <= GRID_OBS and er <= GRID_REW
    assert left_out <= 0.01
    assert done.any() and not done.all()
    # the state stays in its box, and every clip of the observation is hit
    assert (np.abs(new[:, 1:3]) <= PendulumEnv.PI).all()
    assert np.isfinite(new).all() and np.isfinite(rew).all()
    for j in (5, 6, 7):
        assert (obs[:, j] == 10).any() and (obs[:, j] == -10).any(), j
        assert (np.abs(obs[:, j]) <= 10).all()
    assert (np.abs(obs[:, 1:5]) <= 1).all()
    # ... and both wraps of both angles were taken
    for j in (1, 2):
        moved = new[:, j].astype(np.float64) - state[:, j]
        assert (moved < -3).any() and (moved > 3).any(), j
    # the action is clipped: -1.5 steps as -1 does
    a, b = act == np.float32(-1.5), act == np.float32(-1.0)
    assert a.sum() == b.sum() > 0
    assert new[a].tobytes() == new[b].tobytes()


def test_twin_speed_guard_clips_at_100():
    from garage_amd.envs import DoublePendulumEnv
    f = np.float32
    state = np.asarray([[0, 0.3, -0.2, 99.99, 99.99, -99.99],
                        [0, 0.3, -0.2, -99.99, -99.99, 99.99]], dtype=f)
    new, obs, rew, _ = DoublePendulumEnv.advance(state, np.asarray([1, -1], f))
    assert np.isfinite(new).all() and np.isfinite(rew).all()
    assert (np.abs(new[:, 3:]) <= 100).all()
    assert new[0, 3] == 100 and new[1, 3] == -100
    assert (np.abs(new[:, 1:3]) <= np.float32(np.pi)).all()


def test_restatement_upright_is_a_fixed_point():
    s = np.zeros((1, 6))
    for _ in range(3):
        s, obs, rew, y_tip = step_f64(s, np.zeros(1))
        assert (s == 0).all() and y_tip[0] == L1 + L2
        assert abs(rew[0] - (10 - 0.8**2)) < 1e-12  # 9.36: the tip is at 1.2, not 2
        assert obs[0].tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]


def test_restatement_conserves_energy_and_falls_on_step_eight():
    s = np.asarray([[0, .05, -.03, 0, 0, 0]], dtype=np.float64)
    e0 = energy(s)[0]
    falls = []
    for t in range(8):
        s, _, _, y_tip = step_f64(s, np.zeros(1))
        drift = abs(energy(s)[0] - e0)
        print('step {} y_tip {:.4f} energy drift {:.4f}'.format(
            t + 1, y_tip[0], drift))
        assert drift < 0.1
        falls.append(bool(y_tip[0] <= 1))
    assert falls == [False] * 7 + [True]


def test_twin_episode_semantics():
    from garage_amd._dtypes import StepType
    from garage_amd.envs import DoublePendulumEnv
    f = np.float32
    fallen = np.asarray([0, 1.5, 1.5, 0, 0, 0], dtype=f)
    zero = np.zeros(1, dtype=f)
    env = DoublePendulumEnv(seed=3, env_id=4, max_episode_length=7)
    assert env.spec.observation_space.shape == (11, )
    assert env.spec.observation_space.flat_dim == 11
    assert np.isinf(env.spec.observation_space.low).all()
    assert np.isinf(env.spec.observation_space.high).all()
    assert env.spec.action_space.low.tolist() == [-1.0]
    assert env.spec.action_space.high.tolist() == [1.0]
    assert env.spec.max_episode_length == 7
    assert DoublePendulumEnv().max_episode_length == 1000
    # a zero-action episode from a reset: FIRST, MID ..., then TIMEOUT at 7 or
    # TERMINAL before (here they last 6 .. 17 steps)
    obs, info = env.reset()
    assert info == {} and obs.dtype == np.float32 and obs.shape == (11, )
    types = []
    for t in range(7):
        es = env.step(zero)
        assert es.observation.dtype == np.float32
        assert isinstance(es.reward, np.float32) and es.env_info == {}
        types.append(es.step_type)
        if es.step_type in (StepType.TERMINAL, StepType.TIMEOUT):
            break
    assert types[0] == StepType.FIRST
    assert all(s == StepType.MID for s in types[1:-1]) and len(types) >= 6
    assert types[-1] == (StepType.TIMEOUT if len(types) == 7 else
                         StepType.TERMINAL)
    # the terminating step carries its reward: that of the state it reaches
    env = DoublePendulumEnv(max_episode_length=5)
    env.reset()
    env.state = fallen.copy()
    es = env.step(zero)
    _, _, want_rew, done = DoublePendulumEnv.advance(fallen, zero[0])
    assert done and es.step_type == StepType.TERMINAL  # wins over FIRST
    assert es.reward == want_rew and 0 < es.reward < 10
    # max_episode_length 1: every step is a TIMEOUT, fallen or not
    env = DoublePendulumEnv(max_episode_length=1)
    env.reset()
    assert env.step(zero).step_type == StepType.TIMEOUT
    env.reset()
    env.state = fallen.copy()
    assert env.step(zero).step_type == StepType.TIMEOUT  # wins over TERMINAL
    # max_episode_length 2: FIRST then TIMEOUT; TERMINAL on the first step
    env = DoublePendulumEnv(max_episode_length=2)
    env.reset()
    assert env.step(zero).step_type == StepType.FIRST
    env.state = fallen.copy()
    assert env.step(zero).step_type == StepType.TIMEOUT
    env.reset()
    env.state = fallen.copy()
    assert env.step(zero).step_type == StepType.TERMINAL
    assert env.resets == 2
