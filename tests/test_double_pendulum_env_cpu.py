"""The inverted double pendulum on a cart as a device env, the parts that need
no GPU: the fp32 twin (``garage_amd.envs.DoublePendulumEnv``, the arithmetic
``include/garage_amd.h`` fixes) against a float64 restatement of the same scheme
(same substeps, clips and wraps; ``np.sin``, ``np.cos``, ``np.linalg.solve``),
the physics of that restatement, the Philox reset draws against a pure-Python
Philox4x32-10, episode semantics, the ctypes mirror of
``ga_double_pendulum_env`` against the header and the argument errors of the
entry points.

The bounds on |twin - float64| are 4x the worst error measured when the
arithmetic was fixed (the restatement is the yardstick; the factor covers states
the samples miss -- the dynamics are unstable, so this is not a tight
constant).  Measured, observation / reward:
  one step from 4096 reset states, zero action    3.7e-7 / 1.2e-6
  five steps from them                            2.1e-6 / 1.2e-6
  one step from the grid of 225 000 states        1.6e-5 / 9.8e-6"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    m32 = 0xffffffff
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & m32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & m32)
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


STREAM = 7


def reset_draw_py(seed, env_id, counter):
    f = np.float32
    key = (seed & 0xffffffff, seed >> 32)
    w = (philox4x32_10((env_id & 0xffffffff, counter, 0, STREAM << 16), key) +
         philox4x32_10((env_id & 0xffffffff, counter, 1, STREAM << 16), key))
    out = []
    for j in range(6):
        u = (f(w[j] >> 8) + f(0.5)) * f(2.0**-24)
        out.append(f(-0.1) + f(0.2) * u)
    return np.asarray(out, dtype=np.float32)


def test_reset_draws_equal_a_pure_python_philox():
    from garage_amd.envs import DoublePendulumEnv, double_pendulum_reset_draw
    draws = {}
    for seed in (0, (7 << 32) | 11):
        for env_id in (0, 1, 1 << 31):
            for counter in (0, 1, (1 << 32) - 1):
                got = double_pendulum_reset_draw(seed, env_id, counter)
                want = reset_draw_py(seed, env_id, counter)
                assert got.dtype == np.float32 and got.shape == (6, )
                assert got.tobytes() == want.tobytes(), (seed, env_id, counter)
                assert (np.abs(got) <= np.float32(0.1)).all()
                draws[(seed, env_id, counter)] = got.tobytes()
    # another seed, env id or counter: another state; six distinct words
    assert len(set(draws.values())) == len(draws) == 18
    assert len(set(reset_draw_py(0, 0, 0).tolist())) == 6
    # the key's high word counts
    assert double_pendulum_reset_draw(11, 1, 1).tobytes() != draws[
        ((7 << 32) | 11, 1, 1)]
    # the constants are the issue's, each rounded once
    for got, want in zip((DoublePendulumEnv.D1, DoublePendulumEnv.D2,
                          DoublePendulumEnv.D3, DoublePendulumEnv.D4,
                          DoublePendulumEnv.D5, DoublePendulumEnv.D6,
                          DoublePendulumEnv.F1, DoublePendulumEnv.F2),
                         (18.9, 3.78, 1.26, 2.016, 0.756, 0.504, 37.0818,
                          12.3606)):
        assert got == np.float32(want) and isinstance(got, np.float32)
    # the twin starts its episodes there, and the counter advances
    for i in (0, 3, 69):
        env = DoublePendulumEnv(seed=5, env_id=37 + i)
        first, info = env.reset()
        assert info == {} and first.dtype == np.float32
        assert np.array_equal(env.state, double_pendulum_reset_draw(5, 37 + i, 0))
        assert first.tobytes() == DoublePendulumEnv.observe(env.state).tobytes()
        env.reset()
        assert np.array_equal(env.state, double_pendulum_reset_draw(5, 37 + i, 1))


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


def test_double_pendulum_ctypes_struct_matches_the_header():
    from garage_amd import _lib
    cname, py = 'ga_double_pendulum_env', _lib.DoublePendulumEnv
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%d\\n", GA_ENV_DOUBLE_PENDULUM);',
             'printf("{0} %zu\\n", sizeof({0}));'.format(cname)]
    want = ['{}'.format(_lib.ENV_DOUBLE_PENDULUM),
            '{} {}'.format(cname, ctypes.sizeof(py))]
    for field, ftype in py._fields_:
        lines.append('printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                     'sizeof((({0}*)0)->{1}));'.format(cname, field))
        want.append('{}.{} {} {}'.format(cname, field,
                                         getattr(py, field).offset,
                                         ctypes.sizeof(ftype)))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe],
                       check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == want
    assert _lib.ENV_DOUBLE_PENDULUM == 6
    assert _lib.load().ga_abi_version() == 5


def test_double_pendulum_argument_errors_without_a_gpu():
    from garage_amd import _lib
    from garage_amd.envs import DoublePendulumEnv, DoublePendulumVecEnv
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)

    def env(kind=_lib.ENV_DOUBLE_PENDULUM, **kw):
        e = _lib.DoublePendulumEnv(n=4, max_episode_length=5, state=addr,
                                   t=addr, resets=addr)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(_lib.env_ref(kind, e))

    def reset(e, ldo=12):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=12):
        _lib.call('ga_env_step', e, addr, 1, None, addr, ldo, addr, addr, None)

    def record(e, ldo=12):
        rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5,
                              reward=addr, step_type=addr, next_obs=addr,
                              ldo=ldo, obs_dim=11, ep_t=addr, rew_buf=addr,
                              st_buf=addr, tail_buf=addr, lastobs_buf=addr,
                              done=addr, step_eps=addr, step_samples=addr)
        _lib.call('ga_env_step_record', e, C.byref(rec), None, addr, 1, addr,
                  None)

    for fn in (reset, step, record):
        for field in ('state', 't', 'resets'):
            with pytest.raises(_lib.GarageAmdError, match='null env state'):
                fn(env(**{field: None}))
        for bad in (0, 65536):
            with pytest.raises(_lib.GarageAmdError,
                               match='max_episode_length'):
                fn(env(max_episode_length=bad))
        with pytest.raises(_lib.GarageAmdError, match='bad env size'):
            fn(env(n=0))
        with pytest.raises(_lib.GarageAmdError, match='unknown env kind 7'):
            fn(env(kind=7))
    # observation rows narrower than 11
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(env(), ldo=10)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(env(), ldo=10)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        record(env(), ldo=10)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_double_pendulum_reset_draw', 0, 0, 0, None)
    for bad in (None, float('inf'), 0, 65536):
        with pytest.raises(ValueError):
            DoublePendulumVecEnv(4, max_episode_length=bad)
        with pytest.raises(ValueError):
            DoublePendulumEnv(max_episode_length=bad)


def test_rollout_env_steps_takes_the_double_pendulum_kind_as_continuous():
    """With rescale arguments the kind passes the "continuous action space"
    check a discrete env fails, and fails the next one (a rollout of more steps
    than the buffer holds), before any device call."""
    from garage_amd import _lib
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)
    desc = _lib.MlpDesc()
    head = _lib.HeadArgs(col=0, Tcap=4)
    rec = _lib.RecordArgs()
    norm = _lib.NormArgs(act_low=addr, act_high=addr, scaled_action=addr,
                         expected_action_scale=1.0, reward_scale=1.0)
    dp = _lib.DoublePendulumEnv(n=4, max_episode_length=5, state=addr, t=addr,
                                resets=addr)
    with pytest.raises(_lib.GarageAmdError,
                       match='steps exceed the rollout buffer'):
        _lib.call('ga_rollout_env_steps', C.byref(desc), addr, C.byref(head),
                  C.byref(_lib.env_ref(_lib.ENV_DOUBLE_PENDULUM, dp)),
                  C.byref(rec), addr, addr, C.byref(norm), None, None, 5, None)
