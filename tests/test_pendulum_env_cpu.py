"""Pendulum as a device env, the parts that need no GPU: the fp32 twin
(``garage_amd.envs.PendulumEnv``, the arithmetic ``include/garage_amd.h`` fixes)
against the float64 equations of gym 0.17's ``pendulum.py``, the Philox reset
draws against a pure-Python Philox4x32-10, the ctypes mirror of
``ga_pendulum_env`` against the header, and the argument errors of the entry
points.

The bounds are the errors measured when the arithmetic was fixed, with a margin
of 2.5x to 5x for another sample: sincos 1.6e-7 / 2.0e-7 -> 5e-7; one step
4.3e-7 (observation) and 2.3e-6 (reward) -> 2e-6 and 1e-5; twenty steps 4.1e-6
and 7.5e-6 -> 2e-5 and 4e-5."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


STREAM_PENDULUM = 6


def reset_draw_py(seed, env_id, counter):
    f = np.float32
    w = philox4x32_10((env_id & 0xffffffff, counter, 0, STREAM_PENDULUM << 16),
                      (seed & 0xffffffff, seed >> 32))
    u0 = (f(w[0] >> 8) + f(0.5)) * f(2.0**-24)
    u1 = (f(w[1] >> 8) + f(0.5)) * f(2.0**-24)
    th = (-f(3.141592653589793)) + f(6.283185307179586) * u0
    thd = f(-1.0) + f(2.0) * u1
    return np.asarray([th, thd], dtype=np.float32)


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


def test_reset_draws_equal_a_pure_python_philox():
    from garage_amd.envs import PendulumEnv, pendulum_reset_draw
    rng = np.random.RandomState(2)
    cases = [(0, 0, 0), (0, 1, 0), (0, 0, 1), ((7 << 32) | 11, 5, 3),
             (3, (1 << 32) + 2, 9)]
    cases += [(int(rng.randint(0, 1 << 30)) << 20 | int(rng.randint(1 << 20)),
               int(rng.randint(0, 1 << 20)), int(rng.randint(0, 1 << 16)))
              for _ in range(400)]
    assert any(seed >> 32 for seed, _, _ in cases)
    draws = []
    for seed, env_id, counter in cases:
        got = pendulum_reset_draw(seed, env_id, counter)
        want = reset_draw_py(seed, env_id, counter)
        assert got.dtype == np.float32 and got.shape == (2, )
        assert got.tobytes() == want.tobytes(), (seed, env_id, counter)
        assert abs(got[0]) <= PendulumEnv.PI and abs(got[1]) < 1
        draws.append(got)
    # another env id or another counter: another state; the key's high word counts
    assert not np.array_equal(draws[0], draws[1])
    assert not np.array_equal(draws[0], draws[2])
    assert len({d.tobytes() for d in draws}) == len(draws)
    assert not np.array_equal(pendulum_reset_draw(11, 5, 3), draws[3])
    # roughly uniform over the two intervals
    d = np.stack(draws)
    assert abs(d[:, 0].mean()) < 0.3 and d[:, 0].min() < -2.8 < 2.8 < d[:, 0].max()
    assert abs(d[:, 1].mean()) < 0.1 and d[:, 1].min() < -0.9 < 0.9 < d[:, 1].max()
    # the twin starts its episodes there, and the counter advances
    k = 37
    for i in (0, 3, 69):
        a = PendulumEnv(seed=5, env_id=k + i)
        first, _ = a.reset()
        assert np.array_equal(a.state, pendulum_reset_draw(5, i + k, 0))
        sn, cs = PendulumEnv.sincos(a.state[0])
        assert first.tobytes() == np.array([cs, sn, a.state[1]],
                                           np.float32).tobytes()
        a.reset()
        assert np.array_equal(a.state, pendulum_reset_draw(5, i + k, 1))


def test_pendulum_ctypes_struct_matches_the_header():
    from garage_amd import _lib
    cname, py = 'ga_pendulum_env', _lib.PendulumEnv
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%d\\n", GA_ENV_PENDULUM);',
             'printf("{0} %zu\\n", sizeof({0}));'.format(cname)]
    want = ['{}'.format(_lib.ENV_PENDULUM),
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
    assert _lib.ENV_PENDULUM == 5
    assert _lib.load().ga_abi_version() == 5


def test_pendulum_argument_errors_without_a_gpu():
    from garage_amd import _lib
    from garage_amd.envs import PendulumEnv, PendulumVecEnv
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)

    def env(kind=_lib.ENV_PENDULUM, **kw):
        e = _lib.PendulumEnv(n=4, max_episode_length=5, state=addr, t=addr,
                             resets=addr)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(_lib.env_ref(kind, e))

    def reset(e, ldo=4):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=4):
        _lib.call('ga_env_step', e, addr, 1, None, addr, ldo, addr, addr, None)

    def record(e, ldo=4):
        rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5,
                              reward=addr, step_type=addr, next_obs=addr,
                              ldo=ldo, obs_dim=3, ep_t=addr, rew_buf=addr,
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
    # observation rows narrower than 3
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(env(), ldo=2)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(env(), ldo=2)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        record(env(), ldo=2)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_pendulum_reset_draw', 0, 0, 0, None)
    for bad in (None, float('inf'), 0, 65536):
        with pytest.raises(ValueError):
            PendulumVecEnv(4, max_episode_length=bad)
        with pytest.raises(ValueError):
            PendulumEnv(max_episode_length=bad)


def test_rollout_env_steps_takes_the_pendulum_kind_as_continuous():
    """With rescale arguments the pendulum kind passes the "continuous action
    space" check a discrete env fails, and fails the next one (a rollout of
    more steps than the buffer holds), before any device call."""
    from garage_amd import _lib
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)
    desc = _lib.MlpDesc()
    head = _lib.HeadArgs(col=0, Tcap=4)
    rec = _lib.RecordArgs()
    norm = _lib.NormArgs(act_low=addr, act_high=addr, scaled_action=addr,
                         expected_action_scale=1.0, reward_scale=1.0)

    def steps(ref, n_steps):
        _lib.call('ga_rollout_env_steps', C.byref(desc), addr, C.byref(head),
                  ref, C.byref(rec), addr, addr, C.byref(norm), None, None,
                  n_steps, None)

    pend = _lib.PendulumEnv(n=4, max_episode_length=5, state=addr, t=addr,
                            resets=addr)
    cart = _lib.CartPoleEnv(n=4, max_episode_length=5, state=addr, t=addr,
                            resets=addr)
    with pytest.raises(_lib.GarageAmdError, match='continuous action space'):
        steps(C.byref(_lib.env_ref(_lib.ENV_CARTPOLE, cart)), 5)
    with pytest.raises(_lib.GarageAmdError,
                       match='steps exceed the rollout buffer'):
        steps(C.byref(_lib.env_ref(_lib.ENV_PENDULUM, pend)), 5)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind 7'):
        steps(C.byref(_lib.env_ref(7, pend)), 5)
