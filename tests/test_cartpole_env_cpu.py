"""CartPole as a device env, the parts that need no GPU: the fp32 twin
(``garage_amd.envs.CartPoleEnv``, the arithmetic ``include/garage_amd.h`` fixes)
against the float64 cart-pole equations, the Philox reset draws against a
pure-Python Philox4x32-10, the ctypes mirror of ``ga_cartpole_env`` against the
header, and the argument errors of the entry points."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAVITY, M_CART, M_POLE, HALF_LEN, FORCE, TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
X_LIMIT, THETA_LIMIT = 2.4, 12 * 2 * math.pi / 360


def step_f64(state, action):
    """The classic equations in float64 (Barto, Sutton and Anderson; Euler step),
    vectorised over the leading axis: new states and ``done``."""
    x, x_dot, th, th_dot = (state[..., j] for j in range(4))
    force = np.where(np.asarray(action) == 1, FORCE, -FORCE)
    total = M_CART + M_POLE
    pml = M_POLE * HALF_LEN
    temp = (force + pml * th_dot**2 * np.sin(th)) / total
    th_acc = (GRAVITY * np.sin(th) - np.cos(th) * temp) / (
        HALF_LEN * (4.0 / 3.0 - M_POLE * np.cos(th)**2 / total))
    x_acc = temp - pml * th_acc * np.cos(th) / total
    new = np.stack([x + TAU * x_dot, x_dot + TAU * x_acc, th + TAU * th_dot,
                    th_dot + TAU * th_acc], axis=-1)
    done = (np.abs(new[..., 0]) > X_LIMIT) | (np.abs(new[..., 2]) > THETA_LIMIT)
    return new, done


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


STREAM_CARTPOLE = 5


def reset_draw_py(seed, env_id, counter):
    f = np.float32
    words = philox4x32_10((env_id & 0xffffffff, counter, 0,
                           STREAM_CARTPOLE << 16),
                          (seed & 0xffffffff, seed >> 32))
    out = []
    for w in words:
        u = (f(w >> 8) + f(0.5)) * f(2.0**-24)
        out.append(f(-0.05) + f(0.1) * u)
    return np.asarray(out, dtype=np.float32)


def test_twin_step_against_the_float64_equations():
    """One step from 20 000 seeded states of the reachable box, both actions.
    Measured when written (seed 0): max |twin - float64| = 2.13e-07 over all four
    state entries; the bound is 4x that (other seeds), and 1e-6 in any case."""
    from garage_amd.envs import CartPoleEnv
    rng = np.random.RandomState(0)
    m = 20000
    box = np.array([2.4, 3.0, 0.21, 3.5])
    states = (rng.uniform(-1, 1, (m, 4)) * box).astype(np.float32)
    worst = 0.0
    for action in (0, 1):
        got, got_done = CartPoleEnv.advance(states, action == 1)
        assert got.dtype == np.float32 and got.shape == (m, 4)
        want, want_done = step_f64(states.astype(np.float64),
                                   np.full(m, action))
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
        # `done` may differ only where the float64 state sits on a limit
        off = got_done != want_done
        margin = np.minimum(np.abs(np.abs(want[:, 0]) - X_LIMIT),
                            np.abs(np.abs(want[:, 2]) - THETA_LIMIT))
        assert (margin[off] < 1e-6).all()
    print('max |fp32 twin - float64| after one step: {:.3e}'.format(worst))
    measured = 2.13e-07
    assert worst < 4 * measured
    assert worst < 1e-6


def _episode_f64(start, actions, cap):
    s = start.astype(np.float64)
    for t in range(cap):
        s, done = step_f64(s, actions[t])
        if done:
            return t + 1
    return cap


def test_twin_episode_lengths_against_float64():
    """2000 random-action episodes from the Philox reset draws, capped at 200
    steps: the twin and float64 end at the same step in >= 99.5 % of them
    (measured when written: all 2000)."""
    from garage_amd._dtypes import StepType
    from garage_amd.envs import CartPoleEnv
    rng = np.random.RandomState(1)
    n_eps, cap = 2000, 200
    same, lengths = 0, []
    for ep in range(n_eps):
        env = CartPoleEnv(seed=11, env_id=ep, max_episode_length=cap)
        start, info = env.reset()
        assert info == {} and start.dtype == np.float32
        actions = rng.randint(0, 2, cap)
        for t in range(cap):
            es = env.step(actions[t])
            assert es.reward == 1.0
            if es.step_type in (StepType.TERMINAL, StepType.TIMEOUT):
                break
            assert es.step_type == (StepType.FIRST if t == 0 else
                                    StepType.MID)
        lengths.append(t + 1)
        same += (t + 1) == _episode_f64(start, actions, cap)
    lengths = np.asarray(lengths)
    print('equal lengths: {} of {}; mean {:.1f} min {} max {}'.format(
        same, n_eps, lengths.mean(), lengths.min(), lengths.max()))
    assert same >= 0.995 * n_eps
    # at max_episode_length = 30 both endings occur
    ends = set()
    for ep in range(200):
        env = CartPoleEnv(seed=11, env_id=ep, max_episode_length=30)
        env.reset()
        actions = rng.randint(0, 2, 30)
        for t in range(30):
            es = env.step(actions[t])
            if es.step_type >= 2:
                ends.add(int(es.step_type))
                assert (t + 1 == 30) == (es.step_type == StepType.TIMEOUT)
                break
    assert ends == {int(StepType.TERMINAL), int(StepType.TIMEOUT)}


def test_reset_draws_equal_a_pure_python_philox():
    from garage_amd.envs import CartPoleEnv, cartpole_reset_draw
    rng = np.random.RandomState(2)
    cases = [(0, 0, 0), (0, 1, 0), (0, 0, 1), ((7 << 32) | 11, 5, 3),
             (3, (1 << 32) + 2, 9)]
    cases += [(int(rng.randint(0, 1 << 30)) << 20 | int(rng.randint(1 << 20)),
               int(rng.randint(0, 1 << 20)), int(rng.randint(0, 1 << 16)))
              for _ in range(400)]
    draws = []
    for seed, env_id, counter in cases:
        got = cartpole_reset_draw(seed, env_id, counter)
        want = reset_draw_py(seed, env_id, counter)
        assert got.dtype == np.float32 and got.shape == (4, )
        assert got.tobytes() == want.tobytes(), (seed, env_id, counter)
        assert ((got > -0.05) & (got < 0.05)).all()
        draws.append(got)
    # another env id or another counter: another state
    assert not np.array_equal(draws[0], draws[1])
    assert not np.array_equal(draws[0], draws[2])
    assert len({d.tobytes() for d in draws}) == len(draws)
    # roughly uniform over the interval
    flat = np.concatenate(draws)
    assert abs(flat.mean()) < 0.005 and flat.min() < -0.045 < 0.045 < flat.max()
    # env_id0 shifts the stream: member i of a batch with env_id0 = k is member
    # i + k of a batch with env_id0 = 0 (the batch draws env_id0 + i)
    k = 37
    for i in (0, 3, 69):
        a = CartPoleEnv(seed=5, env_id=k + i)
        b = CartPoleEnv(seed=5, env_id=i)
        first, _ = a.reset()
        assert np.array_equal(first, cartpole_reset_draw(5, i + k, 0))
        assert not np.array_equal(first, b.reset()[0])
        # the counter advances with every reset
        assert np.array_equal(a.reset()[0], cartpole_reset_draw(5, i + k, 1))


def test_cartpole_ctypes_struct_matches_the_header():
    from garage_amd import _lib
    cname, py = 'ga_cartpole_env', _lib.CartPoleEnv
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%d\\n", GA_ENV_CARTPOLE);',
             'printf("{0} %zu\\n", sizeof({0}));'.format(cname)]
    want = ['{}'.format(_lib.ENV_CARTPOLE),
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
    assert _lib.ENV_CARTPOLE == 4
    assert _lib.load().ga_abi_version() == 5


def test_cartpole_argument_errors_without_a_gpu():
    from garage_amd import _lib
    from garage_amd.envs import CartPoleEnv, CartPoleVecEnv
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)

    def env(**kw):
        e = _lib.CartPoleEnv(n=4, max_episode_length=5, state=addr, t=addr,
                             resets=addr)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(_lib.env_ref(_lib.ENV_CARTPOLE, e))

    def reset(e, ldo=4):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=4):
        _lib.call('ga_env_step', e, addr, 1, None, addr, ldo, addr, addr, None)

    def record(e):
        rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5,
                              reward=addr, step_type=addr, next_obs=addr,
                              ldo=4, obs_dim=4, ep_t=addr, rew_buf=addr,
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
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(env(), ldo=3)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(env(), ldo=3)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_cartpole_reset_draw', 0, 0, 0, None)
    for bad in (None, float('inf'), 0, 65536):
        with pytest.raises(ValueError):
            CartPoleVecEnv(4, max_episode_length=bad)
        with pytest.raises(ValueError):
            CartPoleEnv(max_episode_length=bad)
