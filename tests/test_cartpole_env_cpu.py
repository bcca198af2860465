"""CartPole as a device env, the parts that need no GPU: the fp32 twin
(``garage_amd.envs.CartPoleEnv``, the arithmetic ``include/garage_amd.h`` fixes)
against the float64 cart-pole equations, step by step and over whole
episodes.

What every kind states the same way (reset draws against a
pure-Python Philox, the ctypes mirror of its struct, the argument errors of the
entry points) is in ``test_state_envs_cpu.py``, row ``cartpole``."""
import math

import numpy as np


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
