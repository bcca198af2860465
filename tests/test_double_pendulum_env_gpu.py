"""``DoublePendulumVecEnv`` on the GPU: the procedures it shares with the other
seeded state-vector kinds (``_state_env_bodies.py``, on the row
``DOUBLE_PENDULUM`` of ``_state_env_kinds.py``), ``NormalizedVecEnv``'s action
rescale in front of it, and learning.

The first device task with a continuous action AND a termination that depends
on the dynamics: with ``max_episode_length`` 7 an episode ends TERMINAL (the tip
fell to ``y <= 1``) or TIMEOUT, both inside a launch of 24 steps, and each is
followed by a reset inside the launch."""
import numpy as np
import pytest
import torch

import _state_env_bodies as bodies
import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import TERMINAL, TIMEOUT, _bits, _np, _same
from _state_env_kinds import DOUBLE_PENDULUM

pytestmark = pytest.mark.gpu
P = DOUBLE_PENDULUM.P


# the shared procedures, for this row
@pytest.mark.parametrize('P', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 65])
def test_reset_and_step_kernels_equal_the_twin_bit_for_bit(n, P):
    bodies.reset_and_step_kernels_equal_the_twin_bit_for_bit(DOUBLE_PENDULUM,
                                                             n, P)


@kinds.cases(DOUBLE_PENDULUM)
def test_one_launch_rollout_equals_python_driven_steps(case):
    bodies.one_launch_rollout_equals_python_driven_steps(DOUBLE_PENDULUM, case)


def test_one_launch_rollout_replays_on_the_host_twin():
    bodies.one_launch_rollout_replays_on_the_host_twin(DOUBLE_PENDULUM)


def test_device_batch_equals_a_host_batch_of_the_twins():
    bodies.device_batch_equals_a_host_batch_of_the_twins(DOUBLE_PENDULUM)


def test_pickled_sampler_continues_identically():
    bodies.pickled_sampler_continues_identically(DOUBLE_PENDULUM)


def test_fragment_worker_fragments_join_up():
    bodies.fragment_worker_fragments_join_up(DOUBLE_PENDULUM)


def test_population_members_equal_lone_workers_and_their_statistics():
    bodies.population_members_equal_lone_workers_and_their_statistics(
        DOUBLE_PENDULUM)


def test_one_cem_epoch_on_statistics():
    bodies.one_cem_epoch_on_statistics(DOUBLE_PENDULUM)


def test_normalized_double_pendulum_rescales_the_push():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    the push bounds are finite, so the policy's actions are rescaled to them in
    a launch of their own and the rollout takes per-step launches; native
    against Python-driven steps, two calls in a row."""
    from garage_amd.envs import DoublePendulumEnv, double_pendulum_reset_draw
    n = 40
    wrap = h.normalized(normalize_obs=True, normalize_reward=True,
                        obs_alpha=0.05, reward_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = h.make(DOUBLE_PENDULUM, (64, 64), n=n, native=native, wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((n * 2 * P, n * 2 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert np.isfinite(a.rewards).all()
        assert h._ending_types(a) == {TERMINAL, TIMEOUT}
    # what the wrapped env was stepped with: two steps into an episode (none
    # ends that early) its state is the twin's after the rescaled (and so
    # clipped) recorded actions
    k = 2
    for native in (True, False):
        s, w = h.make(DOUBLE_PENDULUM, (64, 64), n=n, native=native, wrap=wrap)
        w._start()
        b = w._alloc_buffers(n * P)
        if native:
            assert w._native_steps(b, 0, k)
        else:
            for col in range(k):
                w._step(b, col)
        torch.cuda.synchronize()
        assert (_np(w.env._env._resets) == 1).all()
        policy_actions = _np(b['act'])[:, :k, 0]
        pushes = h.rescaled(policy_actions, -1.0, 1.0)
        assert (np.abs(pushes) <= 1).all()
        state = np.stack([double_pendulum_reset_draw(21, 3 + i, 0)
                          for i in range(n)])
        for t in range(k):
            state, _, _, done = DoublePendulumEnv.advance(state, pushes[:, t])
            assert not done.any()
        assert np.array_equal(_bits(w.env._env.get_state()), _bits(state))
        # ... and not the twin's after the policy's own actions
        other = np.stack([double_pendulum_reset_draw(21, 3 + i, 0)
                          for i in range(n)])
        for t in range(k):
            other, _, _, _ = DoublePendulumEnv.advance(other,
                                                       policy_actions[:, t])
        assert not np.array_equal(_bits(other), _bits(state))


# -- learning ---------------------------------------------------------------------
PPO_ITERS = 20


def _ppo_returns(seed, iters=PPO_ITERS, init_std=1.0, minibatch=1024,
                 discount=0.99):
    """Average return per iteration of PPO on 1024 envs: Gaussian MLP(64, 64)
    policy (output layer at zero, so that every seed starts from the zero-mean
    policy) and value function, P = 100, at least 32 steps per env and
    iteration, Adam at 2.5e-3 for 10 epochs."""
    from garage_amd.algos import PPO
    from garage_amd.envs import DoublePendulumVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    n, length = 1024, 100
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = DoublePendulumVecEnv(n, max_episode_length=length, seed=1 + seed)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(64, 64), init_std=init_std,
                            output_w_init=torch.nn.init.zeros_)
    vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(64, 64))
    sampler = GpuVecSampler(pol, env, max_episode_length=length, n_workers=1,
                            worker_class=GpuVecWorker, seed=1 + seed,
                            worker_args=dict(n_envs=n))
    algo = PPO(env_spec=env.spec, policy=pol, value_function=vf,
               sampler=sampler,
               policy_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), pol,
                   max_optimization_epochs=10, minibatch_size=minibatch),
               vf_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), vf,
                   max_optimization_epochs=10, minibatch_size=minibatch),
               discount=discount, gae_lambda=0.95, center_adv=True)
    returns, terminated = [], []
    for itr in range(iters):
        eps = sampler.obtain_samples(itr, n * 32, None)
        lens = np.asarray(eps.lengths)
        assert lens.max() <= length and lens.sum() >= n * 32
        terminated.append(float((lens < length).mean()))
        returns.append(float(algo._train_once(itr, eps)))
    return returns, terminated


# Measured on an MI355X (DESIGN.md section 7 has every iteration), seeds 0 .. 2,
# (returns[0], max(returns[-3:])) -> improvement:
#   0: (48.4, 860.1) -> 811.7    1: (48.2, 896.7) -> 848.5
#   2: (48.0, 896.7) -> 848.7
# margin = half the smallest improvement seen (811.7); returns[0] of the three
# seeds lie within 0.4 of each other.  The test runs seed 0, whose run repeats
# exactly on a given build.  (936 = 100 steps at 9.36 is the ceiling.)
PPO_MARGIN = 405.8


def test_ppo_learns_the_double_pendulum_on_the_device():
    """The first learning run over real terminations: GAE bootstraps across
    TIMEOUT and not across TERMINAL, and the untrained policy (std 1, pushes of
    up to 500 N) drops the rods within 3 .. 16 steps."""
    returns, terminated = _ppo_returns(0)
    print('double pendulum returns', np.round(returns, 1).tolist())
    print('share of episodes shorter than P', np.round(terminated, 2).tolist())
    assert np.isfinite(returns).all()
    assert terminated[0] == 1.0  # every untrained episode falls
    assert max(returns[-3:]) - returns[0] > PPO_MARGIN, returns
