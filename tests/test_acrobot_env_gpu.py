"""``AcrobotVecEnv`` on the GPU: the procedures it shares with the other seeded
state-vector kinds (``_state_env_bodies.py``, on the row ``ACROBOT`` of
``_state_env_kinds.py``), ``NormalizedVecEnv``'s statistics inside the launch,
and learning.

The first device task with three action classes and a multi-stage integrator."""
import numpy as np
import pytest
import torch

import _state_env_bodies as bodies
import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import TIMEOUT
from _state_env_kinds import ACROBOT

pytestmark = pytest.mark.gpu
P = ACROBOT.P


# the shared procedures, for this row
@pytest.mark.parametrize('P', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 65])
def test_reset_and_step_kernels_equal_the_twin_bit_for_bit(n, P):
    bodies.reset_and_step_kernels_equal_the_twin_bit_for_bit(ACROBOT, n, P)


def test_one_step_from_the_whole_state_box_equals_the_twin():
    bodies.one_step_from_the_whole_state_box_equals_the_twin(ACROBOT)


@kinds.cases(ACROBOT)
def test_one_launch_rollout_equals_python_driven_steps(case):
    bodies.one_launch_rollout_equals_python_driven_steps(ACROBOT, case)


def test_one_launch_rollout_replays_on_the_host_twin():
    bodies.one_launch_rollout_replays_on_the_host_twin(ACROBOT)


def test_device_batch_equals_a_host_batch_of_the_twins():
    bodies.device_batch_equals_a_host_batch_of_the_twins(ACROBOT)


def test_pickled_sampler_continues_identically():
    bodies.pickled_sampler_continues_identically(ACROBOT)


def test_fragment_worker_fragments_join_up():
    bodies.fragment_worker_fragments_join_up(ACROBOT)


def test_population_members_equal_lone_workers_and_their_statistics():
    bodies.population_members_equal_lone_workers_and_their_statistics(ACROBOT)


def test_one_cem_epoch_on_statistics():
    bodies.one_cem_epoch_on_statistics(ACROBOT)


def test_normalized_acrobot_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    a discrete action space has no rescale, so each call's first steps stay one
    launch; native against Python-driven steps, two calls in a row."""
    n = 70
    for a in h.normalized_statistics_inside_the_launch(
            ACROBOT, n, (n * 2 * P, n * 2 * P + 17)):
        assert np.isfinite(a.rewards).all()
        assert h._ending_types(a) == {TIMEOUT}
        # normalised: the rewards are no longer all -1
        assert len(np.unique(a.rewards)) > 5


# -- learning ---------------------------------------------------------------------
PPO_ITERS = 10


def _ppo_returns(seed, iters=PPO_ITERS, minibatch=4096, discount=0.99):
    """Average return per iteration of PPO on 1024 envs: categorical
    MLP(64, 64) policy and an MLP(64, 64) value function, Acrobot-v1's own
    limit of 500 steps, at least 250 steps per env and iteration, Adam at
    2.5e-3 for 10 epochs (the settings of the CartPole learning test, with
    minibatches sized to the larger batch)."""
    from garage_amd.algos import PPO
    from garage_amd.envs import AcrobotVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy,
                                     GaussianMLPValueFunction)
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    n, length = 1024, 500
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = AcrobotVecEnv(n, max_episode_length=length, seed=1 + seed)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
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
        eps = sampler.obtain_samples(itr, n * 250, None)
        lens = np.asarray(eps.lengths)
        assert lens.max() <= length and lens.sum() >= n * 250
        terminated.append(float((lens < length).mean()))
        returns.append(float(algo._train_once(itr, eps)))
    return returns, terminated


# Measured on an MI355X, seeds 0 .. 2, returns per iteration:
#   0: -499.7 -500.0 -485.8 -321.5 -243.3 -206.5 -194.5 -192.4 -191.1 -195.2
#   1: -479.3 -435.8 -299.6 -256.3 -224.1 -201.5 -191.1 -187.8 -190.6 -188.0
#   2: -500.0 -500.0 -491.1 -340.5 -260.5 -216.8 -196.8 -190.5 -189.8 -188.9
# (returns[0], max(returns[-3:])) -> improvement:
#   0: (-499.7, -191.1) -> 308.6    1: (-479.3, -187.8) -> 291.5
#   2: (-500.0, -188.9) -> 311.1
# margin = half the smallest improvement seen (291.5).  The test runs seed 0,
# whose run repeats exactly on a given build (1 .. 2 s).  Under the untrained
# policy 0 .. 25 % of the episodes swing up before the limit; from the fourth
# iteration on every episode does.
PPO_MARGIN = 145.7


def test_ppo_learns_acrobot_on_the_device():
    """The first learning run over a sparse reward and three classes: -1 per
    step until the goal, so all the signal is where episodes end, GAE
    bootstraps across TIMEOUT and not across TERMINAL, and the untrained
    policy almost never reaches the goal."""
    returns, terminated = _ppo_returns(0)
    print('acrobot returns', np.round(returns, 1).tolist())
    print('share of episodes shorter than 500', np.round(terminated, 3).tolist())
    assert np.isfinite(returns).all()
    assert returns[0] < -450 and terminated[0] < 0.5
    assert max(returns[-3:]) - returns[0] > PPO_MARGIN, returns
