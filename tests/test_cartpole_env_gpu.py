"""``CartPoleVecEnv`` on the GPU: its reset and step kernels against the numpy
twin (``garage_amd.envs.CartPoleEnv``) bit for bit on either side of each
limit, the procedures it shares with the other seeded state-vector kinds
(``_state_env_bodies.py``, on the row ``CARTPOLE`` of ``_state_env_kinds.py``),
the ``NormalizedVecEnv`` statistics inside the launch, and learning."""
import numpy as np
import pytest
import torch

import _state_env_bodies as bodies
import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import _bits, _mask, _np
from _state_env_kinds import CARTPOLE

pytestmark = pytest.mark.gpu


def test_reset_and_step_kernels_equal_the_twin_bit_for_bit():
    from garage_amd.envs import (CartPoleEnv, CartPoleVecEnv,
                                 cartpole_reset_draw)
    n, P, seed, id0 = 70, 30, 9, 1000
    f = np.float32
    env = CartPoleVecEnv(n, max_episode_length=P, seed=seed, env_id0=id0)
    assert env.obs_dim == 4 and env.act_width == 1
    assert env.env_info_specs == {}
    env.reset_all()
    first = np.stack([cartpole_reset_draw(seed, id0 + i, 0) for i in range(n)])
    assert np.array_equal(_bits(_np(env.obs)[:, :4]), _bits(first))
    assert np.array_equal(_bits(env.get_state()), _bits(first))
    assert np.array_equal(_np(env._resets), np.ones(n))
    # env_id0 shifts the stream: member i here is member i + 7 of a batch that
    # starts 7 ids earlier
    other = CartPoleVecEnv(n, max_episode_length=P, seed=seed, env_id0=id0 - 7)
    other.reset_all()
    assert np.array_equal(_bits(other.get_state()[7:]), _bits(first[:-7]))

    # states on either side of each limit (one fp32 step), zeros, random ones
    xl, tl = CartPoleEnv.X_LIMIT, CartPoleEnv.THETA_LIMIT
    edge = []
    for lim, col in ((xl, 0), (tl, 2)):
        for sign in (1, -1):
            for v in (np.nextafter(lim, f(0)), lim, np.nextafter(lim, f(9))):
                s = np.zeros(4, np.float32)
                s[col] = sign * v  # xd = thd = 0: the step keeps x and theta
                edge.append(s)
    rng = np.random.RandomState(3)
    box = np.array([2.4, 3.0, 0.21, 3.5])
    states = (rng.uniform(-1, 1, (n, 4)) * box).astype(np.float32)
    states[:len(edge)] = np.stack(edge)
    states[len(edge)] = 0.0
    act = torch.zeros(n, 4, device=env.device)
    seen_done = set()
    for action in (0, 1, 2):  # anything but 1 pushes left
        env.set_state(states)
        assert np.array_equal(_bits(_np(env.obs)[:, :4]), _bits(states))
        env._t.zero_()
        act[:, 0] = float(action)
        env.step_all(act)
        want, done = CartPoleEnv.advance(states, action == 1)
        assert np.array_equal(_bits(_np(env.next_obs)[:, :4]), _bits(want))
        assert np.array_equal(_bits(env.get_state()), _bits(want))
        assert np.array_equal(_np(env.reward), np.ones(n, np.float32))
        assert np.array_equal(_np(env.step_type), np.where(done, 2, 0))
        # x and theta stay where they were put: past the limit is done, on it
        # or below is not
        k = len(edge)
        assert done[:k].tolist() == [False, False, True] * 4
        seen_done.update(done[k:].tolist())
    assert seen_done == {False, True}
    # mixed actions, and the step counter: MID, then TIMEOUT at P whatever done
    mixed = rng.randint(0, 2, n)
    act[:, 0] = torch.from_numpy(mixed.astype(np.float32))
    env.set_state(states)
    env._t.fill_(5)
    env.step_all(act)
    want, done = CartPoleEnv.advance(states, mixed == 1)
    assert np.array_equal(_bits(_np(env.next_obs)[:, :4]), _bits(want))
    assert np.array_equal(_np(env.step_type), np.where(done, 2, 1))
    env._t.fill_(P - 1)
    env.set_state(states)
    env.step_all(act)
    assert np.array_equal(_np(env.step_type), np.full(n, 3))

    # reset_where: only the masked members, only their counters; a second
    # reset of the same member draws another state
    env.advance()
    before = _np(env.obs).copy()
    env.hold()
    flags = (np.arange(n) % 3 == 0)
    flags[-1] = True  # the last member (partial last workgroup)
    env.reset_where(_mask(flags, env.device))
    after = _np(env.next_obs)[:, :4]
    second = np.stack([cartpole_reset_draw(seed, id0 + i, 1) for i in range(n)])
    assert np.array_equal(_bits(after[flags]), _bits(second[flags]))
    assert np.array_equal(_bits(after[~flags]), _bits(before[~flags, :4]))
    assert np.array_equal(_np(env._resets), 1 + flags.astype(np.int32))
    assert np.array_equal(_np(env._t)[flags], np.zeros(flags.sum()))
    assert (_np(env._t)[~flags] == P).all()
    assert np.array_equal(_bits(env.get_state()[flags]), _bits(second[flags]))
    assert np.array_equal(_bits(env.get_state()[~flags]), _bits(want[~flags]))
    assert not (second[flags] == first[flags]).all(axis=1).any()
    with pytest.raises(ValueError, match='set_state'):
        env.set_state(np.zeros((n, 3)))


# the shared procedures, for this row
@kinds.cases(CARTPOLE)
def test_one_launch_rollout_equals_python_driven_steps(case):
    bodies.one_launch_rollout_equals_python_driven_steps(CARTPOLE, case)


def test_one_launch_rollout_replays_on_the_host_twin():
    bodies.one_launch_rollout_replays_on_the_host_twin(CARTPOLE)


def test_device_batch_equals_a_host_batch_of_the_twins():
    bodies.device_batch_equals_a_host_batch_of_the_twins(CARTPOLE)


def test_pickled_sampler_continues_identically():
    bodies.pickled_sampler_continues_identically(CARTPOLE)


def test_normalized_cartpole_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    a discrete action space has no rescale, so each call's first steps stay one
    launch; native against Python-driven steps, two calls in a row."""
    for a in h.normalized_statistics_inside_the_launch(
            CARTPOLE, 70, (70 * 30, 70 * 30 + 17)):
        assert {2} <= h._ending_types(a) <= {2, 3}
        # normalised: not the raw states, and rewards no longer all 1
        assert not np.array_equal(a.rewards, np.ones_like(a.rewards))


LEARN_BATCH = 8192  # 0.5 s; 2048 and 4096 pass the same assertions


def test_ppo_learns_cartpole_on_the_device():
    """The assertions and optimizer settings of
    test_cartpole_ppo_learns_through_the_host_env_adapter, with the device
    batch in place of 16 host envs."""
    from garage_amd.algos import PPO
    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy,
                                     GaussianMLPValueFunction)
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    n, P = 256, 200
    torch.manual_seed(0)
    np.random.seed(0)
    env = CartPoleVecEnv(n, max_episode_length=P, seed=1)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
    vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(64, 64))
    sampler = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                            worker_class=GpuVecWorker, seed=1,
                            worker_args=dict(n_envs=n))
    algo = PPO(env_spec=env.spec, policy=pol, value_function=vf,
               sampler=sampler,
               policy_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), pol,
                   max_optimization_epochs=10, minibatch_size=64),
               vf_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), vf,
                   max_optimization_epochs=10, minibatch_size=64),
               discount=0.99, gae_lambda=0.95, center_adv=True)
    returns = []
    for itr in range(12):
        eps = sampler.obtain_samples(itr, LEARN_BATCH, None)
        lens = np.asarray(eps.lengths)
        assert int(lens.sum()) >= LEARN_BATCH and lens.max() <= P
        returns.append(float(algo._train_once(itr, eps)))
    print('cartpole returns', np.round(returns, 1).tolist())
    assert np.isfinite(returns).all()
    assert returns[0] < 40
    assert max(returns[-3:]) > 2.0 * returns[0], returns
