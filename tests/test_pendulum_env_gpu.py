"""``PendulumVecEnv`` on the GPU: its reset and step kernels against the numpy
twin (``garage_amd.envs.PendulumEnv``) bit for bit with a count of the branches
taken, the procedures it shares with the other seeded state-vector kinds
(``_state_env_bodies.py``, on the row ``PENDULUM`` of ``_state_env_kinds.py``),
``NormalizedVecEnv``'s action rescale in front of it, and learning."""
import numpy as np
import pytest
import torch

import _state_env_bodies as bodies
import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import TIMEOUT, _bits, _mask, _np, _same
from _state_env_kinds import PENDULUM

pytestmark = pytest.mark.gpu
P = PENDULUM.P


def _first_obs(states):
    from garage_amd.envs import PendulumEnv
    sn, cs = PendulumEnv.sincos(states[:, 0])
    return np.stack([cs, sn, states[:, 1]], axis=-1).astype(np.float32)


def test_reset_and_step_kernels_equal_the_twin_bit_for_bit():
    from garage_amd.envs import (PendulumEnv, PendulumVecEnv,
                                 pendulum_reset_draw)
    n, P, seed, id0, T = 70, 30, 9, 1000, 40
    f = np.float32
    pi, half = PendulumEnv.PI, PendulumEnv.HALF_PI
    env = PendulumVecEnv(n, max_episode_length=P, seed=seed, env_id0=id0)
    assert env.obs_dim == 3 and env.act_width == 1
    assert env.env_info_specs == {}
    assert env.spec.action_space.low.tolist() == [-2.0]
    assert env.spec.action_space.high.tolist() == [2.0]
    env.reset_all()
    first = np.stack([pendulum_reset_draw(seed, id0 + i, 0) for i in range(n)])
    assert np.array_equal(_bits(env.get_state()), _bits(first))
    assert np.array_equal(_bits(_np(env.obs)[:, :3]), _bits(_first_obs(first)))
    assert np.array_equal(_np(env._resets), np.ones(n))
    # env_id0 shifts the stream
    other = PendulumVecEnv(n, max_episode_length=P, seed=seed, env_id0=id0 - 7)
    other.reset_all()
    assert np.array_equal(_bits(other.get_state()[7:]), _bits(first[:-7]))

    # scripted starts: th = +-PI, +-HALF_PI and their neighbours, states that
    # wrap either way at the first step, speeds that clip either way; the rest
    # random over the whole box
    rng = np.random.RandomState(3)
    states = np.stack([np.clip(rng.uniform(-np.pi, np.pi, n).astype(f), -pi,
                               pi),
                       rng.uniform(-8, 8, n).astype(f)], axis=-1)
    edge = [(pi, 0), (-pi, 0), (pi, 8), (-pi, -8), (pi, -8), (-pi, 8),
            (half, 0), (-half, 0), (np.nextafter(half, f(9)), 1),
            (np.nextafter(-half, f(-9)), -1), (f(3.1), 6), (f(-3.1), -6),
            (f(1.0), 8), (f(-1.0), -8), (f(0), 0), (np.nextafter(pi, f(0)), 0)]
    states[:len(edge)] = np.asarray(edge, dtype=f)
    env.set_state(states)
    assert np.array_equal(_bits(env.get_state()), _bits(states))
    assert np.array_equal(_bits(_np(env.obs)[:, :3]),
                          _bits(_first_obs(states)))
    with pytest.raises(ValueError, match='set_state'):
        env.set_state(np.zeros((n, 3)))
    with pytest.raises(ValueError, match=r'\[-PI, PI\]'):
        bad = states.copy()
        bad[5, 0] = np.nextafter(pi, f(9))
        env.set_state(bad)
    env._t.zero_()
    # scripted torques, a third of them beyond +-2; the twins are 70 objects
    actions = rng.uniform(-3.5, 3.5, (T, n)).astype(f)
    actions[0, :4] = [2.0, -2.0, 5.0, -5.0]
    twins = [PendulumEnv(seed=seed, env_id=id0 + i, max_episode_length=P)
             for i in range(n)]
    for i, twin in enumerate(twins):
        twin.state = states[i].copy()
    act = torch.zeros(n, 4, device=env.device)
    seen = dict(down=0, up=0, low=0, high=0)
    for t in range(T):
        before = env.get_state()
        act[:, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        steps = [twin.step(actions[t, i:i + 1]) for i, twin in enumerate(twins)]
        want_obs = np.stack([s.observation for s in steps])
        want_rew = np.asarray([s.reward for s in steps], dtype=f)
        want_state = np.stack([twin.state for twin in twins])
        assert np.array_equal(_bits(_np(env.next_obs)[:, :3]),
                              _bits(want_obs)), t
        assert np.array_equal(_bits(_np(env.reward)), _bits(want_rew)), t
        assert np.array_equal(_bits(env.get_state()), _bits(want_state)), t
        # FIRST, MID, and TIMEOUT from step P on (nothing resets the env here)
        assert np.array_equal(_np(env.step_type),
                              [int(s.step_type) for s in steps]), t
        assert int(steps[0].step_type) == (0 if t == 0 else
                                           1 if t < P - 1 else TIMEOUT)
        assert (np.abs(want_state[:, 0]) <= pi).all()
        assert (np.abs(want_state[:, 1]) <= 8).all()
        # which branches this step took (from the states on either side)
        moved = want_state[:, 0].astype(np.float64) - before[:, 0]
        seen['down'] += int((moved < -3).sum())
        seen['up'] += int((moved > 3).sum())
        seen['low'] += int((want_state[:, 1] == -8).sum())
        seen['high'] += int((want_state[:, 1] == 8).sum())
        env.advance()
    print('branches taken', seen)
    assert min(seen.values()) >= 2, seen
    # the step that reaches P is TIMEOUT, whatever the state
    env._t.fill_(P - 1)
    env.step_all(act)
    assert np.array_equal(_np(env.step_type), np.full(n, TIMEOUT))
    want_state, _, _ = PendulumEnv.advance(np.stack([tw.state for tw in twins]),
                                           actions[T - 1])

    # reset_where: only the masked members, only their counters; a second
    # reset of the same member draws another state
    env.advance()
    before = _np(env.obs).copy()
    env.hold()
    flags = (np.arange(n) % 3 == 0)
    flags[-1] = True  # the last member (partial last workgroup)
    env.reset_where(_mask(flags, env.device))
    after = _np(env.next_obs)[:, :3]
    second = np.stack([pendulum_reset_draw(seed, id0 + i, 1) for i in range(n)])
    assert np.array_equal(_bits(after[flags]),
                          _bits(_first_obs(second)[flags]))
    assert np.array_equal(_bits(after[~flags]), _bits(before[~flags, :3]))
    assert np.array_equal(_np(env._resets), 1 + flags.astype(np.int32))
    assert np.array_equal(_np(env._t)[flags], np.zeros(flags.sum()))
    assert (_np(env._t)[~flags] == P).all()
    assert np.array_equal(_bits(env.get_state()[flags]), _bits(second[flags]))
    assert np.array_equal(_bits(env.get_state()[~flags]),
                          _bits(want_state[~flags]))
    assert not (second[flags] == first[flags]).all(axis=1).any()


# the shared procedures, for this row
@kinds.cases(PENDULUM)
def test_one_launch_rollout_equals_python_driven_steps(case):
    bodies.one_launch_rollout_equals_python_driven_steps(PENDULUM, case)


def test_one_launch_rollout_replays_on_the_host_twin():
    bodies.one_launch_rollout_replays_on_the_host_twin(PENDULUM)


def test_device_batch_equals_a_host_batch_of_the_twins():
    bodies.device_batch_equals_a_host_batch_of_the_twins(PENDULUM)


def test_pickled_sampler_continues_identically():
    bodies.pickled_sampler_continues_identically(PENDULUM)


def test_population_members_equal_lone_workers_and_their_statistics():
    bodies.population_members_equal_lone_workers_and_their_statistics(PENDULUM)


def test_one_cem_epoch_on_statistics():
    bodies.one_cem_epoch_on_statistics(PENDULUM)


def test_normalized_pendulum_rescales_the_torque():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    the torque bounds are finite, so the policy's actions are rescaled to them
    in a launch of their own and the rollout takes per-step launches; native
    against Python-driven steps, two calls in a row."""
    from garage_amd.envs import PendulumEnv, pendulum_reset_draw
    wrap = h.normalized(normalize_obs=True, normalize_reward=True,
                        obs_alpha=0.05, reward_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = h.make(PENDULUM, (64, 64), n=70, native=native, wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((70 * P, 70 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert np.isfinite(a.rewards).all()
        assert h._ending_types(a) == {TIMEOUT} and (a.lengths == P).all()
    # what the wrapped env was stepped with: seven steps into an episode its
    # state is the twin's after the rescaled (and so clipped) recorded actions
    k = 7
    for native in (True, False):
        s, w = h.make(PENDULUM, (64, 64), n=70, native=native, wrap=wrap)
        w._start()
        b = w._alloc_buffers(70 * P)
        if native:
            assert w._native_steps(b, 0, k)
        else:
            for col in range(k):
                w._step(b, col)
        torch.cuda.synchronize()
        policy_actions = _np(b['act'])[:, :k, 0]
        torques = h.rescaled(policy_actions, -2.0, 2.0)
        assert np.abs(policy_actions).max() > 1      # the clip had work to do
        assert (np.abs(torques) <= 2).all() and (np.abs(torques) == 2).any()
        state = np.stack([pendulum_reset_draw(21, 3 + i, 0) for i in range(70)])
        for t in range(k):
            state, _, _ = PendulumEnv.advance(state, torques[:, t])
        assert np.array_equal(_bits(w.env._env.get_state()), _bits(state))
        # ... and not the twin's after the policy's own actions
        other = np.stack([pendulum_reset_draw(21, 3 + i, 0) for i in range(70)])
        for t in range(k):
            other, _, _ = PendulumEnv.advance(other, policy_actions[:, t])
        assert not np.array_equal(_bits(other), _bits(state))


# -- learning ---------------------------------------------------------------------
# Measured on an MI355X (DESIGN.md section 7 has every iteration), seeds 0 .. 2,
# (returns[0], max(returns[-3:])) -> improvement:
#   0: (-1231.1, -177.9) -> 1053.2    1: (-1215.7, -198.7) -> 1017.0
#   2: (-1238.8, -187.7) -> 1051.1
# margin = half the smallest improvement seen (1017.0); returns[0] of the three
# seeds lie within 23.1 of each other (37.4 over seeds 0 .. 4), far below it.  The
# test runs seed 0, whose run repeats exactly on a given build.
PPO_MARGIN = 508.5


def test_ppo_learns_pendulum_on_the_device():
    """test_ppo_learns_cartpole_on_the_device's recipe with a Gaussian head:
    256 envs, P = 200, one episode per env and iteration, Adam at 2.5e-3 for 10
    epochs.  What differs: minibatches of 512 (51 200 samples per iteration),
    discount 0.9 (the cost is dense; with xavier output weights 0.99 gained
    260 .. 480 in 15 iterations over three seeds, 0.9 gained 970 .. 1300), and
    an output layer that starts at zero, so that every seed starts from the
    zero-mean policy's return of about -1230 (xavier output weights started
    at -1145 .. -1703, a spread larger than half the smallest gain)."""
    from garage_amd.algos import PPO
    from garage_amd.envs import PendulumVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    n, length = 256, 200
    torch.manual_seed(0)
    np.random.seed(0)
    env = PendulumVecEnv(n, max_episode_length=length, seed=1)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(64, 64),
                            output_w_init=torch.nn.init.zeros_)
    vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(64, 64))
    sampler = GpuVecSampler(pol, env, max_episode_length=length, n_workers=1,
                            worker_class=GpuVecWorker, seed=1,
                            worker_args=dict(n_envs=n))
    algo = PPO(env_spec=env.spec, policy=pol, value_function=vf,
               sampler=sampler,
               policy_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), pol,
                   max_optimization_epochs=10, minibatch_size=512),
               vf_optimizer=OptimizerWrapper(
                   (torch.optim.Adam, dict(lr=2.5e-3)), vf,
                   max_optimization_epochs=10, minibatch_size=512),
               discount=0.9, gae_lambda=0.95, center_adv=True)
    returns = []
    for itr in range(15):
        eps = sampler.obtain_samples(itr, n * length, None)
        lens = np.asarray(eps.lengths)
        assert len(lens) == n and (lens == length).all()
        returns.append(float(algo._train_once(itr, eps)))
    print('pendulum returns', np.round(returns, 1).tolist())
    assert np.isfinite(returns).all()
    assert max(returns[-3:]) - returns[0] > PPO_MARGIN, returns
