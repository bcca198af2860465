"""``CartPoleVecEnv`` on the GPU: the reset and step kernels against the numpy
twin (``garage_amd.envs.CartPoleEnv``) bit for bit, the one-launch rollout
against Python-driven steps, a replay on the twin and a host batch of twins, the
``NormalizedVecEnv`` statistics inside the launch, pickling, and learning."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT = 13  # csrc/prof.h: a whole rollout in one launch


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(flags, device):
    return torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(device)


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


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


def _make(hidden, options=None, n=48, P=30, native=True, wrap=None,
          env_seed=21, id0=3):
    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(5)
    env = CartPoleVecEnv(n, max_episode_length=P, seed=env_seed, env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hidden, **(options or {}))
    with torch.no_grad():  # gamma / beta (the buffer's tail) away from (1, 0)
        if pol.net.ln_off:
            lo = pol.net.ln_off[0]
            pol.net.params[lo:].add_(
                torch.randn_like(pol.net.params[lo:]) * 0.05)
    cls = (GpuVecWorker if native else
           type('PythonSteps', (_PythonSteps, GpuVecWorker), {}))
    s = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                      worker_class=cls, seed=2, worker_args=dict(n_envs=n))
    return s, s._workers[0]


def _same(a, b):
    assert np.array_equal(a.lengths, b.lengths)
    assert np.array_equal([int(s) for s in a.step_types],
                          [int(s) for s in b.step_types])
    for k in ('observations', 'last_observations', 'actions', 'rewards'):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert sorted(a.agent_infos) == sorted(b.agent_infos)
    for k in a.agent_infos:
        assert np.array_equal(_bits(a.agent_infos[k]),
                              _bits(b.agent_infos[k])), k
    assert sorted(a.env_infos) == sorted(b.env_infos) == []


def _ending_types(eps):
    ends = np.cumsum(eps.lengths) - 1
    return {int(eps.step_types[e]) for e in ends}


NUM = 3 * 48 * 30 // 2
_whole_a = {}


def _one_launch_rollout(hidden, options, launches):
    """The native rollout of a fresh sampler (its batch on the host) and the
    sampler, after checking the number of whole-rollout launches."""
    from garage_amd import _lib
    lib = _lib.load()
    s, w = _make(hidden, options)
    assert w._fused_ok()
    before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
    whole = w.rollout_samples(NUM).to_host()
    torch.cuda.synchronize()
    assert int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before == launches
    return whole, s


@pytest.mark.parametrize('hidden,options,launches', [
    ((64, 64), None, 1),
    ((64, 64), dict(hidden_nonlinearity=torch.relu,
                    layer_normalization=True), 1),
    ((32, 32, 32), None, 0),
], ids=['a-tanh-resident', 'b-relu-ln-resident', 'c-four-layers-streamed'])
def test_one_launch_rollout_equals_python_driven_steps(hidden, options,
                                                       launches):
    whole, _ = _one_launch_rollout(hidden, options, launches)
    if launches and options is None:
        _whole_a['batch'] = whole  # the replay test below reads the same batch
    _, wb = _make(hidden, options, native=False)
    stepped = wb.rollout_samples(NUM).to_host()
    _same(whole, stepped)
    assert int(whole.lengths.sum()) >= NUM and whole.lengths.max() <= 30
    assert np.isfinite(whole.agent_infos['prob']).all()
    assert set(np.unique(whole.actions)) == {0.0, 1.0}
    # both endings occur (the reset inside the launch is exercised)
    assert _ending_types(whole) == {2, 3}


def test_one_launch_rollout_replays_on_the_host_twin():
    """Case a's batch: every episode starts from the reset draw of its member
    and reset counter, and the twin stepped with the recorded actions gives the
    recorded observations, rewards, step types and length, bit for bit."""
    from garage_amd.envs import CartPoleEnv, cartpole_reset_draw
    whole = _whole_a.get('batch')
    if whole is None:
        whole, _ = _one_launch_rollout((64, 64), None, 1)
    n, P, seed, id0 = 48, 30, 21, 3
    starts = {}
    for i in range(n):
        for c in range(NUM // n):  # more resets than a member can have
            starts[cartpole_reset_draw(seed, id0 + i, c).tobytes()] = (i, c)
    off = np.concatenate([[0], np.cumsum(whole.lengths)])
    order, counters = [], {}
    for e, L in enumerate(whole.lengths):
        obs = whole.observations[off[e]:off[e + 1]]
        act = whole.actions[off[e]:off[e + 1]].reshape(-1)
        i, c = starts[np.ascontiguousarray(obs[0], np.float32).tobytes()]
        # a member's episodes come in the order of its resets
        assert counters.get(i, -1) + 1 == c
        counters[i] = c
        twin = CartPoleEnv(seed=seed, env_id=id0 + i, max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
        for t in range(L):
            assert np.array_equal(_bits(o), _bits(obs[t])), (e, t)
            es = twin.step(int(act[t]))
            o = es.observation
            assert np.float32(es.reward) == whole.rewards[off[e] + t]
            assert int(es.step_type) == int(whole.step_types[off[e] + t])
            assert (int(es.step_type) >= 2) == (t == L - 1)
        assert np.array_equal(_bits(o), _bits(whole.last_observations[e]))
        order.append(i)
    assert len(counters) == n  # every member finished an episode
    # the completion step of an episode is the sum of its member's lengths so
    # far; the batch is sorted by (completion step, member)
    done_at, keys = {}, []
    for e, L in enumerate(whole.lengths):
        i = order[e]
        done_at[i] = done_at.get(i, 0) + int(L)
        keys.append((done_at[i], i))
    assert keys == sorted(keys)


def test_device_batch_equals_a_host_batch_of_the_twins():
    """The same task behind ``HostVecEnv``: 48 ``CartPoleEnv`` objects with the
    batch's seed and member ids give the device batch's samples, bit for bit,
    over two calls (the second starts with a partial reset)."""
    from garage_amd.envs import CartPoleEnv, HostVecEnv

    def host(env):
        return HostVecEnv([CartPoleEnv(seed=env.seed, env_id=env.env_id0 + i,
                                       max_episode_length=30)
                           for i in range(env.n_envs)])

    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (_make((64, 64), id0=0),
                        _make((64, 64), id0=0, wrap=host))
    for itr in range(2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


def test_normalized_cartpole_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    a discrete action space has no rescale, so each call's first steps stay one
    launch; native against Python-driven steps, two calls in a row."""
    from garage_amd import _lib
    from garage_amd.envs import NormalizedVecEnv
    lib = _lib.load()

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                                obs_alpha=0.05, reward_alpha=0.05)

    out, counts = [], []
    for native in (True, False):
        s, w = _make((64, 64), n=70, native=native, wrap=wrap)
        assert w.env._act_low is None and w._fused_ok()
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((70 * 30, 70 * 30 + 17))])
        torch.cuda.synchronize()
        counts.append(int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before)
    assert counts == [2, 0]  # one whole-rollout launch per native call
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert {2} <= _ending_types(a) <= {2, 3}
        # normalised: not the raw states, and rewards no longer all 1
        assert not np.array_equal(a.rewards, np.ones_like(a.rewards))


def test_pickled_sampler_continues_identically():
    sa, _ = _make((64, 64))
    sa.obtain_samples(0, NUM, None)
    sb = pickle.loads(pickle.dumps(sa))
    assert np.array_equal(_np(sa._workers[0].env._resets),
                          _np(sb._workers[0].env._resets))
    for itr in (1, 2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


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
