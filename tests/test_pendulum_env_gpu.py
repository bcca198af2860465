"""``PendulumVecEnv`` on the GPU: the reset and step kernels against the numpy
twin (``garage_amd.envs.PendulumEnv``) bit for bit, the one-launch rollout
against Python-driven steps for every step kernel, a replay on the twin and a
host batch of twins, ``NormalizedVecEnv``'s action rescale in front of it,
pickling, a population of Gaussian policies with its statistics, and CEM.

Shapes: 48 envs are three workgroups of 16, 70 leave a ragged last one; with
episodes of 30 steps and about 2.5 n P samples per call every env is reset
twice inside the launch."""
import pickle
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE = 13, 14  # csrc/prof.h
TIMEOUT = 3


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(flags, device):
    return torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(device)


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


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


N, P = 48, 30
NUM = 5 * N * P // 2  # 2.5 n P: three episodes per env, two resets in the launch


def _make(hidden, options=None, n=N, native=True, wrap=None, env_seed=21,
          id0=3):
    from garage_amd.envs import PendulumVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(5)
    env = PendulumVecEnv(n, max_episode_length=P, seed=env_seed, env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, **(options or {}))
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


_whole_a = {}


def _one_launch_rollout(hidden, options, launches):
    """The native rollout of a fresh sampler (its batch on the host) after
    checking the whole-rollout launches of kinds (13, 14)."""
    from garage_amd import _lib
    lib = _lib.load()
    s, w = _make(hidden, options)
    assert w._fused_ok()
    kinds = (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)
    before = [int(lib.ga_launch_count(k)) for k in kinds]
    whole = w.rollout_samples(NUM).to_host()
    torch.cuda.synchronize()
    got = tuple(int(lib.ga_launch_count(k)) - b for k, b in zip(kinds, before))
    assert got == launches
    return whole


@pytest.mark.parametrize('hidden,options,launches', [
    ((64, 64), None, (1, 0)),
    ((64, 64), dict(hidden_nonlinearity=torch.relu,
                    layer_normalization=True), (1, 0)),
    ((32, 32, 32), None, (0, 0)),
    ((320, ), None, (0, 1)),
], ids=['a-tanh-resident', 'b-relu-ln-resident', 'c-four-layers-streamed',
        'd-320-wide'])
def test_one_launch_rollout_equals_python_driven_steps(hidden, options,
                                                       launches):
    whole = _one_launch_rollout(hidden, options, launches)
    if hidden == (64, 64) and options is None:
        _whole_a['batch'] = whole  # the replay test below reads the same batch
    _, wb = _make(hidden, options, native=False)
    stepped = wb.rollout_samples(NUM).to_host()
    _same(whole, stepped)
    # never done: every episode runs its P steps and ends in a TIMEOUT
    assert len(whole.lengths) == 3 * N and (whole.lengths == P).all()
    assert _ending_types(whole) == {TIMEOUT}
    assert (np.asarray([int(s) for s in whole.step_types]) != 2).all()
    assert np.isfinite(whole.agent_infos['mean']).all()
    assert np.isfinite(whole.observations).all()
    # the batch keeps the policy's own actions, not the clipped torques
    assert np.abs(whole.actions).max() > 2
    assert (whole.rewards <= 0).all() and len(np.unique(whole.rewards)) > NUM // 2


def test_one_launch_rollout_replays_on_the_host_twin():
    """Case a's batch: every episode starts from the reset draw of its member
    and reset counter, and the twin stepped with the recorded actions gives the
    recorded observations, rewards and step types, bit for bit."""
    from garage_amd.envs import PendulumEnv, pendulum_reset_draw
    whole = _whole_a.get('batch')
    if whole is None:
        whole = _one_launch_rollout((64, 64), None, (1, 0))
    seed, id0 = 21, 3
    starts = {}
    for i in range(N):
        for c in range(4):  # more resets than a member has in this batch
            draw = pendulum_reset_draw(seed, id0 + i, c)
            starts[_first_obs(draw[None])[0].tobytes()] = (i, c)
    off = np.concatenate([[0], np.cumsum(whole.lengths)])
    order, counters = [], {}
    for e, L in enumerate(whole.lengths):
        obs = whole.observations[off[e]:off[e + 1]]
        act = whole.actions[off[e]:off[e + 1]]
        i, c = starts[np.ascontiguousarray(obs[0], np.float32).tobytes()]
        # a member's episodes come in the order of its resets
        assert counters.get(i, -1) + 1 == c
        counters[i] = c
        twin = PendulumEnv(seed=seed, env_id=id0 + i, max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
        for t in range(L):
            assert np.array_equal(_bits(o), _bits(obs[t])), (e, t)
            es = twin.step(act[t])
            o = es.observation
            assert (_bits(es.reward) == _bits(whole.rewards[off[e] + t])).all()
            assert int(es.step_type) == int(whole.step_types[off[e] + t])
            assert (int(es.step_type) == TIMEOUT) == (t == L - 1)
        assert np.array_equal(_bits(o), _bits(whole.last_observations[e]))
        order.append(i)
    assert counters == {i: 2 for i in range(N)}
    # the batch is sorted by (completion step, member): all end together
    assert order == list(range(N)) * 3


def test_device_batch_equals_a_host_batch_of_the_twins():
    """The same task behind ``HostVecEnv``: 48 ``PendulumEnv`` objects with the
    batch's seed and member ids give the device batch's samples, bit for bit,
    over two calls."""
    from garage_amd.envs import HostVecEnv, PendulumEnv

    def host(env):
        return HostVecEnv([PendulumEnv(seed=env.seed, env_id=env.env_id0 + i,
                                       max_episode_length=P)
                           for i in range(env.n_envs)])

    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (_make((64, 64), id0=0),
                        _make((64, 64), id0=0, wrap=host))
    for itr in range(2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


def _rescaled(a):
    """``NormalizedVecEnv``'s rescale of the policy's action to the torque box
    (``ga_action_rescale_f32``: fp32, one rounding per operation)."""
    f = np.float32
    a = np.asarray(a, dtype=f)
    slope = (f(0.5) * (f(2.0) - f(-2.0))) / f(1.0)
    v = f(-2.0) + (a + f(1.0)) * slope
    return np.clip(v, f(-2.0), f(2.0)).astype(f)


def test_normalized_pendulum_rescales_the_torque():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    the torque bounds are finite, so the policy's actions are rescaled to them
    in a launch of their own and the rollout takes per-step launches; native
    against Python-driven steps, two calls in a row."""
    from garage_amd.envs import NormalizedVecEnv, PendulumEnv, pendulum_reset_draw

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                                obs_alpha=0.05, reward_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = _make((64, 64), n=70, native=native, wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((70 * P, 70 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert np.isfinite(a.rewards).all()
        assert _ending_types(a) == {TIMEOUT} and (a.lengths == P).all()
    # what the wrapped env was stepped with: seven steps into an episode its
    # state is the twin's after the rescaled (and so clipped) recorded actions
    k = 7
    for native in (True, False):
        s, w = _make((64, 64), n=70, native=native, wrap=wrap)
        w._start()
        b = w._alloc_buffers(70 * P)
        if native:
            assert w._native_steps(b, 0, k)
        else:
            for col in range(k):
                w._step(b, col)
        torch.cuda.synchronize()
        policy_actions = _np(b['act'])[:, :k, 0]
        torques = _rescaled(policy_actions)
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


def test_pickled_sampler_continues_identically():
    sa, _ = _make((64, 64))
    sa.obtain_samples(0, NUM, None)
    sb = pickle.loads(pickle.dumps(sa))
    ea, eb = sa._workers[0].env, sb._workers[0].env
    for k in ('_state', '_t', '_resets'):
        assert np.array_equal(_np(getattr(ea, k)), _np(getattr(eb, k))), k
    assert _np(ea._resets).min() >= 3
    for itr in (1, 2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


# -- population -----------------------------------------------------------------
POP_SEED, POP_M, POP_G, POP_P, POP_NUM = 5, 3, 16, 12, 40
DISCOUNT = 0.99  # not exact in binary


def _pop_env(n, env_id0=0):
    from garage_amd.envs import PendulumVecEnv
    return PendulumVecEnv(n, max_episode_length=POP_P, seed=3, env_id0=env_id0)


def _pop_policy(spec):
    from garage_amd.policies import GaussianMLPPolicy
    return GaussianMLPPolicy(spec, hidden_sizes=(8, 8), learn_std=True)


def _member_vectors(pol, M):
    """Visibly different parameters per member, the log-std included."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.5 * rng.randn(M, base.size).astype(np.float32)
    vectors[:, 0] = np.log(0.5) + 0.3 * np.arange(M)
    return vectors.astype(np.float32)


def _population(**kw):
    from garage_amd.sampler import GpuPopulationSampler
    torch.manual_seed(1)
    env = _pop_env(POP_M * POP_G)
    pol = _pop_policy(env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=POP_M,
                               max_episode_length=POP_P, seed=POP_SEED, **kw)
    return pop, pol, _member_vectors(pol, POP_M)


def test_population_members_equal_lone_workers_and_their_statistics():
    """3 members x 16 raw Pendulum envs: each member's batch is the lone
    worker's of those envs, and ``obtain_statistics`` of an identically built
    sampler gives, per episode, the length, the undiscounted return
    ``log_performance`` computes (``episode_statistics``: bit-equal) and the
    discounted return of ``log_performance_host``'s fp64 recurrence (bit-equal;
    within one fp32 ulp of ``log_performance``'s fp32 scan) -- over rewards
    that are neither constant nor 0 / 1."""
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.envs import NormalizedVecEnv
    from garage_amd.functions import episode_statistics
    from garage_amd.sampler import GpuPopulationSampler, GpuVecWorker
    pop, pol, vectors = _population()
    batches = pop.obtain_samples(0, POP_NUM, pol.pack_members(vectors))
    assert len(batches) == POP_M
    for m in range(POP_M):
        got = batches[m].to_host()
        env = _pop_env(POP_G, env_id0=m * POP_G)
        lone = _pop_policy(env.spec)
        lone.set_flat_param_values(vectors[m])
        w = GpuVecWorker(seed=POP_SEED, max_episode_length=POP_P,
                         worker_number=0, n_envs=POP_G)
        w.update_agent(lone)
        w.update_env(env)
        _same(got, w.rollout_samples(POP_NUM).to_host())
        assert (got.lengths == POP_P).all() and got.lengths.sum() >= POP_NUM
        assert np.all(got.agent_infos['log_std'] == np.float32(vectors[m, 0]))
    a, b = batches[0].to_host(), batches[1].to_host()
    assert not np.array_equal(a.actions, b.actions)

    twin, tpol, _ = _population()
    stats = twin.obtain_statistics(0, POP_NUM, tpol.pack_members(vectors),
                                   DISCOUNT)
    assert len(stats) == POP_M
    assert twin.total_env_steps == pop.total_env_steps > 0
    for m in range(POP_M):
        st, host = stats[m], batches[m].to_host()
        assert isinstance(st, EpisodeStatistics) and st.success is None
        lengths = np.asarray(host.lengths, dtype=np.int64)
        assert np.array_equal(st.lengths, lengths)
        assert not st.terminated.any()
        und, scan, term, _ = episode_statistics(batches[m], DISCOUNT)
        assert not term.any()
        assert st.undiscounted_returns.tobytes() == und.tobytes(), m
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        want = []
        for s, L in zip(starts, lengths):
            ret = 0.0
            for x in host.rewards[s:s + L][::-1]:
                ret = float(x) + DISCOUNT * ret
            want.append(ret)
        want = np.asarray(want, dtype=np.float64)
        assert st.discounted_returns.tobytes() == want.tobytes(), m
        got32 = st.discounted_returns.astype(np.float32).astype(np.float64)
        ulp = np.spacing(np.abs(scan).astype(np.float32)).astype(np.float64)
        assert (np.abs(got32 - scan) <= ulp).all(), m
        # the sums really ran over distinct, non-integer rewards
        assert len(np.unique(host.rewards)) > len(host.rewards) // 2
        assert len(np.unique(st.undiscounted_returns)) == len(lengths)

    # normalize() rescales a bounded torque: the population launch has no rescale
    gpol = _pop_policy(_pop_env(POP_M * POP_G).spec)
    with pytest.raises(ValueError, match='rescales actions'):
        GpuPopulationSampler(gpol, NormalizedVecEnv(_pop_env(POP_M * POP_G)),
                             n_members=POP_M, max_episode_length=POP_P,
                             seed=POP_SEED)


class _Trainer:
    """``step_epochs`` / ``step_itr`` / ``_train_args`` of ``garage.Trainer``."""

    def __init__(self, epochs, batch_size):
        self._epochs = epochs
        self._train_args = types.SimpleNamespace(batch_size=batch_size)
        self.step_itr = 0
        self.step_episode = None
        self.total_env_steps = 0

    def step_epochs(self):
        for epoch in range(self._epochs):
            yield epoch


def test_one_cem_epoch_on_statistics():
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.algos import CEM
    from garage_amd.envs import PendulumVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    members, g, length = 8, 16, 20
    torch.manual_seed(0)
    env = PendulumVecEnv(members * g, max_episode_length=length, seed=0)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, ))
    sampler = GpuPopulationSampler(pol, env, n_members=members,
                                   max_episode_length=length, seed=0,
                                   statistics_only=True)
    algo = CEM(env.spec, pol, sampler, members, best_frac=0.25, init_std=1,
               extra_std=0)
    returned, kinds, real = [], set(), algo._train_once

    def train_once(itr, episodes):
        rtn = real(itr, episodes)
        returned.append(rtn)
        kinds.add(isinstance(episodes, EpisodeStatistics))
        assert (np.asarray(episodes.lengths) == length).all()
        return rtn

    algo._train_once = train_once
    np.random.seed(0)
    trainer = _Trainer(1, g * length)
    algo.train(trainer)
    sampler.shutdown_worker()
    assert kinds == {True}
    assert trainer.step_itr == members and len(returned) == members
    returned = np.asarray(returned, dtype=np.float64)
    assert np.isfinite(returned).all() and (returned < 0).all()
    assert len(np.unique(returned)) > 1
    assert trainer.total_env_steps >= members * g * length
    assert np.isfinite(algo._cur_mean).all() and np.isfinite(algo._cur_std).all()


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
