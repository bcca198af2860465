"""``AcrobotVecEnv`` on the GPU: the reset and step kernels against the numpy
twin (``garage_amd.envs.AcrobotEnv``) bit for bit, the one-launch rollout
against Python-driven steps for every step kernel, a replay on the twin and a
host batch of twins, ``NormalizedVecEnv``'s statistics inside the launch,
pickling, fragments, a population of three-class categorical policies with its
statistics, CEM and PPO.

The first device task with three action classes and a multi-stage integrator.
An episode from a reset draw (an arm hanging almost at rest) does not swing up
within a short ``max_episode_length``, so the rollouts that must see TERMINAL
inside a launch start some members through ``set_state`` on an arm that points
almost straight up and moves: those end within a step or two, are reset inside
the launch, and time out from then on."""
import pickle
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE = 13, 14  # csrc/prof.h
TERMINAL, TIMEOUT = 2, 3
GUARD = 3
POISON = 12345.0


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(flags, device):
    return torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(device)


def _observe(states):
    from garage_amd.envs import AcrobotEnv
    return AcrobotEnv.observe(np.asarray(states, dtype=np.float32))


def _near_goal(count, classes=(0, 1, 2)):
    """``count`` distinct states (th1 from 2.2 up, the arm straight, moving up)
    whose next step ends the episode whatever the class."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    th1 = np.linspace(2.2, 3.0, 161).astype(f)
    st = np.stack([th1, np.zeros_like(th1), np.full_like(th1, 2.0),
                   np.zeros_like(th1)], axis=-1)
    ok = np.ones(len(st), dtype=bool)
    for k in classes:
        ok &= AcrobotEnv.advance(st, np.full(len(st), k))[3]
    st = st[ok]
    assert len(st) >= count
    return st[np.linspace(0, len(st) - 1, count).astype(int)]


def _edge_states():
    """Scripted starts and their first classes: both speed clips either way,
    angles at exactly +-PI, the folds of sincos, one step from the goal, the
    fixed point."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    pi, half = AcrobotEnv.PI, f(1.5707963267948966)
    v1, v2 = AcrobotEnv.MAX_VEL_1, AcrobotEnv.MAX_VEL_2
    rows = [((1.598, -1.980, -v1, -v2), 0),   # the largest stage angle
            ((-1.598, 1.980, v1, v2), 2),
            ((0.3, -0.2, v1, -v2), 2),
            ((0.3, -0.2, -v1, v2), 0),
            ((pi, -pi, 1, -1), 1),
            ((-pi, pi, -3, 3), 3),
            ((np.nextafter(pi, f(0)), 0.1, 3, 0), -1),
            ((half, -half, 0, 0), 2),
            ((0, 0, 0, 0), 1)]
    rows += [(tuple(s), k) for s, k in zip(_near_goal(3), (0, 1, 2))]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


class _Twins:
    """``n`` twins stepped together: the vectorised ``advance`` plus the
    episode bookkeeping of ``AcrobotEnv.step`` / ``reset``."""

    def __init__(self, seed, id0, n, P, states):
        self.seed, self.id0, self.P = seed, id0, P
        self.state = states.copy()
        self.t = np.zeros(n, dtype=np.int64)
        self.resets = np.ones(n, dtype=np.int64)

    def step(self, classes):
        from garage_amd.envs import AcrobotEnv
        self.state, obs, rew, done = AcrobotEnv.advance(self.state, classes)
        self.t += 1
        types_ = np.where(self.t >= self.P, TIMEOUT,
                          np.where(done, TERMINAL,
                                   np.where(self.t == 1, 0, 1)))
        return obs, rew, types_

    def reset(self, which):
        from garage_amd.envs import acrobot_reset_draw
        for i in np.nonzero(which)[0]:
            self.state[i] = acrobot_reset_draw(self.seed, self.id0 + i,
                                               self.resets[i])
            self.resets[i] += 1
            self.t[i] = 0


def _poison(env, n):
    for t in (env._state, env.obs, env.next_obs, env.reward):
        t[n:] = POISON
    env.step_type[n:] = 77
    env._t[n:] = 1234567
    env._resets[n:] = 7654321


def _guards_intact(env, n):
    for t in (env._state, env.obs, env.next_obs, env.reward):
        assert (_np(t[n:]) == np.float32(POISON)).all()
    assert (_np(env.step_type[n:]) == 77).all()
    assert (_np(env._t[n:]) == 1234567).all()
    assert (_np(env._resets[n:]) == 7654321).all()


@pytest.mark.parametrize('P', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 65])
def test_reset_and_step_kernels_equal_the_twin_bit_for_bit(n, P):
    """40 steps of ``ga_env_step`` with a masked ``ga_env_reset`` of the ended
    members after each, against the twin.  The batch is allocated with three
    more rows than the kernels are told of: those stay as poisoned."""
    from garage_amd.envs import AcrobotEnv, AcrobotVecEnv, acrobot_reset_draw
    seed, id0, T = 9, 1000, 40
    f = np.float32
    env = AcrobotVecEnv(n + GUARD, max_episode_length=P, seed=seed,
                        env_id0=id0)
    assert env.obs_dim == 6 and env.act_width == 1
    assert env.env_info_specs == {}
    assert env.spec.action_space.n == 3
    env._c.n = n  # the kernels' batch; rows n .. n + 2 are guards
    _poison(env, n)
    env.reset_all()
    first = np.stack([acrobot_reset_draw(seed, id0 + i, 0) for i in range(n)])
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(first))
    assert np.array_equal(_bits(_np(env.obs)[:n, :6]), _bits(_observe(first)))
    assert (_np(env.obs)[:n, 6:] == 0).all()
    assert np.array_equal(_np(env._resets)[:n], np.ones(n))
    _guards_intact(env, n)

    rng = np.random.RandomState(3 + n)
    # all three classes and the out-of-range indices 3 and -1
    actions = rng.randint(-1, 4, (T, n)).astype(f)
    states = first.copy()
    if n >= 15:  # the scripted starts, the rest from the reset draws
        edge, edge_act = _edge_states()
        assert len(edge) <= 15
        states[:len(edge)] = edge
        actions[0, :len(edge)] = edge_act
        actions[:, 8] = 1  # the fixed point stays down: TIMEOUT at step P
        with pytest.raises(ValueError, match='set_state'):
            env.set_state(np.zeros((n + GUARD, 5)))
        with pytest.raises(ValueError, match=r'\[-PI, PI\]'):
            bad = np.zeros((n + GUARD, 4), dtype=f)
            bad[5, 1] = np.nextafter(AcrobotEnv.PI, f(9))
            env.set_state(bad)
        with pytest.raises(ValueError, match='speeds'):
            bad = np.zeros((n + GUARD, 4), dtype=f)
            bad[5, 3] = np.nextafter(AcrobotEnv.MAX_VEL_2, f(99))
            env.set_state(bad)
    env.set_state(np.concatenate([states, np.zeros((GUARD, 4), f)]))
    _poison(env, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(states))
    assert np.array_equal(_bits(_np(env.obs)[:n, :6]), _bits(_observe(states)))
    twins = _Twins(seed, id0, n, P, states)
    act = torch.zeros(n + GUARD, 4, device=env.device)
    seen = set()
    box = env.spec.observation_space
    for t in range(T):
        act[:n, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        want_obs, want_rew, want_type = twins.step(actions[t].astype(int))
        assert np.array_equal(_bits(_np(env.next_obs)[:n, :6]),
                              _bits(want_obs)), t
        assert np.array_equal(_bits(_np(env.reward)[:n]), _bits(want_rew)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env.step_type)[:n], want_type), t
        assert (np.abs(twins.state[:, :2]) <= AcrobotEnv.PI).all()
        assert (want_obs >= box.low).all() and (want_obs <= box.high).all()
        if P == 1:
            assert (want_type == TIMEOUT).all()
        seen |= set(want_type.tolist())
        # the ended members are reset, the others keep state and observation
        ended = want_type >= 2
        env.advance()
        env.hold()
        flags = np.ones(n + GUARD, dtype=bool)  # (guard flags set: not read)
        flags[:n] = ended
        env.reset_where(_mask(flags, env.device))
        env.advance()
        twins.reset(ended)
        want_obs[ended] = _observe(twins.state[ended])
        assert np.array_equal(_bits(_np(env.obs)[:n, :6]), _bits(want_obs)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env._resets)[:n], twins.resets), t
        assert np.array_equal(_np(env._t)[:n], twins.t), t
        _guards_intact(env, n)
    print('n', n, 'P', P, 'step types seen', sorted(seen), 'resets',
          int(twins.resets.sum()) - n)
    if n >= 15 and P >= 2:
        assert TERMINAL in seen  # the starts one step from the goal
    if P <= 7:
        assert TIMEOUT in seen
    if P > 2:
        assert {0, 1} <= seen


def test_one_step_from_the_whole_state_box_equals_the_twin():
    """4099 states (no multiple of a block) drawn from the whole box -- a
    quarter on the faces of the speed box, where the RK4 stages overshoot by
    tens of radians -- with all classes: one ``ga_env_step`` against the twin,
    bit for bit."""
    from garage_amd.envs import AcrobotEnv, AcrobotVecEnv
    n, f = 4099, np.float32
    rng = np.random.RandomState(12)
    hi = np.asarray([AcrobotEnv.PI, AcrobotEnv.PI, AcrobotEnv.MAX_VEL_1,
                     AcrobotEnv.MAX_VEL_2], dtype=f)
    st = (rng.uniform(-1, 1, (n, 4)) * hi).astype(f)
    st[:n // 8, 2] = np.where(st[:n // 8, 2] < 0, -1, 1) * hi[2]
    st[:n // 4, 3] = np.where(st[:n // 4, 3] < 0, -1, 1) * hi[3]
    st = np.clip(st, -hi, hi)
    classes = rng.randint(-1, 4, n)
    env = AcrobotVecEnv(n, max_episode_length=9, seed=1)
    env.reset_all()
    env.set_state(st)
    act = torch.zeros(n, 4, device=env.device)
    act[:, 0] = torch.from_numpy(classes.astype(f))
    env.step_all(act)
    new, obs, rew, done = AcrobotEnv.advance(st, classes)
    assert np.array_equal(_bits(env.get_state()), _bits(new))
    assert np.array_equal(_bits(_np(env.next_obs)[:, :6]), _bits(obs))
    assert np.array_equal(_bits(_np(env.reward)), _bits(rew))
    assert np.array_equal(_np(env.step_type) == TERMINAL, done)
    assert done.any() and not done.all()
    assert (np.abs(new[:, 2]) == hi[2]).any()
    assert (np.abs(new[:, 3]) == hi[3]).any()


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


N, P = 64, 7
NUM = N * 24  # 24 steps in the one launch: three or more episodes per env
SCRIPTED = 20  # members 0 .. 19 start one step from the goal


def _scripted_starts(n, seed, id0, count=SCRIPTED):
    from garage_amd.envs import acrobot_reset_draw
    states = np.stack([acrobot_reset_draw(seed, id0 + i, 0) for i in range(n)])
    states[:count] = _near_goal(count)
    return states


def _make(hidden, options=None, n=N, native=True, wrap=None, env_seed=21,
          id0=3, worker=None, worker_args=None, scripted=False):
    from garage_amd.envs import AcrobotVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(5)
    env = inner = AcrobotVecEnv(n, max_episode_length=P, seed=env_seed,
                                env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hidden,
                               **(options or {}))
    with torch.no_grad():  # gamma / beta (the buffer's tail) away from (1, 0)
        if pol.net.ln_off:
            lo = pol.net.ln_off[0]
            pol.net.params[lo:].add_(
                torch.randn_like(pol.net.params[lo:]) * 0.05)
    base = worker or GpuVecWorker
    cls = base if native else type('PythonSteps', (_PythonSteps, base), {})
    s = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                      worker_class=cls, seed=2,
                      worker_args=dict(n_envs=n, **(worker_args or {})))
    w = s._workers[0]
    if scripted:  # after the worker's own reset, which the next call skips
        w._start()
        inner.set_state(_scripted_starts(n, env_seed, id0))
    return s, w


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
    s, w = _make(hidden, options, scripted=True)
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
    ((320, 320), None, (0, 1)),
    ((512, ), None, (0, 1)),
], ids=['a-tanh-resident', 'b-relu-ln-resident', 'c-four-layers-streamed',
        'd-320-320-streamed-wide', 'e-512-wide'])
def test_one_launch_rollout_equals_python_driven_steps(hidden, options,
                                                       launches):
    whole = _one_launch_rollout(hidden, options, launches)
    if hidden == (64, 64) and options is None:
        _whole_a['batch'] = whole  # the replay test below reads the same batch
    _, wb = _make(hidden, options, native=False, scripted=True)
    stepped = wb.rollout_samples(NUM).to_host()
    _same(whole, stepped)
    assert int(whole.lengths.sum()) >= NUM and whole.lengths.max() <= P
    # episodes end both ways inside the launch's 24 steps, resets follow
    assert _ending_types(whole) == {TERMINAL, TIMEOUT}
    assert len(whole.lengths) >= 3 * N
    types_ = np.asarray([int(s) for s in whole.step_types])
    ends = np.cumsum(whole.lengths) - 1
    assert (np.delete(types_, ends) < 2).all()
    assert (whole.lengths[types_[ends] == TIMEOUT] == P).all()
    assert (types_[ends] == TERMINAL).sum() >= SCRIPTED
    assert (whole.lengths[types_[ends] == TERMINAL] < P).all()
    assert np.isfinite(whole.agent_infos['prob']).all()
    assert whole.agent_infos['prob'].shape[-1] == 3
    # all three classes drive the env
    assert set(np.unique(whole.actions)) == {0.0, 1.0, 2.0}
    # -1 per step, 0 on the terminating step only
    want = np.full(len(types_), -1, dtype=np.float32)
    want[ends[types_[ends] == TERMINAL]] = 0
    assert np.array_equal(whole.rewards, want)
    box = wb.env.spec.observation_space
    assert (whole.observations >= box.low).all()
    assert (whole.observations <= box.high).all()


def test_one_launch_rollout_replays_on_the_host_twin():
    """Case a's batch: every episode starts from its member's scripted start or
    from the reset draw of its member and reset counter, and the twin stepped
    with the recorded actions gives the recorded observations, rewards, step
    types and length, bit for bit."""
    from garage_amd.envs import AcrobotEnv, acrobot_reset_draw
    whole = _whole_a.get('batch')
    if whole is None:
        whole = _one_launch_rollout((64, 64), None, (1, 0))
    seed, id0 = 21, 3
    first = _scripted_starts(N, seed, id0)
    starts, state_of = {}, {}
    for i in range(N):
        for c in range(24):  # more resets than a member can have
            draw = first[i] if c == 0 else acrobot_reset_draw(seed, id0 + i, c)
            key = _observe(draw).tobytes()
            assert key not in starts
            starts[key] = (i, c)
            state_of[(i, c)] = draw
    off = np.concatenate([[0], np.cumsum(whole.lengths)])
    order, counters = [], {}
    for e, L in enumerate(whole.lengths):
        obs = whole.observations[off[e]:off[e + 1]]
        act = whole.actions[off[e]:off[e + 1]]
        i, c = starts[np.ascontiguousarray(obs[0], np.float32).tobytes()]
        # a member's episodes come in the order of its resets
        assert counters.get(i, -1) + 1 == c
        counters[i] = c
        twin = AcrobotEnv(seed=seed, env_id=id0 + i, max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
        if c == 0:
            twin.state = state_of[(i, 0)].copy()
            o = _observe(twin.state)
        for t in range(L):
            assert np.array_equal(_bits(o), _bits(obs[t])), (e, t)
            es = twin.step(act[t])
            o = es.observation
            assert (_bits(es.reward) == _bits(whole.rewards[off[e] + t])).all()
            assert int(es.step_type) == int(whole.step_types[off[e] + t])
            assert (int(es.step_type) >= 2) == (t == L - 1)
        assert np.array_equal(_bits(o), _bits(whole.last_observations[e]))
        order.append(i)
    assert len(counters) == N and min(counters.values()) >= 2
    # the completion step of an episode is the sum of its member's lengths so
    # far; the batch is sorted by (completion step, member)
    done_at, keys = {}, []
    for e, L in enumerate(whole.lengths):
        i = order[e]
        done_at[i] = done_at.get(i, 0) + int(L)
        keys.append((done_at[i], i))
    assert keys == sorted(keys)


def _host(env):
    from garage_amd.envs import AcrobotEnv, HostVecEnv
    return HostVecEnv([AcrobotEnv(seed=env.seed, env_id=env.env_id0 + i,
                                  max_episode_length=P)
                       for i in range(env.n_envs)])


def test_device_batch_equals_a_host_batch_of_the_twins():
    """The same task behind ``HostVecEnv``: 64 ``AcrobotEnv`` objects with the
    batch's seed and member ids give the device batch's samples, bit for bit,
    over two calls (the second starts with a partial reset)."""
    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (_make((64, 64), id0=0),
                        _make((64, 64), id0=0, wrap=_host))
    for itr in range(2):
        a = sa.obtain_samples(itr, NUM, None).to_host()
        _same(a, sb.obtain_samples(itr, NUM, None).to_host())
        assert set(np.unique(a.actions)) == {0.0, 1.0, 2.0}


def test_normalized_acrobot_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    a discrete action space has no rescale, so each call's first steps stay one
    launch; native against Python-driven steps, two calls in a row."""
    from garage_amd import _lib
    from garage_amd.envs import NormalizedVecEnv
    lib = _lib.load()
    n = 70

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                                obs_alpha=0.05, reward_alpha=0.05)

    out, counts = [], []
    for native in (True, False):
        s, w = _make((64, 64), n=n, native=native, wrap=wrap)
        assert w.env._act_low is None and w._fused_ok()
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((n * 2 * P, n * 2 * P + 17))])
        torch.cuda.synchronize()
        counts.append(int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before)
    assert counts == [2, 0]  # one whole-rollout launch per native call
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert np.isfinite(a.rewards).all()
        assert _ending_types(a) == {TIMEOUT}
        # normalised: the rewards are no longer all -1
        assert len(np.unique(a.rewards)) > 5


def test_pickled_sampler_continues_identically():
    sa, _ = _make((64, 64), scripted=True)
    sa.obtain_samples(0, NUM, None)
    sb = pickle.loads(pickle.dumps(sa))
    ea, eb = sa._workers[0].env, sb._workers[0].env
    for k in ('_state', '_t', '_resets'):
        assert np.array_equal(_np(getattr(ea, k)), _np(getattr(eb, k))), k
    assert _np(ea._resets).min() >= 3
    for itr in (1, 2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


def test_fragment_worker_fragments_join_up():
    """``GpuFragmentWorker`` with 5 steps per call over 6 calls: the device
    batch's fragments equal a host batch of twins', and they join up -- a
    running fragment's last observation opens its member's next fragment, a
    closed one is followed by the member's next reset draw, and a twin per
    member replays every fragment with the recorded actions."""
    from garage_amd.envs import AcrobotEnv
    from garage_amd.sampler import GpuFragmentWorker
    n, tpc, seed = 17, 5, 21
    args = dict(n=n, id0=0, worker=GpuFragmentWorker,
                worker_args=dict(timesteps_per_call=tpc))
    (_, wa), (_, wb) = _make((64, 64), **args), _make((64, 64), wrap=_host,
                                                      **args)
    twins = [AcrobotEnv(seed=seed, env_id=i, max_episode_length=P)
             for i in range(n)]
    opens = {}  # the observation that opens a member's next fragment
    for i, twin in enumerate(twins):
        opens[twin.reset()[0].tobytes()] = i
    ep_t, endings = np.zeros(n, dtype=np.int64), set()
    for call_no in range(6):
        a, b = wa.rollout().to_host(), wb.rollout().to_host()
        _same(a, b)
        assert int(a.lengths.sum()) == n * tpc
        off = np.concatenate([[0], np.cumsum(a.lengths)])
        for e, L in enumerate(a.lengths):
            obs = a.observations[off[e]:off[e + 1]]
            first = np.ascontiguousarray(obs[0], np.float32).tobytes()
            i = opens.pop(first)
            twin, o = twins[i], obs[0]
            for t in range(L):
                assert np.array_equal(_bits(o), _bits(obs[t])), (call_no, e, t)
                es = twin.step(a.actions[off[e] + t])
                o = es.observation
                assert (_bits(es.reward) ==
                        _bits(a.rewards[off[e] + t])).all()
                assert int(es.step_type) == int(a.step_types[off[e] + t])
                ep_t[i] += 1
                closed = int(es.step_type) >= 2
                assert closed == (t == L - 1 and
                                  (int(es.step_type) == TERMINAL or
                                   ep_t[i] == P))
            assert np.array_equal(_bits(o), _bits(a.last_observations[e]))
            if closed:
                endings.add(int(es.step_type))
                ep_t[i] = 0
                o = twin.reset()[0]
            opens[np.ascontiguousarray(o, np.float32).tobytes()] = i
        assert sorted(opens.values()) == list(range(n))
    assert endings == {TIMEOUT}


# -- population -----------------------------------------------------------------
POP_SEED, POP_M, POP_G, POP_P, POP_NUM = 5, 4, 16, 7, 16 * 24
POP_SCRIPTED = 5  # of each member's 16 envs
DISCOUNT = 0.99  # not exact in binary


def _pop_env(n, env_id0=0):
    from garage_amd.envs import AcrobotVecEnv
    return AcrobotVecEnv(n, max_episode_length=POP_P, seed=3, env_id0=env_id0)


def _pop_starts(n, env_id0=0):
    """The first states of ``n`` envs from ``env_id0`` on: of each member's 16,
    five one step from the goal, the others their reset draws."""
    from garage_amd.envs import acrobot_reset_draw
    states = np.stack([acrobot_reset_draw(3, env_id0 + i, 0)
                       for i in range(n)])
    near = _near_goal(POP_SCRIPTED)
    for lo in range(0, n, POP_G):
        states[lo:lo + POP_SCRIPTED] = near
    return states


def _pop_policy(spec):
    from garage_amd.policies import CategoricalMLPPolicy
    return CategoricalMLPPolicy(spec, hidden_sizes=(8, 8))


def _member_vectors(pol, M):
    """Visibly different parameters per member."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.5 * rng.randn(M, base.size).astype(np.float32)
    return vectors.astype(np.float32)


def _population(**kw):
    """A population sampler whose worker has started (reset) and whose envs
    then got the scripted starts: the next call's start resets nothing."""
    from garage_amd.sampler import GpuPopulationSampler
    torch.manual_seed(1)
    env = _pop_env(POP_M * POP_G)
    pol = _pop_policy(env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=POP_M,
                               max_episode_length=POP_P, seed=POP_SEED, **kw)
    pop._worker._start()
    env.set_state(_pop_starts(POP_M * POP_G))
    return pop, pol, _member_vectors(pol, POP_M)


def test_population_members_equal_lone_workers_and_their_statistics():
    """4 members x 16 envs, 24 steps in the launch: each member's batch is the
    lone worker's of those envs, and ``obtain_statistics`` of an identically
    built sampler gives, per episode, the length, ``terminated`` (true for the
    few episodes that swing up, false for the many that time out), the
    undiscounted return ``log_performance`` computes (``episode_statistics``:
    bit-equal) and the discounted return of ``log_performance_host``'s fp64
    recurrence (bit-equal; within one fp32 ulp of ``log_performance``'s fp32
    scan) -- over rewards that are all -1 but the terminating 0."""
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.functions import episode_statistics
    from garage_amd.sampler import GpuVecWorker
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
        w._start()
        env.set_state(_pop_starts(POP_G, env_id0=m * POP_G))
        _same(got, w.rollout_samples(POP_NUM).to_host())
        assert got.lengths.max() <= POP_P and got.lengths.sum() >= POP_NUM
        assert set(np.unique(got.actions)) <= {0.0, 1.0, 2.0}
    a, b = batches[0].to_host(), batches[1].to_host()
    assert not np.array_equal(a.actions[:50], b.actions[:50])

    twin, tpol, _ = _population()
    stats = twin.obtain_statistics(0, POP_NUM, tpol.pack_members(vectors),
                                   DISCOUNT)
    assert len(stats) == POP_M
    assert twin.total_env_steps == pop.total_env_steps > 0
    terminated = []
    for m in range(POP_M):
        st, host = stats[m], batches[m].to_host()
        assert isinstance(st, EpisodeStatistics) and st.success is None
        lengths = np.asarray(host.lengths, dtype=np.int64)
        assert np.array_equal(st.lengths, lengths)
        und, scan, term, _ = episode_statistics(batches[m], DISCOUNT)
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        ends = starts + lengths - 1
        types_ = np.asarray([int(s) for s in host.step_types])
        assert np.array_equal(np.asarray(term, dtype=bool),
                              types_[ends] == TERMINAL)
        assert np.array_equal(st.terminated,
                              np.asarray(term).astype(np.float64)), m
        terminated.append(np.asarray(term, dtype=bool))
        assert st.undiscounted_returns.tobytes() == und.tobytes(), m
        # sparse reward: the return is the length, less the terminating step
        assert np.array_equal(st.undiscounted_returns,
                              -(lengths - np.asarray(term, dtype=np.int64)))
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
    terminated = np.concatenate(terminated)
    print('population: {} episodes, {} terminated'.format(
        len(terminated), int(terminated.sum())))
    # both occur: the scripted starts swing up, every other episode times out
    assert terminated.sum() >= POP_M * POP_SCRIPTED
    assert (~terminated).sum() >= POP_M * POP_G


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
    """CEM over a three-class categorical policy, scored on returns that tie
    (every episode that does not swing up returns -20)."""
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.algos import CEM
    from garage_amd.envs import AcrobotVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    members, g, length = 8, 16, 20
    torch.manual_seed(0)
    env = AcrobotVecEnv(members * g, max_episode_length=length, seed=0)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(8, ))
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
        lengths = np.asarray(episodes.lengths)
        assert (1 <= lengths).all() and (lengths <= length).all()
        und = np.asarray(episodes.undiscounted_returns)
        term = np.asarray(episodes.terminated)
        assert np.array_equal(und, -(lengths - term))
        return rtn

    algo._train_once = train_once
    np.random.seed(0)
    trainer = _Trainer(1, g * length)
    algo.train(trainer)
    sampler.shutdown_worker()
    assert kinds == {True}
    assert trainer.step_itr == members and len(returned) == members
    returned = np.asarray(returned, dtype=np.float64)
    assert np.isfinite(returned).all()
    assert (returned <= 0).all() and (returned >= -length).all()
    assert trainer.total_env_steps >= members * g * length
    assert np.isfinite(algo._cur_mean).all() and np.isfinite(algo._cur_std).all()


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
