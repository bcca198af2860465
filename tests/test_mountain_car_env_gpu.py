"""``MountainCarVecEnv`` on the GPU, both variants (``MountainCar-v0``'s three
classes behind a categorical policy, ``MountainCarContinuous-v0``'s force
behind a Gaussian one): the reset and step kernels against the numpy twin
(``garage_amd.envs.MountainCarEnv``) bit for bit, the one-launch rollout
against Python-driven steps for every step kernel, a replay on the twin and a
host batch of twins, ``NormalizedVecEnv`` (statistics inside the launch for the
classes, the force rescale on the per-step path), pickling, fragments, and a
population with its statistics.

A car from a reset draw (at rest in the valley) does not reach the goal within
a short ``max_episode_length`` under an untrained policy, so the rollouts that
must see TERMINAL inside a launch start some members through ``set_state`` just
below the goal line, moving right: those end on their first step whatever the
action, are reset inside the launch, and time out from then on."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE = 13, 14  # csrc/prof.h
TERMINAL, TIMEOUT = 2, 3
GUARD = 3
POISON = 12345.0
VARIANTS = pytest.mark.parametrize('continuous', [False, True],
                                   ids=['discrete', 'continuous'])


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(flags, device):
    return torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(device)


def _past_goal(count):
    """``count`` distinct states below the goal line, moving right fast enough
    that the next step passes it whatever the action, in either variant."""
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    st = np.stack([np.linspace(0.47, 0.499, count), np.full(count, 0.06)],
                  axis=-1).astype(f)
    for continuous, acts in ((False, (0, 1, 2)), (True, (-1.0, 0.0, 1.0))):
        for a in acts:
            act = np.full(count, a, dtype=f if continuous else int)
            assert MountainCarEnv.advance(st, act, continuous)[3].all()
    return st


def _edge_states(continuous):
    """Scripted starts and their first actions: on the left wall moving left
    and at rest, running into it, on the right wall at full speed, one step
    from each goal line, past the goal moving left, and actions past +-1 /
    out of range."""
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    lo, hi, vmax = (MountainCarEnv.MIN_X, MountainCarEnv.MAX_X,
                    MountainCarEnv.MAX_V)
    left, right, coast = ((-1.7, 1.7, 0.0) if continuous else (0, 2, 1))
    odd = 0.3 if continuous else 3
    rows = [((lo, -0.03), left), ((lo, 0), coast), ((lo, 0.02), right),
            ((-1.19, -vmax), left), ((-1.15, -0.05), odd),
            ((hi, vmax), right), ((0.58, vmax), right),
            ((0.499, 0.03), right), ((0.449, 0.03), right),
            ((0.499, 0.0005), left), ((0.55, -0.02), left),
            ((-0.5, 0), -1.0 if continuous else -1)]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


def _draws(seed, id0, n, counter=0):
    from garage_amd.envs import mountain_car_reset_draw
    return np.stack([mountain_car_reset_draw(seed, id0 + i, counter)
                     for i in range(n)])


class _Twins:
    """``n`` twins stepped together: the vectorised ``advance`` plus the
    episode bookkeeping of ``MountainCarEnv.step`` / ``reset``."""

    def __init__(self, seed, id0, n, P, states, continuous):
        self.seed, self.id0, self.P = seed, id0, P
        self.continuous = continuous
        self.state = states.copy()
        self.t = np.zeros(n, dtype=np.int64)
        self.resets = np.ones(n, dtype=np.int64)

    def step(self, actions):
        from garage_amd.envs import MountainCarEnv
        act = actions if self.continuous else actions.astype(int)
        self.state, obs, rew, done = MountainCarEnv.advance(
            self.state, act, self.continuous)
        self.t += 1
        types_ = np.where(self.t >= self.P, TIMEOUT,
                          np.where(done, TERMINAL,
                                   np.where(self.t == 1, 0, 1)))
        return obs, rew, types_

    def reset(self, which):
        from garage_amd.envs import mountain_car_reset_draw
        for i in np.nonzero(which)[0]:
            self.state[i] = mountain_car_reset_draw(self.seed, self.id0 + i,
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


@VARIANTS
@pytest.mark.parametrize('P', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 65])
def test_reset_and_step_kernels_equal_the_twin_bit_for_bit(n, P, continuous):
    """40 steps of ``ga_env_step`` with a masked ``ga_env_reset`` of the ended
    members after each, against the twin.  The batch is allocated with three
    more rows than the kernels are told of: those stay as poisoned."""
    from garage_amd.envs import MountainCarEnv, MountainCarVecEnv
    seed, id0, T = 9, 1000, 40
    f = np.float32
    env = MountainCarVecEnv(n + GUARD, continuous, max_episode_length=P,
                            seed=seed, env_id0=id0)
    assert env.obs_dim == 2 and env.act_width == 1
    assert env.env_info_specs == {}
    assert env._c.continuous == int(continuous)
    if continuous:
        assert env.spec.action_space.low.tolist() == [-1.0]
        assert env.spec.action_space.high.tolist() == [1.0]
    else:
        assert env.spec.action_space.n == 3
    env._c.n = n  # the kernels' batch; rows n .. n + 2 are guards
    _poison(env, n)
    env.reset_all()
    first = _draws(seed, id0, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(first))
    assert np.array_equal(_bits(_np(env.obs)[:n, :2]), _bits(first))
    assert (_np(env.obs)[:n, 2:] == 0).all()
    assert np.array_equal(_np(env._resets)[:n], np.ones(n))
    _guards_intact(env, n)

    rng = np.random.RandomState(3 + n)
    if continuous:  # forces outside [-1, 1] included
        actions = rng.uniform(-1.6, 1.6, (T, n)).astype(f)
    else:  # all three classes and the out-of-range indices 3 and -1
        actions = rng.randint(-1, 4, (T, n)).astype(f)
    states = first.copy()
    if n >= 15:  # the scripted starts, the rest from the reset draws
        edge, edge_act = _edge_states(continuous)
        assert len(edge) <= 15
        states[:len(edge)] = edge
        actions[0, :len(edge)] = edge_act
        with pytest.raises(ValueError, match='set_state'):
            env.set_state(np.zeros((n + GUARD, 3)))
        for j, v in ((0, MountainCarEnv.MAX_X), (1, MountainCarEnv.MAX_V),
                     (0, MountainCarEnv.MIN_X), (1, -MountainCarEnv.MAX_V)):
            with pytest.raises(ValueError, match='set_state needs x'):
                bad = np.zeros((n + GUARD, 2), dtype=f)
                bad[5, j] = np.nextafter(v, f(9) * np.sign(v))
                env.set_state(bad)
    env.set_state(np.concatenate([states, np.zeros((GUARD, 2), f)]))
    _poison(env, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(states))
    assert np.array_equal(_bits(_np(env.obs)[:n, :2]), _bits(states))
    twins = _Twins(seed, id0, n, P, states, continuous)
    act = torch.zeros(n + GUARD, 4, device=env.device)
    seen, stopped = set(), 0
    box = env.spec.observation_space
    for t in range(T):
        act[:n, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        want_obs, want_rew, want_type = twins.step(actions[t])
        assert np.array_equal(_bits(_np(env.next_obs)[:n, :2]),
                              _bits(want_obs)), t
        assert np.array_equal(_bits(_np(env.reward)[:n]), _bits(want_rew)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env.step_type)[:n], want_type), t
        assert (want_obs >= box.low).all() and (want_obs <= box.high).all()
        on_wall = want_obs[:, 0] == MountainCarEnv.MIN_X
        assert (want_obs[on_wall, 1] >= 0).all()
        stopped += int(on_wall.sum())
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
        want_obs[ended] = twins.state[ended]
        assert np.array_equal(_bits(_np(env.obs)[:n, :2]), _bits(want_obs)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env._resets)[:n], twins.resets), t
        assert np.array_equal(_np(env._t)[:n], twins.t), t
        _guards_intact(env, n)
    print('n', n, 'P', P, 'step types seen', sorted(seen), 'resets',
          int(twins.resets.sum()) - n, 'steps that ended on the wall', stopped)
    if n >= 15:
        assert stopped >= 2
    if n >= 15 and P >= 2:
        assert TERMINAL in seen  # the starts one step from the goal line
    if P <= 7:
        assert TIMEOUT in seen
    if P > 2:
        assert {0, 1} <= seen


@VARIANTS
def test_one_step_from_the_whole_state_box_equals_the_twin(continuous):
    """4099 states (no multiple of a block) drawn from the whole box, its
    faces included, with every kind of action: one ``ga_env_step`` against the
    twin, bit for bit."""
    from garage_amd.envs import MountainCarEnv, MountainCarVecEnv
    n, f = 4099, np.float32
    rng = np.random.RandomState(13)
    lo = np.asarray([MountainCarEnv.MIN_X, -MountainCarEnv.MAX_V], dtype=f)
    hi = np.asarray([MountainCarEnv.MAX_X, MountainCarEnv.MAX_V], dtype=f)
    st = np.stack([rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)],
                  axis=-1).astype(f)
    st[:100, 0], st[100:200, 0] = lo[0], hi[0]
    st[200:300, 1], st[300:400, 1] = lo[1], hi[1]
    st = np.clip(st, lo, hi)
    if continuous:
        actions = rng.uniform(-1.6, 1.6, n).astype(f)
    else:
        actions = rng.randint(-1, 4, n).astype(f)
    env = MountainCarVecEnv(n, continuous, max_episode_length=9, seed=1)
    env.reset_all()
    env.set_state(st)
    act = torch.zeros(n, 4, device=env.device)
    act[:, 0] = torch.from_numpy(actions)
    env.step_all(act)
    new, obs, rew, done = MountainCarEnv.advance(
        st, actions if continuous else actions.astype(int), continuous)
    assert np.array_equal(_bits(env.get_state()), _bits(new))
    assert np.array_equal(_bits(_np(env.next_obs)[:, :2]), _bits(obs))
    assert np.array_equal(_bits(_np(env.reward)), _bits(rew))
    assert np.array_equal(_np(env.step_type) == TERMINAL, done)
    assert done.any() and not done.all()
    assert ((new[:, 0] == lo[0]) & (new[:, 1] == 0)).any()


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


N, P = 64, 7
NUM = N * 24  # 24 steps in the one launch: three or more episodes per env
SCRIPTED = 20  # members 0 .. 19 start one step from the goal


def _scripted_starts(n, seed, id0, count=SCRIPTED):
    states = _draws(seed, id0, n)
    states[:count] = _past_goal(count)
    return states


def _make(continuous, hidden, options=None, n=N, native=True, wrap=None,
          env_seed=21, id0=3, worker=None, worker_args=None, scripted=False):
    from garage_amd.envs import MountainCarVecEnv
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(5)
    env = inner = MountainCarVecEnv(n, continuous, max_episode_length=P,
                                    seed=env_seed, env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    if continuous:
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.8,
                                **(options or {}))
    else:
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


def _ends(eps):
    types_ = np.asarray([int(s) for s in eps.step_types])
    ends = np.cumsum(eps.lengths) - 1
    return types_, ends


def _check_rewards(eps, continuous):
    """-1 every step; or +100 on the goal step, minus 0.1 a^2 of the policy's
    own (unclipped) action."""
    types_, ends = _ends(eps)
    if continuous:
        f = np.float32
        a = np.asarray(eps.actions, dtype=f)[:, 0]
        bonus = np.zeros(len(a), dtype=f)
        bonus[ends[types_[ends] == TERMINAL]] = 100
        assert np.array_equal(_bits(eps.rewards),
                              _bits(bonus - f(0.1) * (a * a)))
        assert np.abs(a).max() > 1  # the batch keeps the unclipped actions
    else:
        assert (eps.rewards == -1).all()
        assert set(np.unique(eps.actions)) == {0.0, 1.0, 2.0}


_whole_a = {}


def _one_launch_rollout(continuous, hidden, options, launches):
    """The native rollout of a fresh sampler (its batch on the host) after
    checking the whole-rollout launches of kinds (13, 14)."""
    from garage_amd import _lib
    lib = _lib.load()
    s, w = _make(continuous, hidden, options, scripted=True)
    assert w._fused_ok()
    kinds = (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)
    before = [int(lib.ga_launch_count(k)) for k in kinds]
    whole = w.rollout_samples(NUM).to_host()
    torch.cuda.synchronize()
    got = tuple(int(lib.ga_launch_count(k)) - b for k, b in zip(kinds, before))
    assert got == launches
    return whole


@VARIANTS
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
                                                       launches, continuous):
    whole = _one_launch_rollout(continuous, hidden, options, launches)
    if hidden == (64, 64) and options is None:
        _whole_a[continuous] = whole  # the replay test below reads it
    _, wb = _make(continuous, hidden, options, native=False, scripted=True)
    stepped = wb.rollout_samples(NUM).to_host()
    _same(whole, stepped)
    assert int(whole.lengths.sum()) >= NUM and whole.lengths.max() <= P
    # episodes end both ways inside the launch's 24 steps, resets follow
    types_, ends = _ends(whole)
    assert set(types_[ends].tolist()) == {TERMINAL, TIMEOUT}
    assert len(whole.lengths) >= 3 * N
    assert (np.delete(types_, ends) < 2).all()
    assert (whole.lengths[types_[ends] == TIMEOUT] == P).all()
    assert (types_[ends] == TERMINAL).sum() == SCRIPTED
    assert (whole.lengths[types_[ends] == TERMINAL] == 1).all()
    head = 'mean' if continuous else 'prob'
    assert np.isfinite(whole.agent_infos[head]).all()
    _check_rewards(whole, continuous)
    box = wb.env.spec.observation_space
    assert (whole.observations >= box.low).all()
    assert (whole.observations <= box.high).all()


@VARIANTS
def test_one_launch_rollout_replays_on_the_host_twin(continuous):
    """Case a's batch: every episode starts from its member's scripted start or
    from the reset draw of its member and reset counter, and the twin stepped
    with the recorded actions gives the recorded observations, rewards, step
    types and length, bit for bit."""
    from garage_amd.envs import MountainCarEnv
    whole = _whole_a.get(continuous)
    if whole is None:
        whole = _one_launch_rollout(continuous, (64, 64), None, (1, 0))
    seed, id0 = 21, 3
    first = _scripted_starts(N, seed, id0)
    starts, state_of = {}, {}
    for c in range(24):  # more resets than a member can have
        draws = first if c == 0 else _draws(seed, id0, N, c)
        for i in range(N):
            key = draws[i].tobytes()
            assert key not in starts
            starts[key] = (i, c)
            state_of[(i, c)] = draws[i]
    off = np.concatenate([[0], np.cumsum(whole.lengths)])
    order, counters = [], {}
    for e, L in enumerate(whole.lengths):
        obs = whole.observations[off[e]:off[e + 1]]
        act = whole.actions[off[e]:off[e + 1]]
        i, c = starts[np.ascontiguousarray(obs[0], np.float32).tobytes()]
        # a member's episodes come in the order of its resets
        assert counters.get(i, -1) + 1 == c
        counters[i] = c
        twin = MountainCarEnv(seed=seed, env_id=id0 + i, continuous=continuous,
                              max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
        if c == 0:
            twin.state = state_of[(i, 0)].copy()
            o = twin.state.copy()
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
    from garage_amd.envs import HostVecEnv, MountainCarEnv
    return HostVecEnv([MountainCarEnv(seed=env.seed, env_id=env.env_id0 + i,
                                      continuous=env.continuous,
                                      max_episode_length=P)
                       for i in range(env.n_envs)])


@VARIANTS
def test_device_batch_equals_a_host_batch_of_the_twins(continuous):
    """The same task behind ``HostVecEnv``: 64 ``MountainCarEnv`` objects with
    the batch's seed and member ids give the device batch's samples, bit for
    bit, over two calls (the second starts with a partial reset)."""
    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (_make(continuous, (64, 64), id0=0),
                        _make(continuous, (64, 64), id0=0, wrap=_host))
    for itr in range(2):
        a = sa.obtain_samples(itr, NUM, None).to_host()
        _same(a, sb.obtain_samples(itr, NUM, None).to_host())
        _check_rewards(a, continuous)


def test_normalized_mountain_car_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the
    discrete variant: no rescale, so each call's first steps stay one launch;
    native against Python-driven steps, two calls in a row."""
    from garage_amd import _lib
    from garage_amd.envs import NormalizedVecEnv
    lib = _lib.load()
    n = 70

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                                obs_alpha=0.05, reward_alpha=0.05)

    out, counts = [], []
    for native in (True, False):
        s, w = _make(False, (64, 64), n=n, native=native, wrap=wrap)
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
        assert len(np.unique(a.rewards)) > 5  # normalised: no longer all -1


def _rescaled(a):
    """``NormalizedVecEnv``'s rescale of the policy's action to the force box
    (``ga_action_rescale_f32``: fp32, one rounding per operation)."""
    f = np.float32
    a = np.asarray(a, dtype=f)
    slope = (f(0.5) * (f(1.0) - f(-1.0))) / f(1.0)
    v = f(-1.0) + (a + f(1.0)) * slope
    return np.clip(v, f(-1.0), f(1.0)).astype(f)


def test_normalized_continuous_car_rescales_the_force():
    """``NormalizedVecEnv(normalize_obs)`` around the continuous variant: the
    force bounds are finite, so the policy's actions are rescaled (and so
    clipped) to them in a launch of their own and the rollout takes per-step
    launches; native against Python-driven steps, two calls in a row.  The car
    is stepped with, and charged for, the rescaled force."""
    from garage_amd.envs import MountainCarEnv, NormalizedVecEnv
    n = 40

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, obs_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = _make(True, (64, 64), n=n, native=native, wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((n * 2 * P, n * 2 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        types_, ends = _ends(a)
        assert set(types_[ends].tolist()) == {TIMEOUT}
        f = np.float32
        acts = np.asarray(a.actions, dtype=f)[:, 0]
        assert np.abs(acts).max() > 1
        pushes = _rescaled(acts)
        assert np.array_equal(_bits(a.rewards),
                              _bits(f(0) - f(0.1) * (pushes * pushes)))
    k = 3
    for native in (True, False):
        s, w = _make(True, (64, 64), n=n, native=native, wrap=wrap)
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
        pushes = _rescaled(policy_actions)
        assert (np.abs(pushes) <= 1).all()
        state = _draws(21, 3, n)
        for t in range(k):
            state, _, _, done = MountainCarEnv.advance(state, pushes[:, t],
                                                       True)
            assert not done.any()
        assert np.array_equal(_bits(w.env._env.get_state()), _bits(state))


@VARIANTS
def test_pickled_sampler_continues_identically(continuous):
    sa, _ = _make(continuous, (64, 64), scripted=True)
    sa.obtain_samples(0, NUM, None)
    sb = pickle.loads(pickle.dumps(sa))
    ea, eb = sa._workers[0].env, sb._workers[0].env
    assert eb.continuous == continuous
    assert eb._c.continuous == int(continuous)
    assert eb.spec.action_space.flat_dim == ea.spec.action_space.flat_dim
    for k in ('_state', '_t', '_resets'):
        assert np.array_equal(_np(getattr(ea, k)), _np(getattr(eb, k))), k
    assert _np(ea._resets).min() >= 3
    for itr in (1, 2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


@VARIANTS
def test_fragment_worker_fragments_join_up(continuous):
    """``GpuFragmentWorker`` with 5 steps per call over 6 calls: the device
    batch's fragments equal a host batch of twins', and they join up -- a
    running fragment's last observation opens its member's next fragment, a
    closed one is followed by the member's next reset draw, and a twin per
    member replays every fragment with the recorded actions."""
    from garage_amd.envs import MountainCarEnv
    from garage_amd.sampler import GpuFragmentWorker
    n, tpc, seed = 17, 5, 21
    args = dict(n=n, id0=0, worker=GpuFragmentWorker,
                worker_args=dict(timesteps_per_call=tpc))
    (_, wa), (_, wb) = (_make(continuous, (64, 64), **args),
                        _make(continuous, (64, 64), wrap=_host, **args))
    twins = [MountainCarEnv(seed=seed, env_id=i, continuous=continuous,
                            max_episode_length=P) for i in range(n)]
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
POP_AT_GOAL = 21  # the one env (member 1's sixth) that starts below the line
DISCOUNT = 0.99  # not exact in binary


def _pop_env(continuous, n, env_id0=0):
    from garage_amd.envs import MountainCarVecEnv
    return MountainCarVecEnv(n, continuous, max_episode_length=POP_P, seed=3,
                             env_id0=env_id0)


def _pop_starts(n, env_id0=0):
    """The first states of ``n`` envs from ``env_id0`` on: their reset draws,
    but for global env 21, one step from the goal."""
    states = _draws(3, env_id0, n)
    if env_id0 <= POP_AT_GOAL < env_id0 + n:
        states[POP_AT_GOAL - env_id0] = _past_goal(3)[1]
    return states


def _pop_policy(continuous, spec):
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    if continuous:
        return GaussianMLPPolicy(spec, hidden_sizes=(8, 8), learn_std=True)
    return CategoricalMLPPolicy(spec, hidden_sizes=(8, 8))


def _member_vectors(pol, M):
    """Visibly different parameters per member, the log-std included."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.2 * rng.randn(M, base.size).astype(np.float32)
    if pol.kind == 'gaussian':
        vectors[:, 0] = np.log(0.3) + 0.5 * np.arange(M)
    return vectors.astype(np.float32)


def _population(continuous, **kw):
    """A population sampler whose worker has started (reset) and whose envs
    then got the scripted start: the next call's start resets nothing."""
    from garage_amd.sampler import GpuPopulationSampler
    torch.manual_seed(1)
    env = _pop_env(continuous, POP_M * POP_G)
    pol = _pop_policy(continuous, env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=POP_M,
                               max_episode_length=POP_P, seed=POP_SEED, **kw)
    pop._worker._start()
    env.set_state(_pop_starts(POP_M * POP_G))
    return pop, pol, _member_vectors(pol, POP_M)


@VARIANTS
def test_population_members_equal_lone_workers_and_their_statistics(
        continuous):
    """4 members x 16 envs, 24 steps in the launch, exactly ONE env of the 64
    started below the goal line: each member's batch is the lone worker's of
    those envs, and ``obtain_statistics`` of an identically built sampler
    gives, per episode, the length, ``terminated`` (true for one episode of
    all), the undiscounted return ``log_performance`` computes
    (``episode_statistics``: bit-equal) and the discounted return of
    ``log_performance_host``'s fp64 recurrence (bit-equal; within one fp32 ulp
    of ``log_performance``'s fp32 scan)."""
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.envs import NormalizedVecEnv
    from garage_amd.functions import episode_statistics
    from garage_amd.sampler import GpuPopulationSampler, GpuVecWorker
    pop, pol, vectors = _population(continuous)
    batches = pop.obtain_samples(0, POP_NUM, pol.pack_members(vectors))
    assert len(batches) == POP_M
    for m in range(POP_M):
        got = batches[m].to_host()
        env = _pop_env(continuous, POP_G, env_id0=m * POP_G)
        lone = _pop_policy(continuous, env.spec)
        lone.set_flat_param_values(vectors[m])
        w = GpuVecWorker(seed=POP_SEED, max_episode_length=POP_P,
                         worker_number=0, n_envs=POP_G)
        w.update_agent(lone)
        w.update_env(env)
        w._start()
        env.set_state(_pop_starts(POP_G, env_id0=m * POP_G))
        _same(got, w.rollout_samples(POP_NUM).to_host())
        assert got.lengths.max() <= POP_P and got.lengths.sum() >= POP_NUM
        if continuous:
            assert np.all(got.agent_infos['log_std'] ==
                          np.float32(vectors[m, 0]))
    a, b = batches[0].to_host(), batches[1].to_host()
    assert not np.array_equal(a.actions[:50], b.actions[:50])

    twin, tpol, _ = _population(continuous)
    stats = twin.obtain_statistics(0, POP_NUM, tpol.pack_members(vectors),
                                   DISCOUNT)
    assert len(stats) == POP_M
    assert twin.total_env_steps == pop.total_env_steps > 0
    terminated, returns = [], []
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
        returns.append(st.undiscounted_returns)
        assert st.undiscounted_returns.tobytes() == und.tobytes(), m
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
    # exactly one env reached the goal, once: member 1's, on its first step
    counts = [int(t.sum()) for t in terminated]
    print('population: terminated episodes per member', counts)
    assert counts == [0, 1, 0, 0]
    hit = int(np.nonzero(terminated[1])[0][0])
    assert stats[1].lengths[hit] == 1
    best = max(float(r.max()) for r in returns)
    if continuous:  # +100 less the cost of one action: the one return above 0
        assert 90 < returns[1][hit] == best
        assert sum(int((r > 0).sum()) for r in returns) == 1
    else:  # -1 against -7 everywhere else
        assert returns[1][hit] == best == -1
        assert sum(int((r > -POP_P).sum()) for r in returns) == 1

    if continuous:
        # normalize() rescales a bounded force: the population launch has none
        gpol = _pop_policy(True, _pop_env(True, POP_M * POP_G).spec)
        with pytest.raises(ValueError, match='rescales actions'):
            GpuPopulationSampler(
                gpol, NormalizedVecEnv(_pop_env(True, POP_M * POP_G)),
                n_members=POP_M, max_episode_length=POP_P, seed=POP_SEED)
