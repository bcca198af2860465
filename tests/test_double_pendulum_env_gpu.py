"""``DoublePendulumVecEnv`` on the GPU: the reset and step kernels against the
numpy twin (``garage_amd.envs.DoublePendulumEnv``) bit for bit, the one-launch
rollout against Python-driven steps for every step kernel, a replay on the twin
and a host batch of twins, ``NormalizedVecEnv``'s action rescale in front of
it, pickling, fragments, a population of Gaussian policies with its statistics,
CEM and PPO.

The first device task with a continuous action AND a termination that depends
on the dynamics: with ``max_episode_length`` 7 an episode ends TERMINAL (the tip
fell to ``y <= 1``) or TIMEOUT, both inside a launch of 24 steps, and each is
followed by a reset inside the launch."""
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
    from garage_amd.envs import DoublePendulumEnv
    return DoublePendulumEnv.observe(np.asarray(states, dtype=np.float32))


def _tip_threshold_states():
    """Three states ``(0, th, th + d, 0, 0, 0)`` whose step under zero action
    ends with ``y_tip`` exactly 1, one ulp below and one ulp above (found on
    the twin, among consecutive float32 angles around the crossing, for a few
    offsets ``d``: one family alone skips some values of the sum)."""
    from garage_amd.envs import DoublePendulumEnv
    f = np.float32

    def y_after(th, d):
        st = np.zeros((len(th), 6), dtype=f)
        st[:, 1], st[:, 2] = th, th + f(d)
        new, _, _, done = DoublePendulumEnv.advance(st, np.zeros(len(th), f))
        return DoublePendulumEnv._trig(new[:, 1], new[:, 2])[5], done, st

    wants = (f(1.0), np.nextafter(f(1.0), f(0)), np.nextafter(f(1.0), f(2)))
    found = {}
    for d in (0.0, 0.013, -0.027, 0.041):
        coarse = np.linspace(0.2, 0.7, 4001).astype(f)
        y, _, _ = y_after(coarse, d)
        k = int(np.nonzero(y <= 1)[0][0])
        lo = coarse[k - 1]
        span = int((coarse[k].view(np.uint32) - lo.view(np.uint32))) + 1
        th = (lo.view(np.uint32) + np.arange(span, dtype=np.uint32)).view(f)
        y, done, st = y_after(th, d)
        for want in wants:
            hit = np.nonzero(y == want)[0]
            if len(hit) and want.tobytes() not in found:
                assert bool(done[hit[0]]) == bool(want <= 1)
                found[want.tobytes()] = tuple(st[hit[0]])
    assert len(found) == 3, len(found)
    return [found[w.tobytes()] for w in wants]


def _edge_states():
    """Scripted starts and their first actions: the wraps of both angles either
    way, the +-100 speed guard, every +-10 clip of the observation, y_tip
    within one ulp of 1, the folds of sincos, the fixed point, a fallen one."""
    from garage_amd.envs import PendulumEnv
    f = np.float32
    pi, half = PendulumEnv.PI, PendulumEnv.HALF_PI
    rows = [((0, pi, -pi, 0, 5, -5), 0.5),
            ((0, -pi, pi, 0, -5, 5), -0.5),
            ((0, np.nextafter(pi, f(0)), 0.1, 0, 3, 0), 0.0),
            ((0, 0.3, -0.2, 99.99, 99.99, -99.99), 1.6),
            ((0, 0.3, -0.2, -99.99, -99.99, 99.99), -1.6),
            ((0.5, 0.1, 0.1, 11, -11, 4), 1.0),
            ((-0.5, -0.1, 0.1, -11, 11, -4), -1.0)]
    rows += [(s, 0.0) for s in _tip_threshold_states()]
    rows += [((0, half, -half, 0, 0, 0), 0.3),
             ((0, 0, 0, 0, 0, 0), 0.0),
             ((0, 1.5, 1.5, 0, 0, 0), 0.0)]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


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
    """12 steps of ``ga_env_step`` with a masked ``ga_env_reset`` of the ended
    members after each, against ``n`` twin objects.  The batch is allocated
    with three more rows than the kernels are told of: those stay as poisoned."""
    from garage_amd.envs import (DoublePendulumEnv, DoublePendulumVecEnv,
                                 PendulumEnv, double_pendulum_reset_draw)
    seed, id0, T = 9, 1000, 12
    f = np.float32
    env = DoublePendulumVecEnv(n + GUARD, max_episode_length=P, seed=seed,
                               env_id0=id0)
    assert env.obs_dim == 11 and env.act_width == 1
    assert env.env_info_specs == {}
    assert env.spec.action_space.low.tolist() == [-1.0]
    assert env.spec.action_space.high.tolist() == [1.0]
    env._c.n = n  # the kernels' batch; rows n .. n + 2 are guards
    _poison(env, n)
    env.reset_all()
    first = np.stack([double_pendulum_reset_draw(seed, id0 + i, 0)
                      for i in range(n)])
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(first))
    assert np.array_equal(_bits(_np(env.obs)[:n, :11]), _bits(_observe(first)))
    assert (_np(env.obs)[:n, 11] == 0).all()
    assert np.array_equal(_np(env._resets)[:n], np.ones(n))
    _guards_intact(env, n)

    rng = np.random.RandomState(3 + n)
    actions = rng.uniform(-1.6, 1.6, (T, n)).astype(f)
    states = first.copy()
    if n >= 15:  # the scripted starts, the rest from the reset draws
        edge, edge_act = _edge_states()
        assert len(edge) <= 15
        states[:len(edge)] = edge
        actions[0, :len(edge)] = edge_act
        actions[:, 11] = 0  # the fixed point stays up: TIMEOUT at step P
        with pytest.raises(ValueError, match='set_state'):
            env.set_state(np.zeros((n + GUARD, 5)))
        with pytest.raises(ValueError, match=r'\[-PI, PI\]'):
            bad = np.zeros((n + GUARD, 6), dtype=f)
            bad[5, 2] = np.nextafter(PendulumEnv.PI, f(9))
            env.set_state(bad)
    env.set_state(np.concatenate([states, np.zeros((GUARD, 6), f)]))
    _poison(env, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(states))
    assert np.array_equal(_bits(_np(env.obs)[:n, :11]), _bits(_observe(states)))
    twins = [DoublePendulumEnv(seed=seed, env_id=id0 + i, max_episode_length=P)
             for i in range(n)]
    for i, twin in enumerate(twins):
        twin.resets = 1
        twin.state = states[i].copy()
    act = torch.zeros(n + GUARD, 4, device=env.device)
    seen, resets = set(), np.ones(n, dtype=np.int64)
    for t in range(T):
        act[:n, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        steps = [twin.step(actions[t, i:i + 1]) for i, twin in enumerate(twins)]
        want_obs = np.stack([s.observation for s in steps])
        want_rew = np.asarray([s.reward for s in steps], dtype=f)
        want_state = np.stack([twin.state for twin in twins])
        want_type = np.asarray([int(s.step_type) for s in steps])
        assert np.array_equal(_bits(_np(env.next_obs)[:n, :11]),
                              _bits(want_obs)), t
        assert np.array_equal(_bits(_np(env.reward)[:n]), _bits(want_rew)), t
        assert np.array_equal(_bits(env.get_state()[:n]), _bits(want_state)), t
        assert np.array_equal(_np(env.step_type)[:n], want_type), t
        assert np.isfinite(want_state).all() and np.isfinite(want_rew).all()
        assert (np.abs(want_state[:, 1:3]) <= PendulumEnv.PI).all()
        assert (np.abs(want_state[:, 3:]) <= 100).all()
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
        for i in np.nonzero(ended)[0]:
            o, _ = twins[i].reset()
            want_obs[i] = o
        resets += ended
        assert np.array_equal(_bits(_np(env.obs)[:n, :11]), _bits(want_obs)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(np.stack([tw.state for tw in twins]))), t
        assert np.array_equal(_np(env._resets)[:n], resets), t
        assert np.array_equal(_np(env._t)[:n], [tw._t for tw in twins]), t
        _guards_intact(env, n)
    print('n', n, 'P', P, 'step types seen', sorted(seen), 'resets',
          int(resets.sum()) - n)
    if n >= 15 and P >= 2:
        assert TERMINAL in seen  # the fallen start, the y_tip <= 1 starts
    if P <= 2 or (P == 7 and n >= 15):
        assert TIMEOUT in seen
    if P > 2:
        assert {0, 1} <= seen


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


N, P = 33, 7
NUM = N * 24  # 24 steps in the one launch: three or more episodes per env


def _make(hidden, options=None, n=N, native=True, wrap=None, env_seed=21,
          id0=3, worker=None, worker_args=None):
    from garage_amd.envs import DoublePendulumVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(5)
    env = DoublePendulumVecEnv(n, max_episode_length=P, seed=env_seed,
                               env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.5,
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
    assert int(whole.lengths.sum()) >= NUM and whole.lengths.max() <= P
    # episodes end both ways, most of them inside the launch's 24 steps
    assert _ending_types(whole) == {TERMINAL, TIMEOUT}
    assert len(whole.lengths) >= 3 * N
    types_ = np.asarray([int(s) for s in whole.step_types])
    ends = np.cumsum(whole.lengths) - 1
    assert (np.delete(types_, ends) < 2).all()
    assert (whole.lengths[types_[ends] == TIMEOUT] == P).all()
    assert (whole.lengths[types_[ends] == TERMINAL] < P).all()
    assert np.isfinite(whole.agent_infos['mean']).all()
    assert np.isfinite(whole.observations).all()
    assert (whole.observations[:, 8:] == 0).all()
    # the batch keeps the policy's own actions, not the clipped pushes
    assert np.abs(whole.actions).max() > 1
    assert len(np.unique(whole.rewards)) > NUM // 2
    # the terminating step keeps its reward (alive bonus included)
    assert (whole.rewards[ends] > 0).all()


def test_one_launch_rollout_replays_on_the_host_twin():
    """Case a's batch: every episode starts from the reset draw of its member
    and reset counter, and the twin stepped with the recorded actions gives the
    recorded observations, rewards, step types and length, bit for bit."""
    from garage_amd.envs import DoublePendulumEnv, double_pendulum_reset_draw
    whole = _whole_a.get('batch')
    if whole is None:
        whole = _one_launch_rollout((64, 64), None, (1, 0))
    seed, id0 = 21, 3
    starts = {}
    for i in range(N):
        for c in range(24):  # more resets than a member can have
            draw = double_pendulum_reset_draw(seed, id0 + i, c)
            starts[_observe(draw).tobytes()] = (i, c)
    off = np.concatenate([[0], np.cumsum(whole.lengths)])
    order, counters = [], {}
    for e, L in enumerate(whole.lengths):
        obs = whole.observations[off[e]:off[e + 1]]
        act = whole.actions[off[e]:off[e + 1]]
        i, c = starts[np.ascontiguousarray(obs[0], np.float32).tobytes()]
        # a member's episodes come in the order of its resets
        assert counters.get(i, -1) + 1 == c
        counters[i] = c
        twin = DoublePendulumEnv(seed=seed, env_id=id0 + i,
                                 max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
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
    from garage_amd.envs import DoublePendulumEnv, HostVecEnv
    return HostVecEnv([DoublePendulumEnv(seed=env.seed, env_id=env.env_id0 + i,
                                         max_episode_length=P)
                       for i in range(env.n_envs)])


def test_device_batch_equals_a_host_batch_of_the_twins():
    """The same task behind ``HostVecEnv``: 33 ``DoublePendulumEnv`` objects
    with the batch's seed and member ids give the device batch's samples, bit
    for bit, over two calls (the second starts with a partial reset)."""
    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (_make((64, 64), id0=0),
                        _make((64, 64), id0=0, wrap=_host))
    for itr in range(2):
        _same(sa.obtain_samples(itr, NUM, None).to_host(),
              sb.obtain_samples(itr, NUM, None).to_host())


def _rescaled(a):
    """``NormalizedVecEnv``'s rescale of the policy's action to the push box
    (``ga_action_rescale_f32``: fp32, one rounding per operation)."""
    f = np.float32
    a = np.asarray(a, dtype=f)
    slope = (f(0.5) * (f(1.0) - f(-1.0))) / f(1.0)
    v = f(-1.0) + (a + f(1.0)) * slope
    return np.clip(v, f(-1.0), f(1.0)).astype(f)


def test_normalized_double_pendulum_rescales_the_push():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the batch:
    the push bounds are finite, so the policy's actions are rescaled to them in
    a launch of their own and the rollout takes per-step launches; native
    against Python-driven steps, two calls in a row."""
    from garage_amd.envs import (DoublePendulumEnv, NormalizedVecEnv,
                                 double_pendulum_reset_draw)
    n = 40

    def wrap(env):
        return NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                                obs_alpha=0.05, reward_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = _make((64, 64), n=n, native=native, wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((n * 2 * P, n * 2 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        assert np.isfinite(a.rewards).all()
        assert _ending_types(a) == {TERMINAL, TIMEOUT}
    # what the wrapped env was stepped with: two steps into an episode (none
    # ends that early) its state is the twin's after the rescaled (and so
    # clipped) recorded actions
    k = 2
    for native in (True, False):
        s, w = _make((64, 64), n=n, native=native, wrap=wrap)
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


def test_fragment_worker_fragments_join_up():
    """``GpuFragmentWorker`` with 5 steps per call over 6 calls: the device
    batch's fragments equal a host batch of twins', and they join up -- a
    running fragment's last observation opens its member's next fragment, a
    closed one is followed by the member's next reset draw, and a twin per
    member replays every fragment with the recorded actions."""
    from garage_amd.envs import DoublePendulumEnv
    from garage_amd.sampler import GpuFragmentWorker
    n, tpc, seed = 17, 5, 21
    args = dict(n=n, id0=0, worker=GpuFragmentWorker,
                worker_args=dict(timesteps_per_call=tpc))
    (_, wa), (_, wb) = _make((64, 64), **args), _make((64, 64), wrap=_host,
                                                      **args)
    twins = [DoublePendulumEnv(seed=seed, env_id=i, max_episode_length=P)
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
    assert endings == {TERMINAL, TIMEOUT}


# -- population -----------------------------------------------------------------
POP_SEED, POP_M, POP_G, POP_P, POP_NUM = 5, 4, 16, 7, 16 * 24
DISCOUNT = 0.99  # not exact in binary


def _pop_env(n, env_id0=0):
    from garage_amd.envs import DoublePendulumVecEnv
    return DoublePendulumVecEnv(n, max_episode_length=POP_P, seed=3,
                                env_id0=env_id0)


def _pop_policy(spec):
    from garage_amd.policies import GaussianMLPPolicy
    return GaussianMLPPolicy(spec, hidden_sizes=(8, 8), learn_std=True)


def _member_vectors(pol, M):
    """Visibly different parameters per member, the log-std included."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.2 * rng.randn(M, base.size).astype(np.float32)
    vectors[:, 0] = np.log(0.1) + 0.5 * np.arange(M)
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
    """4 members x 16 envs, 24 steps in the launch: each member's batch is the
    lone worker's of those envs, and ``obtain_statistics`` of an identically
    built sampler gives, per episode, the length, ``terminated`` (true for
    some episodes and false for others), the undiscounted return
    ``log_performance`` computes (``episode_statistics``: bit-equal) and the
    discounted return of ``log_performance_host``'s fp64 recurrence (bit-equal;
    within one fp32 ulp of ``log_performance``'s fp32 scan)."""
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
        assert got.lengths.max() <= POP_P and got.lengths.sum() >= POP_NUM
        assert np.all(got.agent_infos['log_std'] == np.float32(vectors[m, 0]))
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
    terminated = np.concatenate(terminated)
    print('population: {} episodes, {} terminated'.format(
        len(terminated), int(terminated.sum())))
    assert terminated.any() and not terminated.all()

    # normalize() rescales a bounded push: the population launch has no rescale
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
    from garage_amd.envs import DoublePendulumVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    members, g, length = 8, 16, 20
    torch.manual_seed(0)
    env = DoublePendulumVecEnv(members * g, max_episode_length=length, seed=0)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(8, ))
    sampler = GpuPopulationSampler(pol, env, n_members=members,
                                   max_episode_length=length, seed=0,
                                   statistics_only=True)
    algo = CEM(env.spec, pol, sampler, members, best_frac=0.25, init_std=1,
               extra_std=0)
    returned, kinds, real = [], set(), algo._train_once
    terminated = []

    def train_once(itr, episodes):
        rtn = real(itr, episodes)
        returned.append(rtn)
        kinds.add(isinstance(episodes, EpisodeStatistics))
        lengths = np.asarray(episodes.lengths)
        assert (1 <= lengths).all() and (lengths <= length).all()
        terminated.append(np.asarray(episodes.terminated))
        return rtn

    algo._train_once = train_once
    np.random.seed(0)
    trainer = _Trainer(1, g * length)
    algo.train(trainer)
    sampler.shutdown_worker()
    assert kinds == {True}
    assert trainer.step_itr == members and len(returned) == members
    returned = np.asarray(returned, dtype=np.float64)
    assert np.isfinite(returned).all() and (returned > 0).all()
    assert len(np.unique(returned)) > 1
    assert trainer.total_env_steps >= members * g * length
    assert np.isfinite(algo._cur_mean).all() and np.isfinite(algo._cur_std).all()
    assert np.concatenate(terminated).any()


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
