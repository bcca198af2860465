"""The procedures the seeded state-vector env kinds share on the GPU, one body
each, taking a row of ``_state_env_kinds.KINDS``: the reset and step kernels
against the numpy twin bit for bit, one step from the whole state box, the
one-launch rollout against Python-driven steps for every step kernel, a replay
on the twin and a host batch of twins, pickling, fragments, a population with
its statistics, and CEM.  ``tests/test_<kind>_env_gpu.py`` calls the bodies that
hold for its kind, under the test names they have always had.

What differs between the kinds -- the classes, the shapes, the scripted states,
and the assertions that only one kind can make -- is in the row; no body asks
which kind it runs.  An episode from a reset draw of Acrobot or MountainCar
does not end within a short ``max_episode_length``, so the rollouts of those
rows start ``SCRIPTED`` members through ``set_state`` one step from the goal:
those end at once, are reset inside the launch, and time out from then on."""
import pickle

import numpy as np
import pytest
import torch

import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import (GUARD, TERMINAL, TIMEOUT, _bits, _mask, _np,
                                _same)

def reset_and_step_kernels_equal_the_twin_bit_for_bit(row, n, P):
    """``kernel_steps`` steps of ``ga_env_step`` with a masked ``ga_env_reset``
    of the ended members after each, against the twin.  The batch is allocated
    with three more rows than the kernels are told of: those stay as
    poisoned."""
    seed, id0, T = 9, 1000, row.kernel_steps
    f, O, S = np.float32, row.obs_dim, row.state_dim
    env = row.new_batch(n + GUARD, max_episode_length=P, seed=seed,
                        env_id0=id0)
    assert env.obs_dim == O and env.act_width == 1
    assert env.env_info_specs == {}
    row.check_spec(env)
    env._c.n = n  # the kernels' batch; rows n .. n + 2 are guards
    h._poison(env, n)
    env.reset_all()
    first = h.draws(row, seed, id0, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(first))
    assert np.array_equal(_bits(_np(env.obs)[:n, :O]),
                          _bits(row.observe(first)))
    assert (_np(env.obs)[:n, O:] == 0).all()
    assert np.array_equal(_np(env._resets)[:n], np.ones(n))
    h._guards_intact(env, n)

    rng = np.random.RandomState(3 + n)
    actions = row.kernel_actions(rng, (T, n)).astype(f)
    states = first.copy()
    if n >= 15:  # the scripted starts, the rest from the reset draws
        edge, edge_act = row.edge_states()
        assert len(edge) <= 15
        states[:len(edge)] = edge
        actions[0, :len(edge)] = edge_act
        for member, action in row.hold:  # a member kept where it starts
            actions[:, member] = action
        for match, bad in row.bad_states(n + GUARD):
            with pytest.raises(ValueError, match=match):
                env.set_state(bad)
    env.set_state(np.concatenate([states, np.zeros((GUARD, S), f)]))
    h._poison(env, n)
    assert np.array_equal(_bits(env.get_state()[:n]), _bits(states))
    assert np.array_equal(_bits(_np(env.obs)[:n, :O]),
                          _bits(row.observe(states)))
    twins = row.kernel_twins(row, seed, id0, n, P, states)
    act = torch.zeros(n + GUARD, 4, device=env.device)
    seen, tally = set(), []
    box = env.spec.observation_space
    for t in range(T):
        act[:n, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        want_obs, want_rew, want_type = twins.step(actions[t])
        assert np.array_equal(_bits(_np(env.next_obs)[:n, :O]),
                              _bits(want_obs)), t
        assert np.array_equal(_bits(_np(env.reward)[:n]), _bits(want_rew)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env.step_type)[:n], want_type), t
        row.check_step(twins.state, want_obs, want_rew, box, tally)
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
        want_obs[ended] = twins.reset(ended)
        assert np.array_equal(_bits(_np(env.obs)[:n, :O]), _bits(want_obs)), t
        assert np.array_equal(_bits(env.get_state()[:n]),
                              _bits(twins.state)), t
        assert np.array_equal(_np(env._resets)[:n], twins.resets), t
        assert np.array_equal(_np(env._t)[:n], twins.t), t
        h._guards_intact(env, n)
    print('n', n, 'P', P, 'step types seen', sorted(seen), 'resets',
          int(twins.resets.sum()) - n)
    row.check_kernel_tally(n, tally)
    if n >= 15 and P >= 2:
        assert TERMINAL in seen  # the starts one step from an episode end
    if row.timeout_seen(n, P):
        assert TIMEOUT in seen
    if P > 2:
        assert {0, 1} <= seen


def one_step_from_the_whole_state_box_equals_the_twin(row):
    """4099 states (no multiple of a block) drawn from the whole box, its
    faces included, with every kind of action: one ``ga_env_step`` against the
    twin, bit for bit."""
    n, f, O = 4099, np.float32, row.obs_dim
    st, actions, reached = row.box_sample(n)
    env = row.new_batch(n, max_episode_length=9, seed=1)
    env.reset_all()
    env.set_state(st)
    act = torch.zeros(n, 4, device=env.device)
    act[:, 0] = torch.from_numpy(actions)
    env.step_all(act)
    new, obs, rew, done = row.advance(st, actions)
    assert np.array_equal(_bits(env.get_state()), _bits(new))
    assert np.array_equal(_bits(_np(env.next_obs)[:, :O]), _bits(obs))
    assert np.array_equal(_bits(_np(env.reward)), _bits(rew))
    assert np.array_equal(_np(env.step_type) == TERMINAL, done)
    assert done.any() and not done.all()
    reached(new)


_whole_a = {}  # row name -> the batch of network case a


def one_launch_rollout_equals_python_driven_steps(row, case):
    _, hidden, options, launches = case
    options = kinds.options_of(options)
    whole = h.one_launch_rollout(row, hidden, options, launches)
    if case is row.rollout_cases[0]:
        _whole_a[row.name] = whole  # the replay test below reads the same batch
    _, wb = h.make(row, hidden, options, native=False,
                   scripted=bool(row.SCRIPTED))
    stepped = wb.rollout_samples(row.NUM).to_host()
    _same(whole, stepped)
    row.check_rollout(row, whole, wb.env)


def one_launch_rollout_replays_on_the_host_twin(row):
    """Case a's batch: every episode starts from its member's scripted start or
    from the reset draw of its member and reset counter, and the twin stepped
    with the recorded actions gives the recorded observations, rewards, step
    types and length, bit for bit."""
    whole = _whole_a.get(row.name)
    if whole is None:
        _, hidden, options, launches = row.rollout_cases[0]
        whole = h.one_launch_rollout(row, hidden, options, launches)
    N, P, seed, id0 = row.N, row.P, 21, 3
    starts, state_of = {}, {}
    for c in range(row.replay_resets):  # more resets than a member can have
        draws = h.draws(row, seed, id0, N, c)
        if c == 0 and row.SCRIPTED:
            draws = h.scripted_starts(row, N, seed, id0)
        for i in range(N):
            key = row.observe(draws[i]).tobytes()
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
        twin = row.new_twin(seed=seed, env_id=id0 + i, max_episode_length=P)
        twin.resets = c
        o, _ = twin.reset()
        if c == 0:  # (a scripted start, or the same draw again)
            twin.state = state_of[(i, 0)].copy()
            o = row.observe(twin.state)
        for t in range(L):
            assert np.array_equal(_bits(o), _bits(obs[t])), (e, t)
            es = twin.step(row.replay_action(act[t]))
            o = es.observation
            assert (_bits(es.reward) == _bits(whole.rewards[off[e] + t])).all()
            assert int(es.step_type) == int(whole.step_types[off[e] + t])
            assert (int(es.step_type) >= 2) == (t == L - 1)
        assert np.array_equal(_bits(o), _bits(whole.last_observations[e]))
        order.append(i)
    row.check_replay(row, whole, counters, order)
    # the completion step of an episode is the sum of its member's lengths so
    # far; the batch is sorted by (completion step, member)
    done_at, keys = {}, []
    for e, L in enumerate(whole.lengths):
        i = order[e]
        done_at[i] = done_at.get(i, 0) + int(L)
        keys.append((done_at[i], i))
    assert keys == sorted(keys)


def device_batch_equals_a_host_batch_of_the_twins(row):
    """The same task behind ``HostVecEnv``: ``N`` twin objects with the
    batch's seed and member ids give the device batch's samples, bit for bit,
    over two calls (the second starts with a partial reset)."""
    # (id0 = 0: the action noise of member i is keyed by env_id0 + i, and a
    # HostVecEnv has no env_id0)
    (sa, _), (sb, _) = (h.make(row, (64, 64), id0=0),
                        h.make(row, (64, 64), id0=0, wrap=h.host_batch(row)))
    for itr in range(2):
        a = sa.obtain_samples(itr, row.NUM, None).to_host()
        _same(a, sb.obtain_samples(itr, row.NUM, None).to_host())
        row.check_host_call(a)


def pickled_sampler_continues_identically(row):
    sa, _ = h.make(row, (64, 64), scripted=bool(row.SCRIPTED))
    sa.obtain_samples(0, row.NUM, None)
    sb = pickle.loads(pickle.dumps(sa))
    ea, eb = sa._workers[0].env, sb._workers[0].env
    row.check_pickled(ea, eb)
    for k in ('_state', '_t', '_resets'):
        assert np.array_equal(_np(getattr(ea, k)), _np(getattr(eb, k))), k
    assert _np(ea._resets).min() >= row.pickle_min_resets
    for itr in (1, 2):
        _same(sa.obtain_samples(itr, row.NUM, None).to_host(),
              sb.obtain_samples(itr, row.NUM, None).to_host())


def fragment_worker_fragments_join_up(row):
    """``GpuFragmentWorker`` with 5 steps per call over 6 calls: the device
    batch's fragments equal a host batch of twins', and they join up -- a
    running fragment's last observation opens its member's next fragment, a
    closed one is followed by the member's next reset draw, and a twin per
    member replays every fragment with the recorded actions."""
    from garage_amd.sampler import GpuFragmentWorker
    n, tpc, seed, P = 17, 5, 21, row.P
    args = dict(n=n, id0=0, worker=GpuFragmentWorker,
                worker_args=dict(timesteps_per_call=tpc))
    (_, wa), (_, wb) = (h.make(row, (64, 64), **args),
                        h.make(row, (64, 64), wrap=h.host_batch(row), **args))
    twins = [row.new_twin(seed=seed, env_id=i, max_episode_length=P)
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
    assert endings == row.fragment_endings


def _population(row, **kw):
    """A population sampler; where the row scripts starts, its worker has
    started (reset) and its envs then got them: the next call's start resets
    nothing."""
    from garage_amd.sampler import GpuPopulationSampler
    n = row.POP_M * row.POP_G
    torch.manual_seed(1)
    env = kinds.pop_env(row, n)
    pol = kinds.pop_policy(row, env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=row.POP_M,
                               max_episode_length=row.POP_P,
                               seed=row.POP_SEED, **kw)
    if row.pop_starts is not None:
        pop._worker._start()
        env.set_state(row.pop_starts(row, n))
    return pop, pol, h._member_vectors(pol, row.POP_M, row.pop_scale,
                                       row.pop_log_std)


def population_members_equal_lone_workers_and_their_statistics(row):
    """``POP_M`` members x 16 envs: each member's batch is the lone worker's of
    those envs, and ``obtain_statistics`` of an identically built sampler
    gives, per episode, the length, ``terminated``, the undiscounted return
    ``log_performance`` computes (``episode_statistics``: bit-equal) and the
    discounted return of ``log_performance_host``'s fp64 recurrence (bit-equal;
    within one fp32 ulp of ``log_performance``'s fp32 scan).  Which episodes
    terminate and what the returns equal is the row's."""
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.functions import episode_statistics
    from garage_amd.sampler import GpuVecWorker
    M, G, POP_P, NUM = row.POP_M, row.POP_G, row.POP_P, row.POP_NUM
    pop, pol, vectors = _population(row)
    batches = pop.obtain_samples(0, NUM, pol.pack_members(vectors))
    assert len(batches) == M
    for m in range(M):
        got = batches[m].to_host()
        env = kinds.pop_env(row, G, env_id0=m * G)
        lone = kinds.pop_policy(row, env.spec)
        lone.set_flat_param_values(vectors[m])
        w = GpuVecWorker(seed=row.POP_SEED, max_episode_length=POP_P,
                         worker_number=0, n_envs=G)
        w.update_agent(lone)
        w.update_env(env)
        if row.pop_starts is not None:
            w._start()
            env.set_state(row.pop_starts(row, G, env_id0=m * G))
        _same(got, w.rollout_samples(NUM).to_host())
        assert got.lengths.max() <= POP_P and got.lengths.sum() >= NUM
        row.check_pop_member(row, got, vectors[m])
    a, b = batches[0].to_host(), batches[1].to_host()
    head = slice(row.pop_actions_head)
    assert not np.array_equal(a.actions[head], b.actions[head])

    twin, tpol, _ = _population(row)
    stats = twin.obtain_statistics(0, NUM, tpol.pack_members(vectors),
                                   row.DISCOUNT)
    assert len(stats) == M
    assert twin.total_env_steps == pop.total_env_steps > 0
    terminated, returns = [], []
    for m in range(M):
        st, host = stats[m], batches[m].to_host()
        assert isinstance(st, EpisodeStatistics) and st.success is None
        lengths = np.asarray(host.lengths, dtype=np.int64)
        assert np.array_equal(st.lengths, lengths)
        und, scan, term, _ = episode_statistics(batches[m], row.DISCOUNT)
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
                ret = float(x) + row.DISCOUNT * ret
            want.append(ret)
        want = np.asarray(want, dtype=np.float64)
        assert st.discounted_returns.tobytes() == want.tobytes(), m
        got32 = st.discounted_returns.astype(np.float32).astype(np.float64)
        ulp = np.spacing(np.abs(scan).astype(np.float32)).astype(np.float64)
        assert (np.abs(got32 - scan) <= ulp).all(), m
        row.check_pop_stats(st, host, lengths, term)
    row.check_pop_final(row, stats, terminated, returns)


def one_cem_epoch_on_statistics(row):
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.algos import CEM
    from garage_amd.sampler import GpuPopulationSampler
    members, g, length = 8, 16, 20
    torch.manual_seed(0)
    env = row.new_batch(members * g, max_episode_length=length, seed=0)
    pol = row.policy(env.spec, hidden_sizes=(8, ))
    sampler = GpuPopulationSampler(pol, env, n_members=members,
                                   max_episode_length=length, seed=0,
                                   statistics_only=True)
    algo = CEM(env.spec, pol, sampler, members, best_frac=0.25, init_std=1,
               extra_std=0)
    returned, seen, real, tally = [], set(), algo._train_once, []

    def train_once(itr, episodes):
        rtn = real(itr, episodes)
        returned.append(rtn)
        seen.add(isinstance(episodes, EpisodeStatistics))
        row.check_cem_episodes(episodes, length, tally)
        return rtn

    algo._train_once = train_once
    np.random.seed(0)
    trainer = h._Trainer(1, g * length)
    algo.train(trainer)
    sampler.shutdown_worker()
    assert seen == {True}
    assert trainer.step_itr == members and len(returned) == members
    returned = np.asarray(returned, dtype=np.float64)
    row.check_cem_final(returned, length, tally)
    assert trainer.total_env_steps >= members * g * length
    assert np.isfinite(algo._cur_mean).all() and np.isfinite(algo._cur_std).all()
