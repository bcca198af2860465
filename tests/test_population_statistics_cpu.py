"""Scoring a population without packing, as far as it goes without a GPU:
``CEM`` driven through ``obtain_statistics`` against the real reference class's
golden file, ``log_performance_statistics`` against ``log_performance_host`` on
the same episodes, and every refusal of ``ga_member_progress`` /
``ga_member_episode_statistics`` through ctypes with host pointers (each check
precedes the first launch)."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from garage_amd import _lib, logger
from garage_amd._dtypes import (Box, EnvSpec, EpisodeBatch, EpisodeStatistics,
                                StepType)
from garage_amd.algos import CEM
from garage_amd.functions import (log_performance_host,
                                  log_performance_statistics)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, 'tests', 'golden', 'cem.npz'))
(N_SAMPLES, BEST_FRAC, EXTRA_DECAY, EPOCHS, N_PARAMS, EPISODES, SEED, DISCOUNT,
 INIT_STD, EXTRA_STD) = GOLDEN['settings']
N_SAMPLES, EPOCHS, EPISODES, SEED = (int(N_SAMPLES), int(EPOCHS), int(EPISODES),
                                     int(SEED))
SPEC = EnvSpec(Box(-1, 1, (2, )), Box(-1, 1, (1, )), max_episode_length=1)


class KeyTabular(logger.Tabular):
    """The stand-in recorder that also keeps the ``record`` calls in order."""

    def __init__(self):
        super().__init__()
        self.keys, self.rows = [], []

    def record(self, key, val):
        super().record(key, val)
        self.keys.append(self._prefix + str(key))
        self.rows.append((self._prefix + str(key), val))


class FlatPolicy:

    def __init__(self, theta):
        self.theta = np.array(theta, dtype=np.float64)

    def get_flat_param_values(self):
        return self.theta.copy()

    def set_flat_param_values(self, theta):
        self.theta = np.array(theta, dtype=np.float64)


class StubStatisticsSampler:
    """``test_cem_cpu.py``'s stub reduced to statistics: per member ``EPISODES``
    one-step ``TERMINAL`` episodes rewarded by the member's own vector.  It has
    no ``obtain_samples``: calling it is an error."""

    n_members = N_SAMPLES
    statistics_only = True

    def __init__(self):
        self.calls = []

    def obtain_statistics(self, itr, num_samples, member_params, discount,
                          env_update=None):
        member_params = np.asarray(member_params)
        self.calls.append((itr, num_samples, member_params.copy(), discount))
        out = []
        for theta in member_params:
            d = theta.astype(np.float64) - GOLDEN['theta_star']
            reward = np.full(EPISODES, -np.sum(d * d), dtype=np.float64)
            # one step: its reward is the sum and the discounted return
            out.append(EpisodeStatistics(
                lengths=np.ones(EPISODES, dtype=np.int64),
                undiscounted_returns=reward, discounted_returns=reward,
                terminated=np.ones(EPISODES), success=None,
                discount=discount))
        return out


class StubTrainer:

    def __init__(self, epochs, batch_size=17):
        self._epochs = epochs
        self._train_args = types.SimpleNamespace(batch_size=batch_size)
        self.step_itr = 0
        self.step_episode = None
        self.total_env_steps = 0

    def step_epochs(self):
        for epoch in range(self._epochs):
            yield epoch


def test_cem_on_statistics_reproduces_the_reference_s_golden_file():
    policy = FlatPolicy(GOLDEN['theta_0'])
    sampler = StubStatisticsSampler()
    algo = CEM(SPEC, policy, sampler, N_SAMPLES, discount=DISCOUNT,
               init_std=INIT_STD, best_frac=BEST_FRAC, extra_std=EXTRA_STD,
               extra_decay_time=EXTRA_DECAY)
    rec, old = KeyTabular(), logger.tabular
    logger.tabular = rec
    trainer = StubTrainer(EPOCHS)
    returned, keys, means, stds, seen = [], [], [], [], []
    real = algo._train_once

    def train_once(itr, episodes):
        rec.keys = []
        rtn = real(itr, episodes)
        returned.append(rtn)
        keys.append('\n'.join(rec.keys))
        seen.append(trainer.step_episode)
        if (itr + 1) % N_SAMPLES == 0:
            means.append(np.array(algo._cur_mean))
            stds.append(np.array(algo._cur_std))
        return rtn

    algo._train_once = train_once
    np.random.seed(SEED)
    try:
        last = algo.train(trainer)
    finally:
        logger.tabular = old
    calls = sampler.calls
    assert [c[0] for c in calls] == [e * N_SAMPLES for e in range(EPOCHS)]
    assert all(c[1] == 17 and c[3] == DISCOUNT for c in calls)
    sampled = np.concatenate([c[2] for c in calls])
    assert sampled.dtype == np.float64
    assert np.array_equal(sampled, GOLDEN['evaluated'])
    assert np.array_equal(np.asarray(means), GOLDEN['cur_mean'])
    assert np.array_equal(np.asarray(stds), GOLDEN['cur_std'])
    got = np.asarray(returned, dtype=np.float64)
    assert np.array_equal(got, GOLDEN['returned'])
    assert np.float64(last) == GOLDEN['train_returned']
    assert np.array_equal(algo._cur_params, GOLDEN['next_candidate'])
    assert np.array_equal(policy.theta, GOLDEN['next_candidate'])
    assert keys == list(GOLDEN['keys'])
    assert trainer.step_itr == EPOCHS * N_SAMPLES
    assert trainer.total_env_steps == EPOCHS * N_SAMPLES * EPISODES
    # trainer.step_episode is the member's statistics
    assert all(isinstance(s, EpisodeStatistics) for s in seen)


# -- log_performance_statistics against log_performance_host ---------------------
LENGTHS = [3, 1, 4, 2]
REWARDS = np.asarray([0.1, -1.7, 2.3, 0.3, 1e-3, 5.5, -0.7, 0.9, 2.0, -3.1])
TYPES = [StepType.FIRST, StepType.MID, StepType.TERMINAL,
         StepType.TIMEOUT,
         StepType.FIRST, StepType.MID, StepType.MID, StepType.TIMEOUT,
         StepType.FIRST, StepType.TERMINAL]
SUCCESS = np.asarray([0, 0, 1, 0, 0, 0, 0, 0, 0, 0], dtype=bool)


def _recorded(fn, *args, **kw):
    rec, old = KeyTabular(), logger.tabular
    logger.tabular = rec
    try:
        out = fn(*args, **kw)
    finally:
        logger.tabular = old
    return rec.rows, out


@pytest.mark.parametrize('with_success', [False, True],
                         ids=['no-success', 'success'])
def test_rows_are_log_performance_host_s(with_success):
    discount, S = 0.99, sum(LENGTHS)
    batch = EpisodeBatch(
        env_spec=EnvSpec(Box(-1, 1, (2, )), Box(-1, 1, (1, )),
                         max_episode_length=4),
        episode_infos={}, observations=np.zeros((S, 2), np.float32),
        last_observations=np.zeros((len(LENGTHS), 2), np.float32),
        actions=np.zeros((S, 1), np.float32), rewards=REWARDS,
        env_infos=dict(success=SUCCESS) if with_success else {},
        agent_infos={}, step_types=np.asarray(TYPES, dtype=StepType),
        lengths=np.asarray(LENGTHS, dtype='l'))
    # the hand-written statistics of those episodes
    und, disc, term, succ, start = [], [], [], [], 0
    for L in LENGTHS:
        r = REWARDS[start:start + L]
        acc = 0.0
        for x in r:
            acc = acc + float(x)
        ret = 0.0
        for x in r[::-1]:
            ret = float(x) + discount * ret
        und.append(acc)
        disc.append(ret)
        term.append(float(StepType.TERMINAL in TYPES[start:start + L]))
        succ.append(float(SUCCESS[start:start + L].any()))
        start += L
    assert term == [1.0, 0.0, 0.0, 1.0] and succ == [1.0, 0.0, 0.0, 0.0]
    stats = EpisodeStatistics(LENGTHS, und, disc, term,
                              succ if with_success else None, discount)
    want, want_ret = _recorded(log_performance_host, 7, batch, discount,
                               prefix='Pop')
    got, got_ret = _recorded(log_performance_statistics, 7, stats,
                             prefix='Pop')
    assert [k for k, _ in got] == [k for k, _ in want]
    assert ('Pop/SuccessRate' in dict(got)) == with_success
    for (k, a), (_, b) in zip(got, want):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), k
    assert isinstance(got_ret, list)
    assert [np.float64(x).tobytes() for x in got_ret] == [
        np.float64(x).tobytes() for x in want_ret]
    assert stats.lengths.dtype == np.int64
    assert stats.terminated.dtype == np.float64
    with pytest.raises(ValueError, match='discounted_returns has shape'):
        EpisodeStatistics(LENGTHS, und, disc[:-1], term)


# -- the C ABI's refusals ------------------------------------------------------
N, TCAP, COLS, MEMBERS, SAMPLES = 64, 8, 6, 2, 10


def _progress(tail='buf', progress='buf', col_base='buf', n=N, tcap=TCAP,
              cols=COLS, members=MEMBERS, samples=SAMPLES):
    buf = (C.c_double * 16)()
    a = {k: (C.addressof(buf) if v == 'buf' else v)
         for k, v in dict(tail=tail, progress=progress,
                          col_base=col_base).items()}
    _lib.call('ga_member_progress', a['tail'], n, tcap, cols, members, samples,
              a['progress'], a['col_base'], None)


def _statistics(n=N, tcap=TCAP, cols=COLS, members=MEMBERS, samples=SAMPLES,
                max_eps=4, **ptrs):
    buf = (C.c_double * 16)()
    names = ('rew', 'st', 'tail', 'success_plane', 'progress', 'col_base',
             'length', 'undiscounted', 'discounted', 'terminated', 'success')
    a = {k: C.addressof(buf) for k in names}
    a.update(ptrs)
    _lib.call('ga_member_episode_statistics', a['rew'], a['st'], a['tail'],
              a['success_plane'], n, tcap, cols, members, samples, 0.99,
              a['progress'], a['col_base'], max_eps, a['length'],
              a['undiscounted'], a['discounted'], a['terminated'],
              a['success'], None)


@pytest.mark.parametrize('entry', [_progress, _statistics],
                         ids=['ga_member_progress',
                              'ga_member_episode_statistics'])
def test_bad_sizes_are_refused_without_a_gpu(entry):
    err = _lib.GarageAmdError
    for bad in (0, -2):
        with pytest.raises(err, match='n_members must be at least 1'):
            entry(members=bad)
    with pytest.raises(err, match='64 envs do not split into 3 members'):
        entry(members=3)
    for bad in (0, -1, TCAP + 1):
        with pytest.raises(err, match=r'n_cols must be in 1\.\.Tcap'):
            entry(cols=bad)
    for bad in (0, -5):
        with pytest.raises(err, match='num_samples must be at least 1'):
            entry(samples=bad)
    with pytest.raises(err, match='rollout buffers too large'):
        entry(n=1 << 20, tcap=1 << 11, cols=4)


def test_null_pointers_are_refused_without_a_gpu():
    err = _lib.GarageAmdError
    for name in ('tail', 'progress', 'col_base'):
        with pytest.raises(err, match='ga_member_progress: null pointer'):
            _progress(**{name: None})
    for name in ('rew', 'st', 'tail', 'progress', 'col_base', 'length',
                 'undiscounted', 'discounted', 'terminated'):
        with pytest.raises(
                err, match='ga_member_episode_statistics: null pointer'):
            _statistics(**{name: None})
    # a success plane needs somewhere to go; without one `success` may be NULL,
    # and the call gets as far as the next check
    with pytest.raises(err, match='null pointer'):
        _statistics(success=None)
    with pytest.raises(err, match='max_eps must be at least 1'):
        _statistics(success_plane=None, success=None, max_eps=0)
    assert b'ga_member_episode_statistics' in _lib.load().ga_last_error()


def test_header_cites_the_reference_and_the_abi_stays_5():
    text = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    for name in ('ga_member_progress', 'ga_member_episode_statistics'):
        assert 'GA_API int %s(' % name in text
        assert name in _lib.SIGNATURES
    start = text.index('a population\'s score from the raw rollout buffers')
    assert '_functions.py:233-275' in text[start:]
    assert _lib.load().ga_abi_version() == 5
