"""``MultiTaskPointVecEnv``, the parts that need no GPU: a numpy twin of the
reference ``MultiEnvWrapper`` over ``PointTwin`` reproduces the committed
fixture (which the real wrapper, ``PointEnv`` and ``VecWorker`` produced,
tests/golden/make_golden_multitask_envs.py) bit for bit, the uniform random
task draw against its numpy restatement, the constructor's argument checks, the
C struct and the C ABI's argument errors.  The GPU tests
(test_multitask_envs_gpu.py) hold the kernels to the same fixture and to
``HostVecEnv`` batches of this twin."""
import collections
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from garage_amd._dtypes import Box, EnvSpec
from oracle import batch as ob
from oracle import sampler as osamp
from oracle.envs import philox4x32
from test_device_envs_cpu import PointTwin, _ended

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM_TASK = 4  # csrc/rollout_dev.h
MODES = ('add-onehot', 'vanilla')


def task_draw_np(seed, env, counter, num_tasks):
    """csrc/rollout_dev.h ``task_draw``: the high half of ``u * K`` for the
    first word ``u`` of the Philox block ``(env, counter, 0, STREAM_TASK << 16)``."""
    u = philox4x32(env, counter, 0, STREAM_TASK << 16, seed)[0]
    return ((u.astype(np.uint64) * np.uint64(num_tasks)) >>
            np.uint64(32)).astype(np.int64)


class TwinStep(collections.namedtuple(
        'TwinStep', 'observation reward step_type env_info action')):
    """The fields the device sampler and the restated workers of
    oracle/sampler.py read of an ``EnvStep``."""

    last = property(lambda self: _ended(self.step_type))


class MultiTaskPointTwin:
    """``MultiEnvWrapper([PointEnv(goal=g, **cfg) for g in goals], ...)``
    (envs/multi_env_wrapper.py:169-226) over ``PointTwin`` in plain numpy.
    ``strategy='random'`` is the device's Philox draw for member ``env_id``,
    not the reference's ``random.randint``."""

    def __init__(self, goals, strategy='round_robin', mode='add-onehot',
                 env_names=None, last_task=None, seed=0, env_id=0, **cfg):
        self._tasks = [PointTwin(goal=g, **cfg) for g in goals]
        self._strategy, self._mode, self._names = strategy, mode, env_names
        self._active = last_task
        self._seed, self._env_id, self._resets = seed, env_id, 0
        K = len(goals)
        D = 3 + (K if mode == 'add-onehot' else 0)
        self.spec = EnvSpec(Box(-np.inf, np.inf, (D, )), Box(-0.1, 0.1, (2, )),
                            max_episode_length=cfg.get('max_episode_length'))

    active_task_index = property(lambda self: self._active)

    def _obs(self, obs):
        if self._mode == 'vanilla':
            return obs
        one_hot = np.zeros(len(self._tasks))
        one_hot[self._active] = 1.0
        return np.concatenate([obs, one_hot])

    def reset(self):
        K = len(self._tasks)
        if self._strategy == 'random':
            self._active = int(task_draw_np(self._seed, self._env_id,
                                            self._resets, K))
        else:
            self._active = (0 if self._active is None else
                            (self._active + 1) % K)
        self._resets += 1
        obs, info = self._tasks[self._active].reset()
        return self._obs(obs), info

    def step(self, action):
        es = self._tasks[self._active].step(action)
        info = dict(es.env_info, task_id=self._active)
        if self._names is not None:
            info['task_name'] = self._names[self._active]
        return TwinStep(self._obs(es.observation), es.reward, es.step_type,
                        info, action)

    def close(self):
        pass


def wrapper_cases(g):
    arena, bonus, max_len = g['wrap_cfg']
    cfg = dict(arena_size=float(arena), done_bonus=float(bonus),
               max_episode_length=int(max_len))
    for K in (1, 3, 4):
        for mode in MODES:
            yield ('k%d_%s_' % (K, mode.replace('-', '')), g['wrap_goals'][:K],
                   mode, cfg)


def sampler_cases(g):
    """(tag, mode, start, env_names) of fixture part 2."""
    names = [str(s) for s in g['sampler_names']]
    for start in ('same', 'spread'):
        for named in (True, False):
            for mode in MODES:
                tag = '%s_%s_%s_' % (start, 'named' if named else 'ids',
                                     mode.replace('-', ''))
                yield tag, mode, start, names if named else None


def sampler_twins(g, mode, start, names, strategy='round_robin', seed=0):
    P, n = [int(v) for v in g['sampler_cfg']]
    K = len(g['sampler_goals'])
    return [MultiTaskPointTwin(
        g['sampler_goals'], strategy, mode, names,
        last_task=((i % K - 1) if i % K else None) if start == 'spread' else
        None, seed=seed, env_id=i, done_bonus=float(g['sampler_bonus']),
        max_episode_length=P) for i in range(n)], P, n


def sampler_noise(step, n):
    """The scripted z of make_golden_device_envs.py (float32, [n, 2])."""
    i = np.arange(n)
    z0 = 0.02 * (((step * 7 + i * 3) % 5) - 2)
    z1 = 0.015 * (((step * 5 + i * 2) % 7) - 3)
    return np.stack([z0, z1], axis=1).astype(np.float32)


class _Scripted:
    """action = (c - point) + z(step): the fixture's scripted policy."""

    def __init__(self, c):
        self.calls, self._c = 0, c

    def reset(self, do_resets=None):
        pass

    def get_actions(self, observations):
        obs = np.asarray(observations, dtype=np.float32)
        a = ((-obs[:, :2]) + self._c +
             sampler_noise(self.calls, obs.shape[0])).astype(np.float32)
        self.calls += 1
        return a, {}


def test_twin_reproduces_the_reference_wrapper(golden):
    g = golden('multitask_point')
    for tag, goals, mode, cfg in wrapper_cases(g):
        envs = [MultiTaskPointTwin(goals, mode=mode, **cfg) for _ in range(3)]
        obs0 = np.stack([e.reset()[0] for e in envs])
        assert np.array_equal(obs0, g[tag + 'obs0']), tag
        for t, acts in enumerate(g[tag + 'actions']):
            for i, e in enumerate(envs):
                es = e.step(acts[i])
                assert np.array_equal(es.observation,
                                      g[tag + 'next_obs'][t, i]), (tag, t, i)
                assert np.float32(es.reward) == g[tag + 'reward'][t, i]
                assert int(es.step_type) == g[tag + 'step_type'][t, i]
                assert es.env_info['success'] == g[tag + 'success'][t, i]
                assert es.env_info['task_id'] == g[tag + 'task_id'][t, i]
                if _ended(es.step_type):
                    assert np.array_equal(e.reset()[0],
                                          g[tag + 'obs_after'][t, i])
        if len(goals) > 1:  # the members' tasks drift apart
            assert (g[tag + 'task_id'][:, 0] != g[tag + 'task_id'][:, 2]).any()


@pytest.mark.parametrize('alias_bug', [True, False])
def test_twin_through_the_vec_worker_reproduces_the_reference(golden,
                                                              alias_bug):
    """``alias_bug=True`` is the reference ``VecWorker`` as it is (every row of
    an episode's observations is its final observation) and
    gives the fixture's ``observations``; without it the restated worker gives
    ``true_observations``, what the reference policy was handed."""
    g = golden('multitask_point')
    for tag, mode, start, names in sampler_cases(g):
        envs, P, n = sampler_twins(g, mode, start, names)
        s = osamp.OracleLocalSampler(
            _Scripted(g['sampler_c']), [envs], max_episode_length=P,
            n_workers=1, worker_class=osamp.OracleVecWorker,
            worker_args=dict(n_envs=n, alias_bug=alias_bug))
        for prefix, num in (('a_', 40), ('b_', 23)):
            p = tag + prefix
            eps = s.obtain_samples(0, num, None)
            assert np.array_equal(eps.lengths, g[p + 'lengths']), p
            assert np.array_equal([int(x) for x in eps.step_types],
                                  g[p + 'step_types'])
            want_obs = g[p + ('observations' if alias_bug else
                              'true_observations')]
            assert np.array_equal(eps.observations, want_obs), p
            for key in ('last_observations', 'actions', 'rewards'):
                assert np.array_equal(getattr(eps, key), g[p + key]), (p, key)
            for key in ('success', 'task_id') + (('task_name', )
                                                 if names else ()):
                assert np.array_equal(eps.env_infos[key], g[p + key]), (p, key)
            assert ('task_name' in eps.env_infos) == bool(names)
            assert g[p + 'task_id'].dtype == np.int64
            if mode == 'add-onehot':  # the one-hot columns are the task's
                K = len(g['sampler_goals'])
                assert np.array_equal(g[p + 'true_observations'][:, 3:],
                                      np.eye(K)[g[p + 'task_id']])
    # the second call starts every member on the task after the one it was
    # cut off in: the two batches of a case differ
    assert not np.array_equal(g['same_named_addonehot_a_lengths'],
                              g['same_named_addonehot_b_lengths'])


def test_twin_batch_gives_the_reference_multitask_rows(golden):
    from test_oracle_golden import check_multitask
    g = golden('multitask_point')
    name_map = dict(zip((int(k) for k in g['name_map_keys']),
                        (str(v) for v in g['name_map_vals'])))
    for tag, mode, start, names in sampler_cases(g):
        if mode != 'add-onehot':
            continue
        envs, P, n = sampler_twins(g, mode, start, names)
        s = osamp.OracleLocalSampler(
            _Scripted(g['sampler_c']), [envs], max_episode_length=P,
            n_workers=1, worker_class=osamp.OracleVecWorker,
            worker_args=dict(n_envs=n))
        s.obtain_samples(0, 40, None)
        eps = s.obtain_samples(1, 23, None)
        rec, und = ob.multitask_performance_stats(
            7, eps, 0.9, name_map=None if names else name_map)
        ltag = tag[:-len(mode.replace('-', '')) - 1] + 'log'
        check_multitask(g, ltag, rec, und)


@pytest.mark.ref
def test_fixture_regenerates_identically_from_the_reference():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.join(
            ROOT, 'tests', 'golden', 'make_golden_multitask_envs.py'),
                        '--check', tmp], check=True, capture_output=True,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
        with open(os.path.join(tmp, 'multitask_point.npz'), 'rb') as f:
            new = f.read()
        with open(os.path.join(ROOT, 'tests', 'golden',
                               'multitask_point.npz'), 'rb') as f:
            assert f.read() == new  # byte for byte


def test_constructor_checks_its_arguments_before_any_device_work():
    from garage_amd import envs
    from garage_amd.envs import MultiTaskPointVecEnv as Env
    goals = [(0.1, 0.1), (0.2, -0.1), (-0.3, 0.)]
    kw = dict(max_episode_length=5)
    assert envs.round_robin_strategy(3) == 0
    assert envs.round_robin_strategy(3, 2) == 0
    assert envs.round_robin_strategy(3, 0) == 1
    assert 0 <= envs.uniform_random_strategy(3, None) < 3
    with pytest.raises(ValueError, match='del-onehot'):
        Env(4, goals, mode='del-onehot', **kw)
    with pytest.raises(ValueError, match='mode must be'):
        Env(4, goals, mode='one-hot', **kw)
    with pytest.raises(NotImplementedError, match='sample_strategy'):
        Env(4, goals, sample_strategy=lambda k, last: 0, **kw)
    with pytest.raises(ValueError, match='must be a list'):
        Env(4, goals, env_names=('a', 'b', 'c'), **kw)
    with pytest.raises(ValueError, match='not unique'):
        Env(4, goals, env_names=['a', 'b', 'a'], **kw)
    with pytest.raises(ValueError, match='not unique'):
        Env(4, goals, env_names=['a', 'b'], **kw)
    with pytest.raises(ValueError, match='start must be'):
        Env(4, goals, start='random', **kw)
    with pytest.raises(ValueError, match='finite'):
        Env(4, goals)
    with pytest.raises(ValueError, match='outside the arena'):
        Env(4, goals + [(3., 0.)], arena_size=2., **kw)
    with pytest.raises(ValueError, match=r'\(K, 2\)'):
        Env(4, [], **kw)
    with pytest.raises(ValueError, match='at most 256 tasks'):
        Env(4, np.zeros((257, 2)), **kw)


def test_new_ctypes_struct_matches_the_header():
    from garage_amd import _lib
    cname, py = 'ga_multi_point_env', _lib.MultiPointEnv
    consts = ['GA_ENV_MULTI_POINT', 'GA_TASK_ROUND_ROBIN',
              'GA_TASK_UNIFORM_RANDOM', 'GA_TASK_VANILLA', 'GA_TASK_ADD_ONEHOT']
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("{}\\n", {});'.format(
                 ' '.join(['%d'] * len(consts)), ', '.join(consts)),
             'printf("{0} %zu\\n", sizeof({0}));'.format(cname)]
    want = ['{} {} {} {} {}'.format(
        _lib.ENV_MULTI_POINT, _lib.TASK_ROUND_ROBIN, _lib.TASK_UNIFORM_RANDOM,
        _lib.TASK_VANILLA, _lib.TASK_ADD_ONEHOT),
            '{} {}'.format(cname, ctypes.sizeof(py))]
    for field, ftype in py._fields_:
        lines.append('printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                     'sizeof((({0}*)0)->{1}));'.format(cname, field))
        want.append('{}.{} {} {}'.format(cname, field,
                                         getattr(py, field).offset,
                                         ctypes.sizeof(ftype)))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe],
                       check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == want
    # the ga_point_env fields come first, in ga_point_env's layout
    for field, _ in _lib.PointEnv._fields_:
        assert (getattr(py, field).offset ==
                getattr(_lib.PointEnv, field).offset), field
    assert _lib.load().ga_abi_version() == 5


def test_new_entry_points_report_argument_errors_without_a_gpu():
    from garage_amd import _lib
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)

    def env(**kw):
        e = _lib.MultiPointEnv(n=4, max_episode_length=5, point=addr,
                               goal=addr, t=addr, task_goals=addr,
                               last_task=addr, resets=addr, num_tasks=3,
                               strategy=_lib.TASK_ROUND_ROBIN,
                               mode=_lib.TASK_ADD_ONEHOT)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(_lib.env_ref(_lib.ENV_MULTI_POINT, e))

    def reset(e, ldo=8):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=8):
        _lib.call('ga_env_step', e, addr, 4, None, addr, ldo, addr, addr, None)

    def record(e, rec):
        _lib.call('ga_env_step_record', e, C.byref(rec), None, addr, 4, addr,
                  None)

    rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5,
                          reward=addr, step_type=addr, next_obs=addr, ldo=4,
                          obs_dim=6, ep_t=addr, rew_buf=addr, st_buf=addr,
                          tail_buf=addr, lastobs_buf=addr, done=addr,
                          step_eps=addr, step_samples=addr)
    for fn in (reset, step, lambda e: record(e, rec)):
        for field in ('point', 'goal', 't', 'task_goals', 'last_task',
                      'resets'):
            with pytest.raises(_lib.GarageAmdError, match='null env state'):
                fn(env(**{field: None}))
        with pytest.raises(_lib.GarageAmdError, match='num_tasks must be'):
            fn(env(num_tasks=0))
        with pytest.raises(_lib.GarageAmdError, match='num_tasks must be'):
            fn(env(num_tasks=257))
        with pytest.raises(_lib.GarageAmdError, match='unknown mode 2'):
            fn(env(mode=2))
        with pytest.raises(_lib.GarageAmdError,
                           match='unknown sample strategy'):
            fn(env(strategy=5))
        with pytest.raises(_lib.GarageAmdError, match='max_episode_length'):
            fn(env(max_episode_length=0))
    # a row narrower than 3 + K
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(env(), ldo=5)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(env(), ldo=5)
    with pytest.raises(_lib.GarageAmdError, match=r'narrower than 3 \+ num'):
        record(env(), rec)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_env_step', env(), None, 4, None, None, 8, None, None,
                  None)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        record(env(), _lib.RecordArgs(n=4, Tcap=8, ldo=8, obs_dim=6))
    assert _lib.load().ga_multi_env_task_draw(0, 0, 0, 0) < 0
    assert _lib.load().ga_multi_env_task_draw(0, 0, 0, 257) < 0


def test_host_task_draw_equals_its_numpy_restatement():
    from garage_amd.envs import task_draw
    rng = np.random.RandomState(5)
    m = 4000
    env = rng.randint(0, 1 << 20, m)
    cnt = rng.randint(0, 1 << 16, m)
    K = rng.randint(1, 257, m)
    for seed in (0, 3, (7 << 32) | 11):
        want = np.asarray([int(task_draw_np(seed, e, c, k))
                           for e, c, k in zip(env[:300], cnt[:300], K[:300])])
        got = [task_draw(seed, e, c, k)
               for e, c, k in zip(env[:300], cnt[:300], K[:300])]
        assert np.array_equal(got, want)
    # vectorised over the lot for one K at a time
    for k in (1, 2, 7, 16, 256):
        want = task_draw_np(9, env, cnt, k)
        got = [task_draw(9, e, c, k) for e, c in zip(env, cnt)]
        assert np.array_equal(got, want)
        assert want.min() >= 0 and want.max() < k
    with pytest.raises(ValueError, match='num_tasks'):
        task_draw(0, 0, 0, 0)


def test_task_draw_is_uniform_over_the_tasks():
    """600 members x 100 resets, K = 7, seed 0: every task's count lies within
    5 standard deviations of 60 000 / 7 (a fixed sample: the largest deviation
    is printed; binomial sd = sqrt(N p (1 - p)))."""
    from garage_amd.envs import task_draw
    K, n_env, n_reset = 7, 600, 100
    env, cnt = np.meshgrid(np.arange(n_env), np.arange(n_reset),
                           indexing='ij')
    tasks = task_draw_np(0, env.ravel(), cnt.ravel(), K)
    assert [task_draw(0, e, c, K) for e, c in ((0, 0), (599, 99), (17, 3))] \
        == [tasks[0], tasks[-1], tasks[17 * n_reset + 3]]
    N = tasks.size
    counts = np.bincount(tasks, minlength=K)
    sd = np.sqrt(N * (1 / K) * (1 - 1 / K))
    dev = np.abs(counts - N / K) / sd
    print('task counts', counts.tolist(), 'deviations (sd)',
          np.round(dev, 2).tolist())
    assert N == 60000 and dev.max() < 5.0
    # a member's sequence is not a constant or a cycle of the round robin
    seq = tasks.reshape(n_env, n_reset)
    assert (np.diff(seq, axis=1) % K != 1).any(axis=1).all()
