"""Generate the multi-task device-env fixture by running the REAL reference
``MultiEnvWrapper`` over the real ``PointEnv`` with ``round_robin_strategy``,
alone and through the real ``LocalSampler(VecWorker)``, and the rows the real
``log_multitask_performance`` records.

Run in the build container only (needs ``/root/reference``)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_multitask_envs.py

Writes ``multitask_point.npz`` (plain arrays only) next to this file;
``--check DIR`` writes it into DIR instead.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_harness as ref  # noqa: E402

ref.install()

from garage import StepType  # noqa: E402
import garage._functions as gfun  # noqa: E402
from garage.envs import PointEnv  # noqa: E402
from garage.envs.multi_env_wrapper import (MultiEnvWrapper,  # noqa: E402
                                           round_robin_strategy)
from garage.sampler import LocalSampler, VecWorker, WorkerFactory  # noqa: E402

from make_golden_device_envs import (SAMPLER_C, SAMPLER_P,  # noqa: E402
                                     sampler_noise)

OUT = HERE

# part 1: wrappers stepped by hand.  Every member is its own wrapper; the gains
# make their episodes end at different steps, so their tasks drift apart.
WRAP_GOALS = [(0.25, 0.2), (-0.2, 0.15), (0.1, -0.3), (0.35, 0.35)]
WRAP_KS = (1, 3, 4)
WRAP_MODES = ('add-onehot', 'vanilla')
WRAP_GAINS = (1.3, 0.9, 0.4)
WRAP_CFG = dict(arena_size=0.35, done_bonus=1.5, max_episode_length=5)
WRAP_T = 48

# part 2: the scripted policy of point_sampler.npz (it steers at SAMPLER_C): the
# first two goals are reached, the third is not (those episodes time out)
SAMPLER_GOALS = [(0.33, 0.08), (0.4, 0.27), (-0.5, 0.5)]
SAMPLER_NAMES = ['near', 'nearer', 'far']
SAMPLER_N = 4
SAMPLER_BONUS = 1.5
NAME_MAP = {0: 'zero', 1: 'one', 2: 'two'}


def _done(st):
    return st in (StepType.TERMINAL, StepType.TIMEOUT)


def _wrapper(goals, mode, names=None, env_cls=PointEnv, **cfg):
    return MultiEnvWrapper([env_cls(goal=g, **cfg) for g in goals],
                           sample_strategy=round_robin_strategy, mode=mode,
                           env_names=names)


def gen_wrapper(out):
    rng = np.random.RandomState(11)
    for K in WRAP_KS:
        for mode in WRAP_MODES:
            tag = 'k%d_%s_' % (K, mode.replace('-', ''))
            goals = np.asarray(WRAP_GOALS[:K], np.float32)
            envs = [_wrapper(WRAP_GOALS[:K], mode, **WRAP_CFG)
                    for _ in WRAP_GAINS]
            n, D = len(envs), 3 + (K if mode == 'add-onehot' else 0)
            assert envs[0].spec.observation_space.shape == (D, )
            obs = np.stack([e.reset()[0] for e in envs])
            out[tag + 'obs0'] = obs.astype(np.float32)
            acts = np.zeros((WRAP_T, n, 2), np.float32)
            nxt = np.zeros((WRAP_T, n, D), np.float32)
            after = np.zeros((WRAP_T, n, D), np.float32)
            rew = np.zeros((WRAP_T, n), np.float32)
            st = np.zeros((WRAP_T, n), np.uint8)
            succ = np.zeros((WRAP_T, n), bool)
            task = np.zeros((WRAP_T, n), np.int64)
            for t in range(WRAP_T):
                # the steering rule of point_env.npz, at the active task's goal
                active = goals[[e.active_task_index for e in envs]]
                a = ((active - obs[:, :2]) * np.asarray(WRAP_GAINS)[:, None] +
                     rng.normal(0, 0.05, (n, 2))).astype(np.float32)
                if t % 11 == 5:
                    a[0] = np.float32([3.0, -3.0])  # far outside the action box
                acts[t] = a
                for i, e in enumerate(envs):
                    es = e.step(a[i])
                    assert es.observation.dtype == (
                        np.float64 if mode == 'add-onehot' else np.float32)
                    nxt[t, i] = es.observation
                    rew[t, i] = es.reward
                    st[t, i] = int(es.step_type)
                    succ[t, i] = es.env_info['success']
                    assert isinstance(es.env_info['task_id'], int)
                    task[t, i] = es.env_info['task_id']
                    after[t, i] = (e.reset()[0] if _done(es.step_type) else
                                   es.observation)
                obs = after[t]
            assert np.array_equal(nxt.astype(np.float64).astype(np.float32),
                                  nxt)
            out.update({tag + 'actions': acts, tag + 'next_obs': nxt,
                        tag + 'obs_after': after, tag + 'reward': rew,
                        tag + 'step_type': st, tag + 'success': succ,
                        tag + 'task_id': task})
    out['wrap_goals'] = np.asarray(WRAP_GOALS, np.float32)
    out['wrap_cfg'] = np.asarray([WRAP_CFG['arena_size'],
                                  WRAP_CFG['done_bonus'],
                                  WRAP_CFG['max_episode_length']])


class ScriptedPointPolicy:
    """The scripted policy of make_golden_device_envs.py; it also keeps what
    the reference ``VecWorker`` loses, the observations it was handed: the
    worker stores views of one array it overwrites (vec_worker.py:188), so its
    batch holds every episode's final observation in all the episode's rows.
    ``agent.reset(completes)`` (vec_worker.py:202-203) says which episodes
    ended with the last call."""

    def __init__(self, n):
        self.calls = 0
        self.name = 'scripted'
        self._n = n
        self.begin()

    def begin(self):
        self._cur = [[] for _ in range(self._n)]
        self.episodes = []
        self._stepped = False

    def reset(self, do_resets=None):
        if self._stepped:
            for i, done in enumerate(do_resets):
                if done:
                    self.episodes.append(np.asarray(self._cur[i]))
                    self._cur[i] = []
        self._stepped = False

    def get_actions(self, observations):
        for i, o in enumerate(observations):
            self._cur[i].append(np.array(o, copy=True))
        self._stepped = True
        obs = np.asarray(observations, dtype=np.float32)
        mu = (-obs[:, :2]) + SAMPLER_C
        a = (mu + sampler_noise(self.calls, obs.shape[0])).astype(np.float32)
        self.calls += 1
        return a, {}

    def get_param_values(self):
        return None

    def set_param_values(self, _):
        pass


class _NoEpisodeInfoPointEnv(PointEnv):
    """The reference PointEnv without reset()'s episode_info: the reference
    VecWorker cannot pack a vector-valued one (``ValueError: Entry 'goal' in
    episode_infos has batch size 2``)."""

    def reset(self):
        return super().reset()[0], {}


def gen_sampler(out):
    n, P, K = SAMPLER_N, SAMPLER_P, len(SAMPLER_GOALS)
    for start in ('same', 'spread'):
        for named in (True, False):
            tag = '%s_%s_' % (start, 'named' if named else 'ids')
            names = SAMPLER_NAMES if named else None
            for mode in WRAP_MODES:
                mtag = tag + mode.replace('-', '') + '_'

                def make():
                    return _wrapper(SAMPLER_GOALS, mode, names,
                                    env_cls=_NoEpisodeInfoPointEnv,
                                    done_bonus=SAMPLER_BONUS,
                                    max_episode_length=P)

                if start == 'same':  # VecWorker deep-copies it n times
                    envs = make()
                else:                # member i begins with task i % K
                    envs = [make() for _ in range(n)]
                    for i, e in enumerate(envs):
                        e._active_task_index = (i % K - 1) if i % K else None
                    envs = [envs]
                pol = ScriptedPointPolicy(n)
                wf = WorkerFactory(seed=1, n_workers=1, worker_class=VecWorker,
                                   worker_args=dict(n_envs=n),
                                   max_episode_length=P)
                sampler = LocalSampler.from_worker_factory(wf, pol, envs)
                for prefix, num in (('a_', 40), ('b_', 23)):
                    pol.begin()
                    eps = sampler.obtain_samples(0, num, None)
                    true_obs = np.concatenate(pol.episodes)
                    assert true_obs.shape == eps.observations.shape
                    assert [len(e) for e in pol.episodes] == list(eps.lengths)
                    p = mtag + prefix
                    out.update({
                        p + 'observations': eps.observations,
                        p + 'true_observations': true_obs,
                        p + 'last_observations': eps.last_observations,
                        p + 'actions': eps.actions,
                        p + 'rewards': eps.rewards,
                        p + 'step_types': np.asarray(
                            [int(s) for s in eps.step_types]),
                        p + 'lengths': eps.lengths,
                        p + 'success': np.asarray(eps.env_infos['success']),
                        p + 'task_id': np.asarray(eps.env_infos['task_id']),
                    })
                    if named:
                        out[p + 'task_name'] = np.asarray(
                            eps.env_infos['task_name'])
                    assert ('task_name' in eps.env_infos) == named
                    if prefix == 'b_' and mode == 'add-onehot':
                        # part 3: the rows of log_multitask_performance
                        rec = ref.TabularRecorder()
                        gfun.tabular = rec
                        und = gfun.log_multitask_performance(
                            7, eps, 0.9, name_map=None if named else NAME_MAP)
                        out[tag + 'log_undiscounted'] = np.asarray(und)
                        out[tag + 'log_keys'] = np.asarray(
                            list(rec.values.keys()))
                        out[tag + 'log_vals'] = np.asarray(
                            [float(v) for v in rec.values.values()])
    out['sampler_goals'] = np.asarray(SAMPLER_GOALS, np.float32)
    out['sampler_names'] = np.asarray(SAMPLER_NAMES)
    out['sampler_cfg'] = np.asarray([P, n])
    out['sampler_bonus'] = np.asarray(SAMPLER_BONUS)
    out['sampler_c'] = SAMPLER_C
    out['name_map_keys'] = np.asarray(list(NAME_MAP.keys()))
    out['name_map_vals'] = np.asarray(list(NAME_MAP.values()))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--check':
        OUT = sys.argv[2]
    arrays = {}
    gen_wrapper(arrays)
    gen_sampler(arrays)
    path = os.path.join(OUT, 'multitask_point.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path)
