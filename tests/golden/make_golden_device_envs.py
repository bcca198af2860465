"""Generate the device-env fixtures by running the REAL reference ``PointEnv``,
``GridWorldEnv`` and ``VecWorker``.

Run in the build container only (needs ``/root/reference``)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_device_envs.py

Writes ``point_env.npz``, ``grid_env.npz`` and ``point_sampler.npz`` (plain
arrays only) next to this file; ``--check DIR`` writes them into DIR instead.
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
from garage.envs import GridWorldEnv, PointEnv  # noqa: E402
from garage.sampler import LocalSampler, VecWorker, WorkerFactory  # noqa: E402

OUT = HERE

# PointEnv groups: one device batch each (shared arena / bonus / never_done,
# one goal per env; goals on the arena edge included)
POINT_GROUPS = [
    dict(arena=0.35, bonus=2.5, never_done=False, max_len=12,
         goals=[(0.3, 0.3), (0.35, -0.35), (-0.2, 0.1), (0.0, 0.05)]),
    dict(arena=5.0, bonus=0.7, never_done=True, max_len=9,
         goals=[(1.0, 1.0), (0.1, 0.1), (-0.05, 0.02), (5.0, -5.0)]),
    dict(arena=1.5, bonus=-0.3, never_done=False, max_len=20,
         goals=[(0.12, -0.07), (-1.5, 1.5), (0.4, 0.0)]),
]
POINT_T = 40

GRID_CASES = [('4x4', 15), ('4x4_safe', 12), ('8x8', 25), ('chain', 30),
              (['SxFFo', 'FxFxF', '.FFxG'], 14)]
GRID_T = 60

# the scripted policy of point_sampler: action = (C - point) + z(step, env)
SAMPLER_GOALS = [(0.3, 0.2), (0.25, 0.25), (1.0, 1.0), (-0.5, 0.5)]
SAMPLER_C = np.asarray([0.3, 0.2], dtype=np.float32)
SAMPLER_P = 8


def save(name, **arrays):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path)


def sampler_noise(step, n):
    """The scripted perturbation z (float32, [n, 2]) of vectorised step `step`."""
    i = np.arange(n)
    z0 = 0.02 * (((step * 7 + i * 3) % 5) - 2)
    z1 = 0.015 * (((step * 5 + i * 2) % 7) - 3)
    return np.stack([z0, z1], axis=1).astype(np.float32)


def _done(st):
    return st in (StepType.TERMINAL, StepType.TIMEOUT)


def gen_point():
    out = {}
    rng = np.random.RandomState(7)
    for k, g in enumerate(POINT_GROUPS):
        envs = [PointEnv(goal=goal, arena_size=g['arena'], done_bonus=g['bonus'],
                         never_done=g['never_done'], max_episode_length=g['max_len'])
                for goal in g['goals']]
        n = len(envs)
        obs = np.stack([e.reset()[0] for e in envs])
        out['g%d_obs0' % k] = obs.astype(np.float32)
        acts = np.zeros((POINT_T, n, 2), np.float32)
        nxt = np.zeros((POINT_T, n, 3), np.float32)
        after = np.zeros((POINT_T, n, 3), np.float32)
        rew = np.zeros((POINT_T, n), np.float32)
        st = np.zeros((POINT_T, n), np.uint8)
        succ = np.zeros((POINT_T, n), bool)
        goals = np.asarray(g['goals'], np.float32)
        for t in range(POINT_T):
            # steer at the goal with gains that overshoot the +-0.1 clip
            a = ((goals - obs[:, :2]) * 1.3 +
                 rng.normal(0, 0.08, (n, 2))).astype(np.float32)
            if t % 11 == 5:
                a[0] = np.float32([3.0, -3.0])  # far outside the action box
            acts[t] = a
            for i, e in enumerate(envs):
                es = e.step(a[i])
                nxt[t, i] = es.observation
                rew[t, i] = es.reward
                st[t, i] = int(es.step_type)
                succ[t, i] = es.env_info['success']
                after[t, i] = (e.reset()[0] if _done(es.step_type) else
                               es.observation)
            obs = after[t]
        out.update({'g%d_cfg' % k: np.asarray([g['arena'], g['bonus'],
                                               float(g['never_done']),
                                               g['max_len']]),
                    'g%d_goals' % k: goals, 'g%d_actions' % k: acts,
                    'g%d_next_obs' % k: nxt, 'g%d_obs_after' % k: after,
                    'g%d_reward' % k: rew, 'g%d_step_type' % k: st,
                    'g%d_success' % k: succ})
    out['n_groups'] = np.asarray(len(POINT_GROUPS))
    # PointEnv.sample_tasks: the draw of numpy's global RNG
    np.random.seed(123)
    out['sample_tasks_seed123'] = np.stack(
        [t['goal'] for t in PointEnv().sample_tasks(5)])
    save('point_env', **out)


def gen_grid():
    out = {}
    rng = np.random.RandomState(3)
    for k, (desc, max_len) in enumerate(GRID_CASES):
        n = 3
        envs = [GridWorldEnv(desc=desc, max_episode_length=max_len)
                for _ in range(n)]
        s = np.asarray([e.reset()[0] for e in envs])
        out['c%d_start' % k] = s
        acts = rng.choice(4, size=(GRID_T, n), p=[0.1, 0.4, 0.4, 0.1])
        nxt = np.zeros((GRID_T, n), np.int64)
        after = np.zeros((GRID_T, n), np.int64)
        rew = np.zeros((GRID_T, n), np.float32)
        st = np.zeros((GRID_T, n), np.uint8)
        for t in range(GRID_T):
            for i, e in enumerate(envs):
                es = e.step(int(acts[t, i]))
                nxt[t, i] = es.observation
                rew[t, i] = es.reward
                st[t, i] = int(es.step_type)
                after[t, i] = (e.reset()[0] if _done(es.step_type) else
                               es.observation)
        rows = desc if isinstance(desc, list) else []
        out.update({'c%d_name' % k: np.asarray(desc if isinstance(desc, str)
                                               else ''),
                    'c%d_rows' % k: np.asarray(rows, dtype='U'),
                    'c%d_max_len' % k: np.asarray(max_len),
                    'c%d_actions' % k: acts, 'c%d_next' % k: nxt,
                    'c%d_after' % k: after, 'c%d_reward' % k: rew,
                    'c%d_step_type' % k: st})
    out['n_cases'] = np.asarray(len(GRID_CASES))
    save('grid_env', **out)


class ScriptedPointPolicy:
    """action = (C - point) + z(step): what a linear Gaussian policy with weight
    [[-1, 0, 0], [0, -1, 0]], bias C, std 1 and noise z computes in fp32."""

    def __init__(self):
        self.calls = 0
        self.name = 'scripted'

    def reset(self, do_resets=None):
        pass

    def get_actions(self, observations):
        obs = np.asarray(observations, dtype=np.float32)
        mu = (-obs[:, :2]) + SAMPLER_C
        a = (mu + sampler_noise(self.calls, obs.shape[0])).astype(np.float32)
        self.calls += 1
        return a, {}

    def get_param_values(self):
        return None

    def set_param_values(self, _):
        pass


def _episode_goals(eps, goals):
    """The goal of each episode: the one whose distance from the episode's last
    point is the distance its last observation reports.  (The reference
    VecWorker cannot pack a non-scalar episode_info -- vec_worker.py:142-153
    makes the goal itself the batch axis -- nor keep per-env env_infos apart
    before an env's first reset, vec_worker.py:56-58; its last observations are
    exact.)"""
    out = []
    for last in eps.last_observations:
        hit = [g for g in goals
               if np.linalg.norm(last[:2] - g) == last[2]]
        assert len(hit) == 1, (last, hit)
        out.append(hit[0])
    return np.asarray(out, np.float32)


class _NoEpisodeInfoPointEnv(PointEnv):
    """The reference PointEnv without reset()'s episode_info (see above)."""

    def reset(self):
        return super().reset()[0], {}


def gen_point_sampler():
    n, P = len(SAMPLER_GOALS), SAMPLER_P
    envs = [_NoEpisodeInfoPointEnv(goal=g, done_bonus=1.5, max_episode_length=P)
            for g in SAMPLER_GOALS]
    wf = WorkerFactory(seed=1, n_workers=1, worker_class=VecWorker,
                       worker_args=dict(n_envs=n), max_episode_length=P)
    sampler = LocalSampler.from_worker_factory(wf, ScriptedPointPolicy(),
                                               [envs])
    out = {}
    for prefix, num in (('a_', 40), ('b_', 23)):
        eps = sampler.obtain_samples(0, num, None)
        out.update({
            prefix + 'observations': eps.observations,
            prefix + 'last_observations': eps.last_observations,
            prefix + 'actions': eps.actions,
            prefix + 'rewards': eps.rewards,
            prefix + 'step_types': np.asarray([int(s) for s in eps.step_types]),
            prefix + 'lengths': eps.lengths,
            prefix + 'success': np.asarray(eps.env_infos['success']),
            prefix + 'goal': _episode_goals(
                eps, np.asarray(SAMPLER_GOALS, np.float32)),
        })
    out['goals'] = np.asarray(SAMPLER_GOALS, np.float32)
    out['cfg'] = np.asarray([P, n])
    out['c'] = SAMPLER_C
    save('point_sampler', **out)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--check':
        OUT = sys.argv[2]
    gen_point()
    gen_grid()
    gen_point_sampler()
