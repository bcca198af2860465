"""Env-steps per second of ``GpuVecSampler.obtain_samples`` with one of the
seeded state-vector env kinds against ``SyntheticVecEnv`` of the same shape and
against a neighbouring kind: 4096 envs, a policy with hidden (64, 64),
categorical for the kinds that take a class and Gaussian for the others.

    python tools/state_env_rate.py --kind cartpole [--envs 4096] [--T 128]
                                                   [--reps 7]
    python tools/state_env_rate.py --kind pendulum [--T 200] [--reps 7]
    python tools/state_env_rate.py --kind double_pendulum [--T 200] [--reps 15]
    python tools/state_env_rate.py --kind acrobot [--T 200] [--reps 15]
    python tools/state_env_rate.py --kind mountain_car [--T 200] [--reps 15]

Rows of ``obtain_samples(n * T)``, max_episode_length = T, per kind:

``cartpole`` (BASELINE.json configs[1]'s size): ``cartpole`` (a random policy's
episodes last about 22 steps, so they end and restart inside the launch all the
time), ``synthetic`` (4 observations, 2 classes, every episode exactly T steps)
and ``synthetic_ragged`` (episode lengths uniform in 8..T: the same kind of
tail of Python-driven steps after the one launch, until the finished episodes
hold the samples asked for).

``pendulum`` (T = Pendulum-v0's TimeLimit): ``pendulum`` (every episode is
exactly T steps, so a call is one launch), ``synthetic`` (the same, 3
observations and 1 unbounded action, with a Philox draw for an env step:
``pendulum / synthetic`` is what the dynamics cost inside the launch) and
``pendulum_normalized`` (``normalize`` rescales the policy's action to the
torque bounds; the env thread of the one launch does it, so a call stays one
launch: ``pendulum_normalized / pendulum`` is what the rescale costs there).

``double_pendulum``: ``double_pendulum`` (under the untrained policy an episode
falls within 3 .. 16 steps, so the first T steps are one launch with the resets
inside it and the few steps that the in-flight episodes still lack are driven
from Python with a host check each), ``synthetic`` (11 observations, every
episode exactly T steps: a call is one launch), ``pendulum`` (the same) and
``double_pendulum_normalized`` (``normalize`` around the batch: the force is
rescaled inside the launch).

``acrobot`` / ``mountain_car`` (the discrete variant): the kind itself (under
the untrained policy no episode reaches its goal within T steps, so every
episode is exactly T steps and a call is one launch), ``synthetic_6`` /
``synthetic_2`` (the same observation width and three classes, every episode
exactly T steps) and ``cartpole`` (episodes of 10 .. 60 steps: the resets are
inside the launch and a tail of Python-driven steps follows it).

Rows of the launch alone, for the kinds that have them (``*_launch``: the T
steps of ``ga_rollout_env_steps`` into a preallocated buffer, no packing and no
tail): ``<kind>_launch / synthetic_launch`` is what the dynamics -- five
substeps of two sincos and a 3 x 3 solve for the double pendulum, four
evaluations of the two-link equations with two reductions and two sincos each
for Acrobot -- cost inside the launch against a Philox draw.

The samplers take turns within each repetition.  Prints one JSON line per row:
the median, min and max over ``reps`` calls of (env steps taken) / (wall time,
ended by a device synchronise), and one line with the kind's ratios.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _synthetic(obs_dim, act_dim, **kw):
    def env(envs, n, T):
        return envs.SyntheticVecEnv(n, obs_dim, act_dim, T, seed=1, **kw)
    return env


def _batch(name, normalized=False):
    def env(envs, n, T):
        e = getattr(envs, name)(n, max_episode_length=T, seed=1)
        return envs.NormalizedVecEnv(e) if normalized else e
    return env


def _discrete_task(task, batch, synth, obs_dim):
    """Acrobot's and MountainCar's rows: the task, a synthetic env of its
    shape and CartPole; the launch alone for the first two."""
    return dict(
        T=200, reps=15, policy='CategoricalMLPPolicy',
        rows={task: _batch(batch),
              synth: _synthetic(obs_dim, 3, discrete=True),
              'cartpole': _batch('CartPoleVecEnv')},
        launch=(task, synth),
        ratios={task + '_over_synthetic': (task, synth),
                task + '_over_cartpole': (task, 'cartpole'),
                'launch_' + task + '_over_synthetic':
                    (task + '_launch', synth + '_launch')})


# per kind: the defaults, the policy, the rows in the order they take turns
# (name -> env), the rows that are also timed as the launch alone, the ratios
KINDS = {
    'cartpole': dict(
        T=128, reps=7, policy='CategoricalMLPPolicy',
        rows={'cartpole': _batch('CartPoleVecEnv'),
              'synthetic': _synthetic(4, 2, discrete=True, min_len=None),
              'synthetic_ragged': _synthetic(4, 2, discrete=True, min_len=8)},
        launch=(),
        ratios={'cartpole_over_synthetic': ('cartpole', 'synthetic'),
                'cartpole_over_synthetic_ragged':
                    ('cartpole', 'synthetic_ragged')}),
    'pendulum': dict(
        T=200, reps=7, policy='GaussianMLPPolicy',
        rows={'pendulum': _batch('PendulumVecEnv'),
              'synthetic': _synthetic(3, 1),
              'pendulum_normalized': _batch('PendulumVecEnv',
                                            normalized=True)},
        launch=('pendulum', 'synthetic', 'pendulum_normalized'),
        ratios={'pendulum_over_synthetic': ('pendulum', 'synthetic'),
                'pendulum_normalized_over_pendulum':
                    ('pendulum_normalized', 'pendulum'),
                'launch_pendulum_over_synthetic':
                    ('pendulum_launch', 'synthetic_launch'),
                'launch_pendulum_normalized_over_pendulum':
                    ('pendulum_normalized_launch', 'pendulum_launch')}),
    'double_pendulum': dict(
        T=200, reps=15, policy='GaussianMLPPolicy',
        rows={'double_pendulum': _batch('DoublePendulumVecEnv'),
              'synthetic': _synthetic(11, 1),
              'pendulum': _batch('PendulumVecEnv'),
              'double_pendulum_normalized': _batch('DoublePendulumVecEnv',
                                                   normalized=True)},
        launch=('double_pendulum', 'synthetic'),
        ratios={'double_pendulum_over_synthetic':
                    ('double_pendulum', 'synthetic'),
                'double_pendulum_normalized_over_double_pendulum':
                    ('double_pendulum_normalized', 'double_pendulum'),
                'double_pendulum_over_pendulum':
                    ('double_pendulum', 'pendulum'),
                'launch_double_pendulum_over_synthetic':
                    ('double_pendulum_launch', 'synthetic_launch')}),
    'acrobot': _discrete_task('acrobot', 'AcrobotVecEnv', 'synthetic_6', 6),
    'mountain_car': _discrete_task('mountain_car', 'MountainCarVecEnv',
                                   'synthetic_2', 2),
}


def make(kind, row, n, T):
    from garage_amd import envs, policies
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(0)
    env = kind['rows'][row](envs, n, T)
    pol = getattr(policies, kind['policy'])(env.spec, hidden_sizes=(64, 64))
    return GpuVecSampler(pol, env, max_episode_length=T, n_workers=1,
                         worker_class=GpuVecWorker, seed=1,
                         worker_args=dict(n_envs=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', required=True, choices=sorted(KINDS))
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--T', type=int, help='default: 128 for cartpole, else 200')
    ap.add_argument('--reps', type=int,
                    help='default: 7 for cartpole and pendulum, else 15')
    a = ap.parse_args()
    kind = KINDS[a.kind]
    n = a.envs
    T = kind['T'] if a.T is None else a.T
    reps = kind['reps'] if a.reps is None else a.reps
    samplers = {k: make(kind, k, n, T) for k in kind['rows']}
    launchers = {k + '_launch': make(kind, k, n, T) for k in kind['launch']}
    buffers = {}
    for k, s in launchers.items():
        w = s._workers[0]
        w._start()
        buffers[k] = w._alloc_buffers(n * T)
    rows = tuple(samplers) + tuple(launchers)
    rates = {k: [] for k in rows}
    steps = {k: [] for k in rows}
    for r in range(reps + 1):
        for k in rows:
            s = samplers.get(k) or launchers[k]
            w = s._workers[0]
            torch.cuda.synchronize()
            step0 = w._global_step
            t0 = time.perf_counter()
            if k in samplers:
                s.obtain_samples(r, n * T, None)
            else:
                w._ep_t.zero_()
                assert w._native_steps(buffers[k], 0, T)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:  # the first call warms up
                rates[k].append(n * (w._global_step - step0) / dt)
                steps[k].append(w._global_step - step0)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    for k in rows:
        print(json.dumps(dict(env=k, n_envs=n, T=T, hidden=[64, 64],
                              env_steps_per_s=med[k],
                              min=float(np.min(rates[k])),
                              max=float(np.max(rates[k])),
                              steps_per_call=float(np.median(steps[k])))))
    print(json.dumps({name: med[num] / med[den]
                      for name, (num, den) in kind['ratios'].items()}))


if __name__ == '__main__':
    main()
