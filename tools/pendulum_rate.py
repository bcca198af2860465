"""Env-steps per second of ``GpuVecSampler.obtain_samples`` with
``PendulumVecEnv`` against ``SyntheticVecEnv`` of the same shape (3
observations, 1 continuous action, unbounded) and against
``NormalizedVecEnv(PendulumVecEnv)``: 4096 envs, T = 200 (Pendulum-v0's
TimeLimit), a ``GaussianMLPPolicy`` with hidden (64, 64).

    python tools/pendulum_rate.py [--envs 4096] [--T 200] [--reps 7]

Rows: ``pendulum`` (max_episode_length = T: every episode is exactly T steps,
so a call is one launch), ``synthetic`` (the same, with a Philox draw for an
env step: ``pendulum / synthetic`` is what the dynamics cost inside the launch)
and ``pendulum_normalized`` (``normalize`` rescales the policy's action to the
torque bounds in a launch of its own, so the rollout takes three launches per
step: ``pendulum_normalized / pendulum`` is what that path costs).  The
samplers take turns within each repetition.  Prints one JSON line per row: the
median, min and max over ``reps`` calls of (env steps taken) / (wall time of
obtain_samples, ended by a device synchronise), and the two ratios.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ('pendulum', 'synthetic', 'pendulum_normalized')


def make(kind, n, T):
    from garage_amd.envs import (NormalizedVecEnv, PendulumVecEnv,
                                 SyntheticVecEnv)
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(0)
    if kind == 'synthetic':
        env = SyntheticVecEnv(n, 3, 1, T, seed=1)
    else:
        env = PendulumVecEnv(n, max_episode_length=T, seed=1)
        if kind == 'pendulum_normalized':
            env = NormalizedVecEnv(env)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(64, 64))
    return GpuVecSampler(pol, env, max_episode_length=T, n_workers=1,
                         worker_class=GpuVecWorker, seed=1,
                         worker_args=dict(n_envs=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--T', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    n, T = a.envs, a.T
    samplers = {k: make(k, n, T) for k in KINDS}
    rates = {k: [] for k in KINDS}
    steps = {k: [] for k in KINDS}
    for r in range(a.reps + 1):
        for k in KINDS:
            s = samplers[k]
            w = s._workers[0]
            torch.cuda.synchronize()
            step0 = w._global_step
            t0 = time.perf_counter()
            s.obtain_samples(r, n * T, None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:  # the first call warms up
                rates[k].append(n * (w._global_step - step0) / dt)
                steps[k].append(w._global_step - step0)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    for k in KINDS:
        print(json.dumps(dict(env=k, n_envs=n, T=T, hidden=[64, 64],
                              env_steps_per_s=med[k],
                              min=float(np.min(rates[k])),
                              max=float(np.max(rates[k])),
                              steps_per_call=float(np.median(steps[k])))))
    print(json.dumps(dict(
        pendulum_over_synthetic=med['pendulum'] / med['synthetic'],
        pendulum_normalized_over_pendulum=(med['pendulum_normalized'] /
                                           med['pendulum']))))


if __name__ == '__main__':
    main()
