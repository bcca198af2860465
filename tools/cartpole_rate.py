"""Env-steps per second of ``GpuVecSampler.obtain_samples`` with
``CartPoleVecEnv`` against ``SyntheticVecEnv(discrete=True)`` of the same shape
(4 observations, 2 actions), at BASELINE.json configs[1]'s size: 4096 envs,
T = 128, a ``CategoricalMLPPolicy`` with hidden (64, 64).

    python tools/cartpole_rate.py [--envs 4096] [--T 128] [--reps 7]

Rows: ``cartpole`` (max_episode_length = T; a random policy's episodes last
about 22 steps, so they end and restart inside the launch all the time),
``synthetic`` (every episode exactly T steps) and ``synthetic_ragged`` (episode
lengths uniform in 8..T: the same kind of tail of Python-driven steps after the
one launch, until the finished episodes hold the samples asked for).  The
samplers take turns within each repetition.  Prints one JSON line per row: the
median over ``reps`` calls of (env steps taken) / (wall time of obtain_samples,
ended by a device synchronise), and the ratio cartpole / synthetic.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(kind, n, T):
    from garage_amd.envs import CartPoleVecEnv, SyntheticVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(0)
    if kind == 'cartpole':
        env = CartPoleVecEnv(n, max_episode_length=T, seed=1)
    else:
        env = SyntheticVecEnv(n, 4, 2, T, seed=1, discrete=True,
                              min_len=8 if kind == 'synthetic_ragged' else None)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
    return GpuVecSampler(pol, env, max_episode_length=T, n_workers=1,
                         worker_class=GpuVecWorker, seed=1,
                         worker_args=dict(n_envs=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--T', type=int, default=128)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    n, T = a.envs, a.T
    kinds = ('cartpole', 'synthetic', 'synthetic_ragged')
    samplers = {k: make(k, n, T) for k in kinds}
    rates = {k: [] for k in kinds}
    steps = {k: [] for k in kinds}
    for r in range(a.reps + 1):
        for k in kinds:
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
    for k in kinds:
        print(json.dumps(dict(env=k, n_envs=n, T=T, hidden=[64, 64],
                              env_steps_per_s=med[k],
                              min=float(np.min(rates[k])),
                              max=float(np.max(rates[k])),
                              steps_per_call=float(np.median(steps[k])))))
    print(json.dumps(dict(cartpole_over_synthetic=med['cartpole'] /
                          med['synthetic'],
                          cartpole_over_synthetic_ragged=med['cartpole'] /
                          med['synthetic_ragged'])))


if __name__ == '__main__':
    main()
