"""Env-steps per second of the one-launch rollout (ga_rollout_env_steps)
with PointVecEnv against SyntheticVecEnv of the same
observation / action sizes, and with MultiTaskPointVecEnv (K = 4 and K = 16 goals
on the unit circle, round robin, add-onehot: observations 3 + K wide;
never_done, so that every episode runs its T steps as the other rows' do and the
rows differ by the work per step alone): 4096 envs x T 256, a (256, 256)
Gaussian MLP policy.  ``--options`` adds PointVecEnv behind a relu, an elu and a
LayerNorm + tanh policy of the same sizes (rows ``point_relu``, ``point_elu``,
``point_ln_tanh``): the one-launch rollout with the network options.  ``--wide`` adds
SyntheticVecEnv behind networks wider than 256 (the step kernel at WIDTH = 512; with
``GARAGE_AMD_ROLLOUT_WIDE=0`` in the environment the same rows take the per-layer path):
``synthetic_c5`` -- obs 376, act 17, (512, 512, 512), ragged episodes of 32..T steps,
8192 envs unless ``--envs`` says otherwise -- and ``synthetic_320`` -- obs 17, act 6,
(320, 320).

    python tools/device_env_rate.py [--envs 4096] [--T 256] [--reps 5] [--options]
                                    [--wide] [--lib path/to/libgarage_amd.so]
                                    [--digest]

``--lib`` loads another build of the library (A/B runs against an earlier commit's).
``--digest`` times nothing: per row, a sha256 over the first rollout's observations,
actions, rewards and lengths (same seeds every run; meant for small sizes, e.g.
``--envs 64 --T 16``), to compare two builds bit for bit.

Prints one JSON line per env: the median over `reps` rollouts of
(env steps taken) / (wall time of rollout_samples incl. packing).
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(kind, n, T, reps, digest=False):
    from garage_amd.envs import (MultiTaskPointVecEnv, PointVecEnv,
                                 SyntheticVecEnv, round_robin_strategy)
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(0)
    options = {}
    hidden = (256, 256)
    if kind in POLICY_OPTIONS:
        options = POLICY_OPTIONS[kind]()
    if kind == 'point' or options:
        env = PointVecEnv(n, goal=(1., 1.), max_episode_length=T)
    elif kind.startswith('multitask'):
        K = int(kind.split('_k')[1])
        angle = 2 * np.pi * np.arange(K) / K
        env = MultiTaskPointVecEnv(
            n, np.stack([np.cos(angle), np.sin(angle)], axis=1),
            round_robin_strategy, 'add-onehot', start='spread',
            never_done=True, max_episode_length=T)
    elif kind in WIDE_ROWS:
        O, A, hidden, min_len = WIDE_ROWS[kind]
        env = SyntheticVecEnv(n, O, A, T, min_len=min_len and min(min_len, T),
                              seed=1)
    else:
        env = SyntheticVecEnv(n, 3, 2, T, seed=1)
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.1,
                            **options)
    s = GpuVecSampler(pol, env, max_episode_length=T, n_workers=1,
                      worker_class=GpuVecWorker, seed=1,
                      worker_args=dict(n_envs=n))
    w = s._workers[0]
    if digest:
        s._update_workers(None, None)
        eps = w.rollout_samples(n * T).to_host()
        h = hashlib.sha256()
        for x in (eps.observations, eps.actions, eps.rewards, eps.lengths):
            h.update(np.ascontiguousarray(x).tobytes())
        return dict(env=kind, n_envs=n, T=T, hidden=list(hidden),
                    samples=int(np.sum(eps.lengths)), sha256=h.hexdigest())
    rates = []
    for r in range(reps + 1):
        s._update_workers(None, None)
        torch.cuda.synchronize()
        step0 = w._global_step
        t0 = time.perf_counter()
        w.rollout_samples(n * T)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r:  # the first rollout warms up
            rates.append(n * (w._global_step - step0) / dt)
    return dict(env=kind, n_envs=n, T=T, hidden=list(hidden),
                env_steps_per_s=float(np.median(rates)),
                min=float(np.min(rates)), max=float(np.max(rates)))


def _relu():
    return dict(hidden_nonlinearity=torch.relu)


def _elu():
    return dict(hidden_nonlinearity=torch.nn.functional.elu)


def _ln_tanh():
    return dict(layer_normalization=True)


POLICY_OPTIONS = {'point_relu': _relu, 'point_elu': _elu,
                  'point_ln_tanh': _ln_tanh}


# obs, act, hidden, min_len
WIDE_ROWS = {'synthetic_c5': (376, 17, (512, 512, 512), 32),
             'synthetic_320': (17, 6, (320, 320), None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=None,
                    help='default 4096 (synthetic_c5: 8192)')
    ap.add_argument('--T', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--options', action='store_true',
                    help='also the point_relu / point_elu / point_ln_tanh rows')
    ap.add_argument('--wide', action='store_true',
                    help='also the synthetic_c5 / synthetic_320 rows')
    ap.add_argument('--lib', help='load this build of libgarage_amd.so')
    ap.add_argument('--digest', action='store_true',
                    help='sha256 of the first rollout per row instead of a rate')
    a = ap.parse_args()
    if a.lib:
        from garage_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    kinds = ('point', 'synthetic', 'multitask_k4', 'multitask_k16')
    if a.options:
        kinds += tuple(POLICY_OPTIONS)
    if a.wide:
        kinds += tuple(WIDE_ROWS)
    for kind in kinds:
        n = a.envs or (8192 if kind == 'synthetic_c5' else 4096)
        print(json.dumps(measure(kind, n, a.T, a.reps, a.digest)), flush=True)


if __name__ == '__main__':
    main()
