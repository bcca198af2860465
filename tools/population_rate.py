"""Env-steps per second of a POPULATION rollout: one
``GpuPopulationSampler.obtain_samples`` over ``members`` policies x ``g``
CartPole envs each (default 64 x 64, categorical MLP(64, 64), T = 128 steps:
``num_samples = g * T``, ``max_episode_length = T``), against

- ``sequential``: ``members`` consecutive single-policy ``rollout_samples`` calls
  on ``g`` envs each, ``set_flat_param_values`` between them -- what scoring
  the candidates one after another costs -- and
- ``single``: one single-policy rollout over all ``members * g`` envs, the
  ceiling (same launch, one parameter vector, one packing).

    python tools/population_rate.py [--members 64] [--g 64] [--T 128] [--reps 7]

The three take turns within each repetition; the first repetition warms up.
Prints one JSON line per row -- the median over ``reps`` of (env steps taken) /
(wall time, ended by a device synchronise) -- then the ratios, then where the
population call's time goes: the launches (first chunk and the rest, to their
completion), the host checks between them and the packing -- the joint pack of all
members (``ga_member_pack_index``, ``ga_member_pack_gather``, one copy to the
host), or with ``--per-member-pack`` one ``GpuVecWorker._pack`` per member -- and,
for the joint pack, the gather launch alone between two HIP events with the bytes it
moves (each packed byte read and written once, plus the index).

    python tools/population_rate.py --statistics [--reps 7]

times ``obtain_statistics`` (per-episode statistics from the raw rollout buffers,
nothing packed) beside ``obtain_samples`` on the same sampler, taking turns, with
the ``single`` ceiling: every run's milliseconds, both ranges, the env-steps/s
and where an ``obtain_statistics`` call's time goes -- the launches, the progress
checks after them (kernel, copy of three integers per member, host logic), the
final statistics (two launches) and the copy and split of the result.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=64)
    ap.add_argument('--g', type=int, default=64)
    ap.add_argument('--T', type=int, default=128)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--statistics', action='store_true',
                    help='time obtain_statistics beside obtain_samples')
    ap.add_argument('--per-member-pack', action='store_true',
                    help='joint_pack=False: one _pack per member')
    a = ap.parse_args()
    M, g, T = a.members, a.g, a.T
    n, num = M * g, g * T

    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import (GpuPopulationSampler, GpuVecSampler,
                                    GpuVecWorker)
    torch.manual_seed(0)
    env = CartPoleVecEnv(n, max_episode_length=T, seed=1)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(0)
    vectors = base + 0.1 * rng.randn(M, base.size).astype(np.float32)
    pop = GpuPopulationSampler(pol, env, n_members=M, max_episode_length=T,
                               seed=1, joint_pack=not a.per_member_pack)
    packed = pol.pack_members(vectors)

    def single_sampler(envs):
        e = CartPoleVecEnv(envs, max_episode_length=T, seed=1)
        p = CategoricalMLPPolicy(e.spec, hidden_sizes=(64, 64))
        s = GpuVecSampler(p, e, max_episode_length=T, n_workers=1,
                          worker_class=GpuVecWorker, seed=1,
                          worker_args=dict(n_envs=envs))
        return s, p

    seq, seq_pol = single_sampler(g)
    one, _ = single_sampler(n)

    def run_population(r):
        w = pop._worker
        step0 = w._global_step
        pop.obtain_samples(r, num, packed)
        return n * (w._global_step - step0)

    def run_sequential(r):
        w = seq._workers[0]
        step0 = w._global_step
        for m in range(M):
            seq_pol.set_flat_param_values(vectors[m])
            w._needs_agent_reset = True
            w.rollout_samples(num)
        return g * (w._global_step - step0)

    def run_single(r):
        w = one._workers[0]
        step0 = w._global_step
        w._needs_agent_reset = True
        w.rollout_samples(n * T)
        return n * (w._global_step - step0)

    if a.statistics:
        return statistics_mode(a, pop, packed, run_population, run_single)

    rows = dict(population=run_population, sequential=run_sequential,
                single=run_single)
    rates = {k: [] for k in rows}
    for r in range(a.reps + 1):
        for k, fn in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = fn(r)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:
                rates[k].append(steps / dt)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    for k in rows:
        print(json.dumps(dict(row=k, members=M, envs_per_member=g, T=T,
                              hidden=[64, 64], env_steps_per_s=med[k],
                              min=float(np.min(rates[k])),
                              max=float(np.max(rates[k])))))
    print(json.dumps(dict(
        population_over_sequential=med['population'] / med['sequential'],
        population_over_single=med['population'] / med['single'])))

    # where one population call spends its time (a synchronise after every
    # part, so the parts add up to more than the untimed call)
    parts = dict(first_launch=0.0, later_launches=0.0, host_checks=0.0,
                 packing=0.0)
    import garage_amd.sampler as sampler_module
    w = pop._worker
    real_steps, real_pack = pop._steps, w._pack
    real_joint, real_call = pop._pack_population, sampler_module.call
    state = dict(calls=0, last=None)
    gather = dict(events=[], bytes=0)

    def call(name, *args):
        if name != 'ga_member_pack_gather':
            return real_call(name, *args)
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        real_call(name, *args)
        stop.record()
        gather['events'].append((start, stop))
        planes, n_planes, n_rows, n_eps = args[0], args[1], args[3], args[6]
        for p in list(planes)[:n_planes]:
            rows = n_eps if p.per_episode else n_rows
            # read and written once; one index entry a row (two per episode)
            gather['bytes'] += rows * (2 * p.width * p.elem_size
                                       + (8 if p.per_episode else 4))

    def timed(key, fn, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if state['last'] is not None:
            parts['host_checks'] += t0 - state['last']
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        state['last'] = time.perf_counter()
        parts[key] += state['last'] - t0
        return out

    def steps(*args):
        state['calls'] += 1
        return timed('first_launch' if state['calls'] == 1
                     else 'later_launches', real_steps, *args)

    pop._steps = steps
    w._pack = lambda *args, **kw: timed('packing', real_pack, *args, **kw)
    pop._pack_population = lambda *args, **kw: timed('packing', real_joint,
                                                     *args, **kw)
    sampler_module.call = call
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop.obtain_samples(0, num, packed)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        pop._steps, w._pack = real_steps, real_pack
        pop._pack_population, sampler_module.call = real_joint, real_call
    print(json.dumps(dict(breakdown_ms={k: 1e3 * v for k, v in parts.items()},
                          total_ms=1e3 * total, launches=state['calls'],
                          joint_pack=not a.per_member_pack)))
    if gather['events']:
        # the launch alone, over further calls (the first one above included)
        sampler_module.call = call
        try:
            for r in range(a.reps):
                pop.obtain_samples(r, num, packed)
            torch.cuda.synchronize()
        finally:
            sampler_module.call = real_call
        ms = [s.elapsed_time(e) for s, e in gather['events']]
        per_call = gather['bytes'] / len(ms)
        print(json.dumps(dict(
            gather_launches=len(ms), gather_ms_median=float(np.median(ms)),
            gather_ms_min=min(ms), gather_ms_max=max(ms),
            gather_bytes=per_call,
            gather_GB_per_s=per_call / (1e6 * float(np.median(ms))))))


def statistics_mode(a, pop, packed, run_population, run_single):
    """``obtain_samples`` / ``obtain_statistics`` / the single-policy ceiling,
    taking turns; then the parts of one ``obtain_statistics`` call."""
    import garage_amd.sampler as sampler_module
    M, g, T = a.members, a.g, a.T
    n, num = M * g, g * T
    w = pop._worker

    def run_statistics(r):
        step0 = w._global_step
        pop.obtain_statistics(r, num, packed, 0.99)
        return n * (w._global_step - step0)

    rows = dict(obtain_samples=run_population,
                obtain_statistics=run_statistics, single=run_single)
    ms, rates = {k: [] for k in rows}, {k: [] for k in rows}
    for r in range(a.reps + 1):
        for k, fn in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = fn(r)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r:
                ms[k].append(1e3 * dt)
                rates[k].append(steps / dt)
    for k in rows:
        print(json.dumps(dict(
            row=k, members=M, envs_per_member=g, T=T, hidden=[64, 64],
            runs_ms=[round(x, 3) for x in ms[k]], min_ms=min(ms[k]),
            max_ms=max(ms[k]), env_steps_per_s=float(np.median(rates[k])))))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps(dict(
        every_statistics_run_faster_than_every_samples_run=bool(
            max(ms['obtain_statistics']) < min(ms['obtain_samples'])),
        statistics_over_samples=med['obtain_statistics'] /
        med['obtain_samples'],
        statistics_over_single=med['obtain_statistics'] / med['single'])))

    # where one obtain_statistics call spends its time (a synchronise after
    # every part, so the parts add up to more than the untimed call)
    parts = dict(launches=0.0, progress_checks=0.0, final_statistics=0.0,
                 copy_and_split=0.0)
    real_steps, real_call = pop._steps, sampler_module.call
    state = dict(launches=0, checks=0, last=None)

    def close_check(now):
        if state['last'] is not None:
            parts['progress_checks'] += now - state['last']
            state['last'] = None

    def steps(*args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        close_check(t0)
        real_steps(*args)
        torch.cuda.synchronize()
        state['last'] = time.perf_counter()
        state['launches'] += 1
        parts['launches'] += state['last'] - t0

    def call(name, *args):
        if name == 'ga_member_progress':
            state['checks'] += 1
        if name != 'ga_member_episode_statistics':
            return real_call(name, *args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        close_check(t0)
        real_call(name, *args)
        torch.cuda.synchronize()
        state['end'] = time.perf_counter()
        parts['final_statistics'] += state['end'] - t0

    pop._steps, sampler_module.call = steps, call
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pop.obtain_statistics(0, num, packed, 0.99)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    finally:
        pop._steps, sampler_module.call = real_steps, real_call
    parts['copy_and_split'] = t1 - state['end']
    print(json.dumps(dict(breakdown_ms={k: 1e3 * v for k, v in parts.items()},
                          total_ms=1e3 * (t1 - t0),
                          launches=state['launches'],
                          progress_checks=state['checks'])))


if __name__ == '__main__':
    main()
