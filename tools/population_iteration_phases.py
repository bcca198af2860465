"""Where one ``PopulationPPO.train`` iteration spends its time.

``population_update_rate.py``'s configuration -- M members x 64 CartPole envs x 128
steps (8192 samples a member), categorical MLP(64, 64) policy and MLP(64, 64) value
function, 10 epochs, minibatch 256 (32 minibatches per pass) -- run as ``train`` runs
it, with a device synchronise before and after each of the five phases:

  rollout        the launches and progress checks of ``obtain_samples``
  packing        the joint pack (``--per-member-pack``: one ``_pack`` per member)
  before_train   every member's ``_before_train``, one after another
  update         ``PopulationPPO._train``: the joint passes of both networks
  after_train    every member's ``_after_train``, one after another
                 (``--joint-diagnostics``: the joint launches and one host copy
                 of ``PopulationPPO(joint_diagnostics=True)``)

``--linear-baseline``: the value functions are the members of one
``LinearFeatureBaselinePopulation``: before_train and after_train then begin with
the one predict launch for all members, and update is the joint fit around the
policies' passes.

After warm-up every repeat runs the five phases in order; printed is one JSON line
per phase with the median over the repeats, the range and the spread
((max - min) / median), then the phases' total.

    python tools/population_iteration_phases.py [--members 64] [--repeats 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

from population_update_rate import ENVS, STEPS, make_members  # noqa: E402

PHASES = ('rollout', 'packing', 'before_train', 'update', 'after_train')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--members', type=int, default=64)
    ap.add_argument('--minibatch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--per-member-pack', action='store_true',
                    help='joint_pack=False: one _pack per member')
    ap.add_argument('--linear-baseline', action='store_true',
                    help='one LinearFeatureBaselinePopulation as the value '
                         'functions')
    ap.add_argument('--joint-diagnostics', action='store_true',
                    help='PopulationPPO(joint_diagnostics=True): the members\' '
                         'diagnostics after the update in joint launches')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('population_iteration_phases needs an MI355X: there is '
                         'nothing to measure on a CPU')
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    M = args.members
    env, members = make_members(M, args.minibatch,
                                'joint' if args.linear_baseline else None)
    pop = PopulationPPO(members, joint_diagnostics=args.joint_diagnostics)
    sampler = GpuPopulationSampler(members[0].policy, env, n_members=M,
                                   max_episode_length=STEPS, seed=5,
                                   joint_pack=not args.per_member_pack)
    ms = {k: [] for k in PHASES}
    clock = dict(t=None, packing=0.0)

    def tick():
        torch.cuda.synchronize()
        now = time.perf_counter()
        out = None if clock['t'] is None else 1e3 * (now - clock['t'])
        clock['t'] = now
        return out

    # the pack is the tail of obtain_samples: timed from inside it
    w = sampler._worker
    real_joint, real_pack = sampler._pack_population, w._pack

    def timed_pack(real):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **kw)
            torch.cuda.synchronize()
            clock['packing'] += 1e3 * (time.perf_counter() - t0)
            return out
        return run

    sampler._pack_population = timed_pack(real_joint)
    w._pack = timed_pack(real_pack)
    for itr in range(args.warmup + args.repeats):
        keep = itr >= args.warmup
        clock['packing'] = 0.0
        tick()
        batches = sampler.obtain_samples(itr, ENVS * STEPS, pop.member_params)
        sampled = tick()
        ctxs = pop._before_trains(batches)
        before = tick()
        pop._train(ctxs)
        update = tick()
        pop._after_trains(itr, ctxs)
        after = tick()
        if keep:
            for k, v in zip(PHASES, (sampled - clock['packing'], clock['packing'],
                                     before, update, after)):
                ms[k].append(v)
    total = np.sum([ms[k] for k in PHASES], axis=0)
    for k, v in list(ms.items()) + [('total', total)]:
        v = np.asarray(v)
        print(json.dumps(dict(
            phase=k, members=M, minibatch=args.minibatch,
            joint_pack=not args.per_member_pack,
            linear_baseline=args.linear_baseline,
            joint_diagnostics=args.joint_diagnostics, median_ms=float(np.median(v)),
            min_ms=float(v.min()), max_ms=float(v.max()),
            spread=float((v.max() - v.min()) / np.median(v)),
            share=float(np.median(v) / np.median(total)),
            repeats=args.repeats)), flush=True)


if __name__ == '__main__':
    main()
