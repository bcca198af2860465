"""Update time of a population of narrow PPO learners: shared launches against lone runs.

M in {1, 8, 64} members x 64 CartPole envs x 128 steps (8192 samples a member),
categorical MLP(64, 64) policy and MLP(64, 64) value function, 10 epochs, with the
reference's minibatch of 64 and with 32 minibatches per pass (minibatch 256).  Timed
is the UPDATE only (``_train``: every optimisation pass of both networks), on the same
batches and from the same initial state, for

  (a) ``PopulationPPO``: step k of every member in two launches;
  (b) the same M lone ``PPO`` objects one after another, in their default
      configuration (the code path a population had before ``PopulationPPO``: the
      one-launch small step for minibatches of up to 64 rows, the narrow step above);
  (c) the same with ``ga_set_small_step(0)``: the lone NARROW path at every minibatch
      size, the path each member is the bit-for-bit twin of.

``--linear-baseline``: the members' value functions are the members of one
``LinearFeatureBaselinePopulation`` (lone ``LinearFeatureBaseline`` objects in (b)
and (c)): the update is then the policies' passes around the closed-form fit, and
no value-function pass at all.

A, B and C take turns inside one process; after warm-up every repeat is timed with HIP
events around the update and the medians, their ratio and the run-to-run spread
((max - min) / median over the repeats) are printed, one JSON line per row.

    python tools/population_update_rate.py [--members 1 8 64] [--repeats 10]
                                           [--linear-baseline]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENVS, STEPS, EPOCHS = 64, 128, 10


def make_members(M, minibatch, linear=None):
    """``linear``: None -- MLP(64, 64) value functions; 'joint' -- the members of
    one LinearFeatureBaselinePopulation; 'lone' -- lone LinearFeatureBaselines."""
    from garage_amd.algos import PPO
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy,
                                     GaussianMLPValueFunction)
    env = CartPoleVecEnv(M * ENVS, max_episode_length=STEPS, seed=3)
    joint = LinearFeatureBaselinePopulation(env.spec, M) if linear == 'joint' \
        else None
    members = []
    for m in range(M):
        torch.manual_seed(100 + m)
        pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
        opt = (torch.optim.Adam, dict(lr=2.5e-4 * (1 + m % 4)))
        if linear is None:
            vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(64, 64))
            vf_opt = OptimizerWrapper(opt, vf, EPOCHS, minibatch,
                                      permutation='device', seed=1000 + m)
        else:
            vf = joint[m] if joint is not None else LinearFeatureBaseline(
                env.spec)
            vf_opt = None
        members.append(PPO(
            env_spec=env.spec, policy=pol, value_function=vf, sampler=None,
            policy_optimizer=OptimizerWrapper(opt, pol, EPOCHS, minibatch,
                                              permutation='device', seed=m),
            vf_optimizer=vf_opt))
    return env, members


def timed(fn):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def measure(M, minibatch, repeats, warmup, linear=False):
    from garage_amd import _lib
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    lib = _lib.load()
    env, members = make_members(M, minibatch, 'joint' if linear else None)
    _, lones = make_members(M, minibatch, 'lone' if linear else None)
    _, narrows = make_members(M, minibatch, 'lone' if linear else None)
    pop = PopulationPPO(members)
    sampler = GpuPopulationSampler(members[0].policy, env, n_members=M,
                                   max_episode_length=STEPS, seed=5)
    batches = sampler.obtain_samples(0, ENVS * STEPS, pop.member_params)
    joint = pop._before_trains(batches)
    lone = [a._before_train(b) for a, b in zip(lones, batches)]
    narrow = [a._before_train(b) for a, b in zip(narrows, batches)]

    def run_a():
        pop._train(joint)

    def run_b():
        for a, c in zip(lones, lone):
            a._train(c.batch, c.adv, c.returns, c.old_ll)

    def run_c():
        lib.ga_set_small_step(0)
        try:
            for a, c in zip(narrows, narrow):
                a._train(c.batch, c.adv, c.returns, c.old_ll)
        finally:
            lib.ga_set_small_step(1)

    for _ in range(warmup):
        run_a()
        run_b()
        run_c()
    ta, tb, tc = [], [], []
    for _ in range(repeats):  # A, B and C take turns
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        tc.append(timed(run_c))
    ta, tb, tc = np.asarray(ta), np.asarray(tb), np.asarray(tc)

    def spread(t):
        return float((t.max() - t.min()) / np.median(t))

    return dict(
        members=M, minibatch=minibatch, linear_baseline=bool(linear),
        samples_per_member=[int(c.S) for c in joint][:4],
        population_ms=float(np.median(ta)), lone_ms=float(np.median(tb)),
        lone_narrow_ms=float(np.median(tc)),
        lone_over_population=float(np.median(tb) / np.median(ta)),
        lone_narrow_over_population=float(np.median(tc) / np.median(ta)),
        population_spread=spread(ta), lone_spread=spread(tb),
        lone_narrow_spread=spread(tc),
        repeats=repeats)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--members', type=int, nargs='+', default=[1, 8, 64])
    ap.add_argument('--minibatches', type=int, nargs='+', default=[64, 256],
                    help='minibatch sizes (64: the reference\'s default; 256: 32 '
                         'minibatches per pass of 8192 samples)')
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--linear-baseline', action='store_true',
                    help='LinearFeatureBaseline value functions: one '
                         'LinearFeatureBaselinePopulation in (a), lone ones in '
                         '(b) and (c)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('population_update_rate needs an MI355X: there is nothing '
                         'to measure on a CPU')
    if args.repeats < 10:
        raise SystemExit('medians of at least 10 repeats')
    for minibatch in args.minibatches:
        for M in args.members:
            print(json.dumps(measure(M, minibatch, args.repeats, args.warmup,
                                     args.linear_baseline)),
                  flush=True)


if __name__ == '__main__':
    main()
