"""Policy-step time of a population of narrow TRPO learners: joint launches against lone
runs.

M in {1, 64} members x 64 envs x 128 steps (8192 samples a member), MLP(64, 64)
policies: categorical on CartPole and Gaussian on Pendulum.  Timed is the POLICY STEP
only -- gradient, 10 conjugate-gradient iterations, step length and the backtracking
line search -- on the same batches and from the same parameters (restored before every
repeat), for

  (a) ``PopulationTRPO._natural_step``: every member's solve in 2 (cg_iters + 1) + 2
      launches, two launches and one host copy per backtrack round;
  (b) the same M lone ``TRPO`` objects' ``_train_policy`` one after another (the code
      path a population had before ``PopulationTRPO``).

A and B take turns inside one process; after warm-up every repeat is timed by the host
clock around work that ends in a device synchronise (both paths wait for the host
inside), and the medians, their ratio and the run-to-run spread ((max - min) / median)
are printed, one JSON line per row, with the launches of one joint step as the
library's counter gives them.

``--obs-dim N`` puts both heads on a ``SyntheticVecEnv`` of N-wide observations (4
actions) instead: the wide kernel of the joint step above 32 inputs.

    python tools/population_trpo_rate.py [--members 1 64] [--repeats 10] [--obs-dim 39]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENVS, STEPS = 64, 128
GA_PROF_MEMBERS_STEP = 15


def make_members(M, head, obs_dim=None):
    from garage_amd.algos import TRPO
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    from garage_amd.envs import CartPoleVecEnv, PendulumVecEnv, SyntheticVecEnv
    from garage_amd.optimizers import (ConjugateGradientOptimizer,
                                       OptimizerWrapper)
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    if obs_dim:
        env = SyntheticVecEnv(M * ENVS, obs_dim, 4, STEPS, seed=3,
                              discrete=head == 'categorical')
    elif head == 'categorical':
        env = CartPoleVecEnv(M * ENVS, max_episode_length=STEPS, seed=3)
    else:
        env = PendulumVecEnv(M * ENVS, max_episode_length=STEPS, seed=3)
    # (the policy step is what is timed: the baselines only feed the advantages)
    vfs = LinearFeatureBaselinePopulation(env.spec, M)
    members = []
    for m in range(M):
        torch.manual_seed(100 + m)
        cls = CategoricalMLPPolicy if head == 'categorical' else GaussianMLPPolicy
        pol = cls(env.spec, hidden_sizes=(64, 64))
        members.append(TRPO(
            env_spec=env.spec, policy=pol, value_function=vfs[m], sampler=None,
            policy_optimizer=OptimizerWrapper(
                (ConjugateGradientOptimizer, dict(max_constraint_value=0.01)), pol)))
    return env, members


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def measure(M, head, repeats, warmup, obs_dim=None):
    from garage_amd import _lib
    from garage_amd.algos import PopulationTRPO
    from garage_amd.sampler import GpuPopulationSampler
    lib = _lib.load()
    env, members = make_members(M, head, obs_dim)
    _, lones = make_members(M, head, obs_dim)
    pop = PopulationTRPO(members)
    sampler = GpuPopulationSampler(members[0].policy, env, n_members=M,
                                   max_episode_length=STEPS, seed=5)
    batches = sampler.obtain_samples(0, ENVS * STEPS, pop.member_params)
    joint = pop._before_trains(batches)
    start = pop.member_params.clone()
    for a, m in zip(lones, range(M)):
        a.policy.net.params.copy_(start[m])
    lone = [a._before_train(b, c.values) for a, b, c in zip(lones, batches, joint)]

    @_lib.narrow_wide_scope  # (as PopulationTRPO._train runs it)
    def run_a():
        pop.member_params.copy_(start)
        pop._natural_step(joint)

    def run_b():
        for m, (a, c) in enumerate(zip(lones, lone)):
            a.policy.net.params.copy_(start[m])
            a._train_policy(c.batch, c.adv, c.old_ll, None)

    for _ in range(warmup):
        run_a()
        run_b()
    before = int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP))
    run_a()
    launches = int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP)) - before
    ta, tb = [], []
    for _ in range(repeats):  # A and B take turns
        ta.append(timed(run_a))
        tb.append(timed(run_b))
    ta, tb = np.asarray(ta), np.asarray(tb)

    def spread(t):
        return float((t.max() - t.min()) / np.median(t))

    return dict(members=M, head=head, obs_dim=int(env.spec.observation_space.flat_dim),
                samples_per_member=[int(c.S) for c in joint][:4],
                population_ms=float(np.median(ta)), lone_ms=float(np.median(tb)),
                lone_over_population=float(np.median(tb) / np.median(ta)),
                population_spread=spread(ta), lone_spread=spread(tb),
                population_launches=launches,
                accepted=[a.last_cg['accepted'] for a in pop.members][:8],
                lone_accepted=[a.last_cg['accepted'] for a in lones][:8],
                repeats=repeats)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--members', type=int, nargs='+', default=[1, 64])
    ap.add_argument('--heads', nargs='+', default=['categorical', 'gaussian'])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--obs-dim', type=int, default=None,
                    help='observation width of a SyntheticVecEnv in the place of '
                         'CartPole / Pendulum')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('population_trpo_rate needs an MI355X: there is nothing to '
                         'measure on a CPU')
    if args.repeats < 10:
        raise SystemExit('medians of at least 10 repeats')
    for head in args.heads:
        for M in args.members:
            print(json.dumps(measure(M, head, args.repeats, args.warmup, args.obs_dim)), flush=True)


if __name__ == '__main__':
    main()
