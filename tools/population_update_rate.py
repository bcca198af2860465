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

``--obs-dim D``: the members act in a ``SyntheticVecEnv`` of ``D``-wide observations
(two discrete actions, episodes of 128 steps) instead of CartPole.  Above 32 inputs the
small step does not apply and (c) becomes the path such a learner took before the
narrow step's wide instantiations existed: ``_lib.NARROW_WIDE = False``, the per-layer
launches (reported as ``lone_per_layer_ms``), so that (b) against (c) is the lone
default against its predecessor and (a) against (c) the population against lone updates
without the wide step.

``--hidden-nonlinearity NAME`` (relu, elu, leaky_relu, sigmoid, softplus, none): the
members' networks use it instead of tanh.  (a) and (b) then run under
``garage_amd.engine.set_narrow_activations(True)`` -- the narrow step's generic-activation
instantiations -- and (c) is the lone update with the flag off: the per-layer launches,
what such a learner takes by default (reported as ``lone_per_layer_ms``).

A, B and C take turns inside one process; after warm-up every repeat is timed with HIP
events around the update and the medians, their ratio and the run-to-run spread
((max - min) / median over the repeats) are printed, one JSON line per row.

    python tools/population_update_rate.py [--members 1 8 64] [--repeats 10]
                                           [--linear-baseline] [--obs-dim D]
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


def make_members(M, minibatch, linear=None, obs_dim=None, solver='host',
                 hidden='tanh'):
    """``obs_dim``: None -- CartPole; D -- synthetic D-wide observations.
    ``linear``: None -- MLP(64, 64) value functions; 'joint' -- the members of
    one LinearFeatureBaselinePopulation; 'lone' -- lone LinearFeatureBaselines."""
    from garage_amd.algos import PPO
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    from garage_amd.envs import CartPoleVecEnv, SyntheticVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy,
                                     GaussianMLPValueFunction)
    if obs_dim is None:
        env = CartPoleVecEnv(M * ENVS, max_episode_length=STEPS, seed=3)
    else:
        env = SyntheticVecEnv(M * ENVS, obs_dim, 2, STEPS, discrete=True, seed=3)
    joint = LinearFeatureBaselinePopulation(env.spec, M, solver=solver) \
        if linear == 'joint' else None
    members = []
    net_kw = dict(hidden_sizes=(64, 64),
                  hidden_nonlinearity=None if hidden == 'none' else hidden)
    for m in range(M):
        torch.manual_seed(100 + m)
        pol = CategoricalMLPPolicy(env.spec, **net_kw)
        opt = (torch.optim.Adam, dict(lr=2.5e-4 * (1 + m % 4)))
        if linear is None:
            vf = GaussianMLPValueFunction(env.spec, **net_kw)
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


def measure(M, minibatch, repeats, warmup, linear=False, obs_dim=None, hidden=None):
    from garage_amd import _lib, engine
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    lib = _lib.load()
    fn = hidden or 'tanh'
    env, members = make_members(M, minibatch, 'joint' if linear else None, obs_dim,
                                hidden=fn)
    _, lones = make_members(M, minibatch, 'lone' if linear else None, obs_dim, hidden=fn)
    _, narrows = make_members(M, minibatch, 'lone' if linear else None, obs_dim,
                              hidden=fn)
    if hidden is not None:
        engine.set_narrow_activations(True)
    # (c): the lone narrow path up to 32 inputs, the per-layer path above (and for
    # another nonlinearity than tanh)
    wide = obs_dim is not None and obs_dim > 32
    def switch_c(on):
        if hidden is not None:
            engine.set_narrow_activations(bool(on))
        elif wide:
            _lib.NARROW_WIDE = bool(on)
        else:
            lib.ga_set_small_step(on)
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
        switch_c(0)
        try:
            for a, c in zip(narrows, narrow):
                a._train(c.batch, c.adv, c.returns, c.old_ll)
        finally:
            switch_c(1)

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

    c_name = 'lone_per_layer' if wide or hidden is not None else 'lone_narrow'
    row = dict(
        members=M, minibatch=minibatch, linear_baseline=bool(linear),
        samples_per_member=[int(c.S) for c in joint][:4],
        population_ms=float(np.median(ta)), lone_ms=float(np.median(tb)),
        lone_over_population=float(np.median(tb) / np.median(ta)),
        population_spread=spread(ta), lone_spread=spread(tb),
        repeats=repeats)
    row[c_name + '_ms'] = float(np.median(tc))
    row[c_name + '_over_population'] = float(np.median(tc) / np.median(ta))
    row[c_name + '_spread'] = spread(tc)
    for name, t in (('population', ta), ('lone', tb), (c_name, tc)):
        row[name + '_min_max_ms'] = [float(t.min()), float(t.max())]
    if hidden is not None:
        row['hidden_nonlinearity'] = hidden
        engine.set_narrow_activations(False)
    if obs_dim is not None:
        row['obs_dim'] = obs_dim
        row[c_name + '_over_lone'] = float(np.median(tc) / np.median(tb))
    return row


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
    ap.add_argument('--obs-dim', type=int, default=None,
                    help='synthetic observations of this width instead of CartPole; '
                         'above 32, (c) is the per-layer path (_lib.NARROW_WIDE off)')
    ap.add_argument('--hidden-nonlinearity', default=None,
                    choices=['relu', 'elu', 'leaky_relu', 'sigmoid', 'softplus', 'none'],
                    help='the networks\' hidden nonlinearity instead of tanh: (a) and '
                         '(b) under set_narrow_activations(True), (c) the per-layer '
                         'path with the flag off')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('population_update_rate needs an MI355X: there is nothing '
                         'to measure on a CPU')
    if args.repeats < 10:
        raise SystemExit('medians of at least 10 repeats')
    for minibatch in args.minibatches:
        for M in args.members:
            print(json.dumps(measure(M, minibatch, args.repeats, args.warmup,
                                     args.linear_baseline, args.obs_dim,
                                     args.hidden_nonlinearity)),
                  flush=True)


if __name__ == '__main__':
    main()
