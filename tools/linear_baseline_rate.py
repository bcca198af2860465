"""Rates of the linear feature baseline's kernels, and what the closed-form fit
replaces.

Two shapes: the C3 batch (S = 4096 x 256 samples, obs_dim 17, F = 38 features)
and the widest the kernels take (S = 2^18, obs_dim 128, F = 260).  Timed with HIP
events, after warm-up, ``--repeats`` times each, taking turns inside one process:

  gram      ``ga_linear_features_gram_f64`` (both launches)
  predict   ``ga_linear_features_predict_f32``
  fit       ``LinearFeatureBaseline.fit_batch``: Gram pass, copy to pinned host
            memory, numpy's lstsq on the host, upload (host clock around it, the
            device idle before and after)
  torch     ``Phi.T @ Phi`` in fp64 on PRE-BUILT features of the same shape (the
            features' own 8 * S * F bytes are read; building them is not timed)
  vf_mlp    at C3 only: the value function's optimisation passes as they stand
            without this baseline -- GaussianMLPValueFunction MLP(256, 256),
            10 epochs x 32 minibatches of Adam on the current stream

``--members M``: instead of the above, a population of M baselines at the
population tools' member batch (64 episodes x 128 steps = 8192 samples, obs_dim 4,
F = 12), host clock around each, the device idle before and after, taking turns:

  joint     ``LinearFeatureBaselinePopulation``: ``begin_fit`` / ``finish_fit`` /
            ``predict_batches`` -- one Gram launch, one reduce launch, one copy,
            one wait, one predict launch for all members
  lone      M ``LinearFeatureBaseline`` objects one after another, each
            ``begin_fit`` / ``finish_fit`` / ``predict_batch``
  (and the fit and the predict halves of each on their own)

Printed per row, one JSON line: the median, the run-to-run spread
((max - min) / median), and for the two kernels the share of the fp64 matrix
peak (algorithmic flops S * F * (F + 1) over 78.6 TF) and of the HBM bandwidth
(algorithmic bytes 4 * S * (obs_dim + 1) over 8.0 TB/s spec).

    python tools/linear_baseline_rate.py [--repeats 10] [--warmup 3] [--members M]
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

FP64_MATRIX_PEAK = 78.6e12  # flop/s, MI355X spec
HBM_PEAK = 8.0e12           # byte/s, MI355X spec
SHAPES = [('c3', 4096, 256, 17), ('wide', 1024, 256, 128)]


def make_batch(n_eps, T, obs_dim, seed=0):
    from garage_amd._dtypes import Box, DeviceEpisodeBatch, EnvSpec
    dev = torch.device('cuda:0')
    S = n_eps * T
    gen = torch.Generator(device=dev).manual_seed(seed)
    ldo = (obs_dim + 3) // 4 * 4
    obs = torch.zeros(S, ldo, device=dev)
    obs[:, :obs_dim] = torch.rand(S, obs_dim, device=dev, generator=gen) * 6 - 3
    returns = 30 * torch.randn(S, device=dev, generator=gen)
    spec = EnvSpec(Box(-np.inf, np.inf, (obs_dim, )), Box(-np.inf, np.inf, (6, )),
                   max_episode_length=T)
    batch = DeviceEpisodeBatch(
        spec, lengths=np.full(n_eps, T), obs_dev=obs,
        last_obs_dev=torch.zeros(n_eps, ldo, device=dev),
        actions_dev=torch.zeros(S, 8, device=dev),
        rewards_dev=torch.zeros(S, device=dev),
        step_types_dev=torch.zeros(S, dtype=torch.uint8, device=dev),
        ep_off_dev=torch.arange(0, S + 1, T, dtype=torch.int64, device=dev))
    return spec, batch, returns


def event_ms(fn):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def features_fp64(batch, obs_dim, T):
    x = batch.obs_dev[:, :obs_dim].double().clamp(-10, 10)
    al = (torch.arange(batch.n_samples, device=x.device) % T).double().view(
        -1, 1) / 100.0
    return torch.cat([x, x * x, al, al * al, al * al * al,
                      torch.ones_like(al)], dim=1).contiguous()


def vf_mlp_pass(spec, batch, returns):
    """The MLP value function's passes at this batch: a callable."""
    from garage_amd.algos import PPO
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    torch.manual_seed(1)
    pol = GaussianMLPPolicy(spec, hidden_sizes=(256, 256))
    vf = GaussianMLPValueFunction(spec, hidden_sizes=(256, 256))
    opt = (torch.optim.Adam, dict(lr=2.5e-4))
    mb = batch.n_samples // 32
    algo = PPO(env_spec=spec, policy=pol, value_function=vf, sampler=None,
               policy_optimizer=OptimizerWrapper(opt, pol, 10, mb,
                                                 permutation='device', seed=2),
               vf_optimizer=OptimizerWrapper(opt, vf, 10, mb,
                                             permutation='device', seed=3))
    return lambda: algo._native_pass(algo._vf_optimizer, vf, 1, batch, None,
                                     returns, None)


def members_rows(M, repeats, warmup):
    """The joint fit + predict of M members against M lone ones."""
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    n_eps, T, obs_dim = 64, 128, 4
    made = [make_batch(n_eps, T, obs_dim, seed=m) for m in range(M)]
    spec = made[0][0]
    batches, returns = [b for _, b, _ in made], [r for _, _, r in made]
    pop = LinearFeatureBaselinePopulation(spec, M)
    lones = [LinearFeatureBaseline(spec) for _ in range(M)]

    def joint_fit():
        pop.begin_fit(batches, returns)
        pop.finish_fit()

    def lone_fit():
        for b, batch, ret in zip(lones, batches, returns):
            b.begin_fit(batch, ret)
            b.finish_fit()

    def lone_predict():
        return [b.predict_batch(batch) for b, batch in zip(lones, batches)]

    rows = [('joint fit', joint_fit), ('lone fit', lone_fit),
            ('joint predict', lambda: pop.predict_batches(batches)),
            ('lone predict', lone_predict),
            ('joint fit+predict', lambda: (joint_fit(),
                                           pop.predict_batches(batches))),
            ('lone fit+predict', lambda: (lone_fit(), lone_predict()))]
    times = {name: [] for name, _ in rows}
    for rep in range(warmup + repeats):
        for name, fn in rows:
            ms = host_ms(fn)
            if rep >= warmup:
                times[name].append(ms)
    for m in range(M):  # the two sides computed the same
        assert np.array_equal(pop[m].get_param_values(),
                              lones[m].get_param_values()), m
    for name, _ in rows:
        t = np.asarray(times[name])
        med = float(np.median(t))
        print(json.dumps(dict(
            members=M, S=n_eps * T, obs_dim=obs_dim, F=2 * obs_dim + 4,
            what=name, median_ms=round(med, 4), min_ms=round(float(t.min()), 4),
            max_ms=round(float(t.max()), 4),
            spread=round(float((t.max() - t.min()) / med), 3),
            repeats=len(t))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--members', type=int, default=0,
                    help='a population of this many baselines against as many '
                         'lone ones, instead of the kernels\' rates')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('linear_baseline_rate: needs an MI355X')
    if args.members:
        members_rows(args.members, args.repeats, args.warmup)
        return
    from garage_amd import _lib
    from garage_amd.baselines import LinearFeatureBaseline
    for tag, n_eps, T, obs_dim in SHAPES:
        spec, batch, returns = make_batch(n_eps, T, obs_dim)
        S, F = batch.n_samples, 2 * obs_dim + 4
        base = LinearFeatureBaseline(spec)
        base.fit_batch(batch, returns)
        out, _ = base._buffers(batch.obs_dev.device, S)
        ws = base._workspace

        def gram():
            _lib.call('ga_linear_features_gram_f64', _lib.dptr(batch.obs_dev),
                      batch.obs_dev.stride(0), obs_dim,
                      _lib.dptr(batch.ep_off_dev), n_eps, S, _lib.dptr(returns),
                      _lib.dptr(out), out[F * F:].data_ptr(), _lib.dptr(ws),
                      _lib.stream_ptr())

        phi = features_fp64(batch, obs_dim, T)
        rows = [('gram', event_ms, gram),
                ('predict', event_ms, lambda: base.predict_batch(batch)),
                ('fit', host_ms, lambda: base.fit_batch(batch, returns)),
                ('fit+predict', host_ms, lambda: (
                    base.fit_batch(batch, returns), base.predict_batch(batch))),
                ('torch', event_ms, lambda: phi.t() @ phi)]
        if tag == 'c3':
            rows.append(('vf_mlp', event_ms, vf_mlp_pass(spec, batch, returns)))
        times = {name: [] for name, _, _ in rows}
        for rep in range(args.warmup + args.repeats):
            for name, clock, fn in rows:
                ms = clock(fn)
                if rep >= args.warmup:
                    times[name].append(ms)
        flops, nbytes = S * F * (F + 1), 4 * S * (obs_dim + 1)
        for name, _, _ in rows:
            t = np.asarray(times[name])
            med = float(np.median(t))
            row = dict(shape=tag, S=S, obs_dim=obs_dim, F=F, what=name,
                       median_ms=round(med, 4),
                       spread=round(float((t.max() - t.min()) / med), 3),
                       repeats=len(t))
            if name == 'gram':
                row['fp64_matrix_peak_share'] = round(
                    flops / (med * 1e-3) / FP64_MATRIX_PEAK, 4)
                row['hbm_share'] = round(nbytes / (med * 1e-3) / HBM_PEAK, 4)
            if name == 'predict':
                row['hbm_share'] = round(
                    4 * S * (obs_dim + 1) / (med * 1e-3) / HBM_PEAK, 4)
            print(json.dumps(row), flush=True)
        del phi


if __name__ == '__main__':
    main()
