"""The one-launch rollout step with every MLP option of ``ga_mlp_desc``
(``hidden_nonlinearity``, ``output_nonlinearity``, ``layer_normalization``):

A. the fused step against the per-layer path, both measured against an fp64
   evaluation of the policy's own parameters on the first step's observations;
B. a whole rollout in ONE launch (weights resident) bit for bit against the
   same kernel stepped one launch at a time (weights streamed);
C. the NormalizedEnv statistics inside that launch against Python-driven steps;
D. the training forward of such a network stays on the per-layer GEMMs.

Measured on an MI355X (fused error, per-layer error; the bound of A is
``max(2e-6, 2 x per-layer error)``): see DESIGN.md section 7.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_device_envs_gpu import GA_PROF_ROLLOUT, _same, _stepwise
from test_multitask_envs_gpu import GOALS4, NAMES4

pytestmark = pytest.mark.gpu

ACT64 = {'tanh': torch.tanh, 'relu': torch.relu, 'none': lambda x: x,
         'sigmoid': torch.sigmoid, 'elu': F.elu, 'leaky_relu': F.leaky_relu,
         'softplus': F.softplus}


def _fp64_head(pol, obs):
    """Means (Gaussian) / probabilities (categorical) of ``obs`` in fp64 on the
    CPU from the policy's own parameters."""
    from garage_amd.engine import round4
    net = pol.net
    x = torch.as_tensor(np.asarray(obs), dtype=torch.float64)
    nl = len(net.dims) - 1
    for l in range(nl):
        last = l == nl - 1
        D = net.dims[l]
        if net.layer_norm and not last:
            o, w = net.ln_off[l], round4(D)
            gamma = net.params[o:o + D].double().cpu()
            beta = net.params[o + w:o + w + D].double().cpu()
            x = F.layer_norm(x, (D, ), gamma, beta, 1e-5)
        x = x @ net.weight(l).double().cpu().T + net.bias(l).double().cpu()
        x = ACT64[net.output_act if last else net.hidden_act](x)
    if pol.kind == 'categorical':
        x = torch.softmax(x, dim=-1)
        if pol.double_softmax:
            x = torch.softmax(x, dim=-1)
    return x.numpy()


def _sampler(fused, discrete, O, A, hidden, n, P, noise, options):
    """``_rollout`` of test_policy_fused_gpu.py with the policy's options."""
    from garage_amd.envs import SyntheticVecEnv
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(21)
    env = SyntheticVecEnv(n, O, A, P, min_len=max(1, P // 3), seed=5,
                          discrete=discrete)
    cls = CategoricalMLPPolicy if discrete else GaussianMLPPolicy
    pol = cls(env.spec, hidden_sizes=hidden, **options)
    with torch.no_grad():  # biases away from zero, gamma / beta from (1, 0)
        pol.net.params.add_(torch.randn_like(pol.net.params) * 0.05)
        for l in range(len(hidden) + 1):
            w = pol.net.params[pol.net.w_off[l]:pol.net.b_off[l]].view(
                pol.net.dims[l + 1], -1)
            w[:, pol.net.dims[l]:] = 0
    dev = pol.device

    def noise_fn(step):
        return noise[step].to(dev)

    sampler = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                            worker_class=GpuVecWorker,
                            worker_args=dict(n_envs=n, noise_fn=noise_fn,
                                             fused_policy_step=fused))
    return sampler, pol


def _first_step(fused, *case):
    """(observations, means / probabilities, fp64 of the same) of the first
    vectorised step."""
    sampler, pol = _sampler(fused, *case)
    w = sampler._workers[0]
    w.start_episode()
    w.step_episode()
    b = w._api_buffer()
    O, A = pol.net.in_dim, pol.net.out_dim
    obs = b['obs'][:, 0, :O].cpu().numpy()
    head = b['head'][:, 0, :A].cpu().numpy()
    return obs, head, _fp64_head(pol, obs)


S1 = (False, 5, 3, (16, 16), 77)
S2 = (False, 33, 7, (40, 24, 100), 45)
S3 = (True, 9, 5, (32, ), 31)
S4 = (False, 17, 6, (256, 256), 300)
LN = dict(layer_normalization=True)

CASES = (
    [(S2, dict(hidden_nonlinearity=h)) for h in
     (torch.relu, None, torch.sigmoid, F.elu, F.leaky_relu, F.softplus)] +
    [(S1, dict(output_nonlinearity=o)) for o in (torch.tanh, torch.sigmoid)] +
    [(s, dict(hidden_nonlinearity=h, **LN)) for s in (S1, S2, S4)
     for h in (torch.tanh, torch.relu)] +
    [(S2, dict(hidden_nonlinearity=torch.relu, output_nonlinearity=torch.tanh,
               **LN)),
     (S3, dict(hidden_nonlinearity=torch.relu))])


def _case_id(case):
    shape, options = case
    name = {S1: 's1', S2: 's2', S3: 's3', S4: 's4'}[shape]
    for key, val in options.items():
        name += '-' + key.split('_')[0] + '_' + (
            getattr(val, '__name__', str(val)))
    return name


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_fused_step_matches_per_layer_path_with_options(case):
    from garage_amd import _lib
    (discrete, O, A, hidden, n), options = case
    P = 9
    torch.manual_seed(3)
    noise = torch.rand(40, n, 8) if discrete else torch.randn(40, n, 8)
    args = (discrete, O, A, hidden, n, P, noise, options)
    sa, pa = _sampler(True, *args)
    assert _lib.load().ga_policy_step_fused_supported(
        C.byref(pa.net._desc)) == 1
    sb, _ = _sampler(False, *args)
    a = sa.obtain_samples(0, n * P, None)
    b = sb.obtain_samples(0, n * P, None)
    assert np.array_equal(a.lengths, b.lengths)
    assert np.array_equal(a.observations, b.observations)
    assert np.array_equal([int(s) for s in a.step_types],
                          [int(s) for s in b.step_types])
    if discrete:
        # identical uniforms; a pick can only differ when u sits within an ulp
        # of a CDF boundary
        assert (a.actions != b.actions).mean() < 0.01
    # the first step of both paths against fp64: the per-layer path is pinned
    # to the reference; the factor 2 allows for another summation order of
    # the same fp32 terms and nothing more
    obs_f, head_f, want = _first_step(True, *args)
    obs_p, head_p, _ = _first_step(False, *args)
    assert np.array_equal(obs_f, obs_p)
    err_f = float(np.abs(head_f - want).max())
    err_p = float(np.abs(head_p - want).max())
    print('rollout options %s: fused %.3e per-layer %.3e' %
          (_case_id(case), err_f, err_p))
    assert np.isfinite(head_f).all()
    assert err_f <= max(2e-6, 2 * err_p), (err_f, err_p)


def _make(kind, hidden, options, n=48, P=20, seed=5):
    """``_make`` of test_device_envs_gpu.py / test_multitask_envs_gpu.py with
    the policy's options (unwrapped batches: unbounded actions)."""
    from garage_amd.envs import (GridWorldVecEnv, MultiTaskPointVecEnv,
                                 PointVecEnv, round_robin_strategy)
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(seed)
    if kind == 'point':
        goals = [((i % 7) * 0.05 - 0.15, (i % 5) * 0.04 - 0.1)
                 for i in range(n)]
        env = PointVecEnv(n, goal=goals[0], done_bonus=0.5,
                          max_episode_length=P)
        env.set_tasks([{'goal': x} for x in goals])
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.1,
                                **options)
    elif kind == 'multitask':
        # A freshly initialised leaky_relu + LayerNorm policy saturates the
        # +-0.1 action box in one direction and reaches no goal of GOALS4 (a
        # numpy twin of this rollout over 40 initialisations: 7 without a
        # single success).  Goals 20 % closer and an output layer scaled by
        # 0.1, so that the actions are mostly the policy's noise: 40 of 40
        # with successes, a median of 88 in 30 steps.
        goals = [(0.8 * x, 0.8 * y) for x, y in GOALS4]
        env = MultiTaskPointVecEnv(n, goals, round_robin_strategy,
                                   'add-onehot', NAMES4, start='spread',
                                   seed=11, done_bonus=0.5,
                                   max_episode_length=P)
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.1,
                                **options)
        with torch.no_grad():
            last = len(hidden)
            pol.net.weight(last).mul_(0.1)
            pol.net.bias(last).mul_(0.1)
    else:
        env = GridWorldVecEnv(n, kind, max_episode_length=P)
        pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hidden, **options)
    with torch.no_grad():  # gamma / beta (the buffer's tail) away from (1, 0)
        if pol.net.ln_off:
            lo = pol.net.ln_off[0]
            pol.net.params[lo:].add_(
                torch.randn_like(pol.net.params[lo:]) * 0.05)
    s = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                      worker_class=GpuVecWorker, seed=2,
                      worker_args=dict(n_envs=n))
    return s, s._workers[0]


@pytest.mark.parametrize('kind,hidden,options,launches', [
    ('point', (64, 64), dict(hidden_nonlinearity=torch.relu), 1),
    ('point', (64, 64), dict(hidden_nonlinearity=F.elu, **LN), 1),
    ('point', (256, 256), dict(hidden_nonlinearity=torch.sigmoid), 1),
    ('4x4', (64, 64), dict(hidden_nonlinearity=torch.relu), 1),
    ('multitask', (64, 64), dict(hidden_nonlinearity=F.leaky_relu, **LN), 1),
    ('8x8', (64, 64), dict(hidden_nonlinearity=torch.relu), 0),
], ids=['point-relu', 'point-elu-ln', 'point-sigmoid-256', 'grid4x4-relu',
        'multitask-leaky_relu-ln', 'grid8x8-relu-streamed'])
def test_one_launch_rollout_with_options_equals_the_per_step_path(
        kind, hidden, options, launches):
    from garage_amd import _lib
    lib = _lib.load()
    (sa, wa), (sb, wb) = (_make(kind, hidden, options),
                          _make(kind, hidden, options))
    assert wb._fused_ok()
    num = 3 * 48 * 20 // 2
    got = _stepwise(wa, num)
    before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
    whole = wb.rollout_samples(num).to_host()
    torch.cuda.synchronize()
    assert int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before == launches
    _same(got, whole)
    assert np.isfinite(whole.agent_infos[
        'prob' if kind in ('4x4', '8x8') else 'mean']).all()
    if kind in ('point', 'multitask'):
        # (the reset path inside the launch is exercised)
        assert whole.env_infos['success'].any()
    if kind == 'multitask':
        assert sorted(set(whole.env_infos['task_id'])) == [0, 1, 2, 3]


def test_normalized_env_statistics_inside_the_launch_with_options():
    """NormalizedVecEnv(normalize_obs, normalize_reward) over the ragged
    synthetic env behind a relu + LayerNorm policy: ``ga_rollout_env_steps``
    against Python-driven steps, bit for bit, twice in a row (the second call
    exercises the partial reset and the odd / even buffer parity)."""
    from garage_amd.envs import NormalizedVecEnv, SyntheticVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker

    class PythonSteps(GpuVecWorker):

        def _native_steps(self, b, col, n_steps):
            return False

    n, P, O, A = 70, 11, 6, 3
    out = []
    for cls in (GpuVecWorker, PythonSteps):
        torch.manual_seed(4)
        env = SyntheticVecEnv(n, O, A, P, min_len=3, seed=8)
        env = NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                               scale_reward=0.5, obs_alpha=0.05,
                               reward_alpha=0.05)
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=(32, 32),
                                hidden_nonlinearity=torch.relu,
                                layer_normalization=True)
        with torch.no_grad():
            lo = pol.net.ln_off[0]
            pol.net.params[lo:].add_(
                torch.randn_like(pol.net.params[lo:]) * 0.05)
        sampler = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                                seed=3, worker_class=cls,
                                worker_args=dict(n_envs=n))
        assert sampler._workers[0]._fused_ok()
        out.append([sampler.obtain_samples(0, num, None)
                    for num in (n * P, n * P + 17)])
    for a, b in zip(*out):
        assert np.array_equal(a.lengths, b.lengths)
        assert np.array_equal(a.observations, b.observations)
        assert np.array_equal(a.actions, b.actions)
        assert np.array_equal(a.rewards, b.rewards)
        assert np.array_equal(a.last_observations, b.last_observations)
        assert np.array_equal(a.agent_infos['mean'], b.agent_infos['mean'])
        assert np.isfinite(a.observations).all() and a.lengths.sum() > 0
        assert np.array_equal([int(s) for s in a.step_types],
                              [int(s) for s in b.step_types])


def _relu_net(O, A, hidden, M):
    from garage_amd.engine import FlatMLP, pad_rows, require_gpu
    dev = require_gpu()
    rng = np.random.RandomState(0)
    net = FlatMLP(O, A, hidden, dev, hidden_act='relu')
    for l in range(len(hidden) + 1):
        net.weight(l).copy_(torch.from_numpy(
            (rng.randn(net.dims[l + 1], net.dims[l]) * 0.2).astype(np.float32)))
        net.bias(l).copy_(torch.from_numpy(
            (rng.randn(net.dims[l + 1]) * 0.2).astype(np.float32)))
    X = pad_rows(rng.randn(M, O).astype(np.float32))
    return net, X


def test_training_forward_of_a_relu_network_stays_on_the_per_layer_gemms():
    """The widened rollout predicate does not leak into ga_mlp_forward_f32's
    dispatch to the (tanh only) fused training forward."""
    from garage_amd._lib import load
    O, A, hidden, M = 5, 3, (16, 40), 333
    net, X = _relu_net(O, A, hidden, M)
    lib = load()
    assert lib.ga_policy_step_fused_supported(C.byref(net._desc)) == 1
    lib.ga_set_fused_forward(0)
    want = net.forward(X, M).clone()
    want_acts = net._acts.clone()
    try:
        lib.ga_set_fused_forward(1)
        got = net.forward(X, M).clone()
        got_acts = net._acts.clone()
    finally:
        lib.ga_set_fused_forward(0)
    assert torch.equal(got, want)
    assert torch.equal(got_acts, want_acts)
    ref = torch.from_numpy(X.cpu().numpy()[:, :O].astype(np.float64))
    for l in range(3):
        ref = ref @ net.weight(l).double().cpu().T + net.bias(l).double().cpu()
        if l < 2:
            ref = torch.relu(ref)
    assert np.allclose(got[:, :A].cpu().numpy(), ref.numpy(), atol=1e-5)


def test_fused_training_forward_refuses_a_relu_network():
    """A direct ABI caller does not get tanh applied to a relu network."""
    from garage_amd._lib import GarageAmdError, call, dptr, stream_ptr
    O, A, hidden, M = 5, 3, (16, 40), 333
    net, X = _relu_net(O, A, hidden, M)
    net._workspace(M)
    out = torch.zeros(M, net.ld_out, device=X.device)
    with pytest.raises(GarageAmdError, match='unsupported'):
        call('ga_mlp_forward_fused_f32', C.byref(net._desc), dptr(net.params),
             dptr(X), X.stride(0), None, M, dptr(net._acts), dptr(out),
             out.stride(0), stream_ptr())
