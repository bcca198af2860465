"""The one-launch rollout step for networks with layer inputs up to 512 wide
(``policy_step_fused_kernel<WIDTH = 512>``: 256-column panels, weights streamed):

A. the wide step against the per-layer path, both measured against an fp64
   evaluation of the policy's own parameters on the first step's observations;
B. a whole rollout in ONE launch bit for bit against the same kernel stepped
   one launch at a time, for device envs behind wide networks;
C. the NormalizedEnv statistics inside that launch against Python-driven steps;
D. C5's policy -- MLP(512, 512, 512), obs 376, act 17 -- against the oracle's
   ``VecWorker``;
E. the training forward of a wide network stays on the per-layer GEMMs;
F. a (256, 256) policy against its zero-padded (272, 272) twin, bit for bit: the
   kernel at WIDTH = 256 (weights resident and streamed) against WIDTH = 512.

Measured on an MI355X: see DESIGN.md, "Networks up to 512 wide through the
one-launch rollout".
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _mlp_option_cases import TOL_FORWARD
from test_device_envs_gpu import _same, _stepwise
from test_rollout_options_gpu import LN, _first_step, _make, _sampler

pytestmark = pytest.mark.gpu

# csrc/prof.h: whole rollouts in one launch (weights resident / wide, streamed)
GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE = 13, 14

# (discrete, O, A, hidden, n_envs)
W1 = (False, 5, 3, (272, ), 20)       # one 16-column tile in the second panel
W2 = (False, 300, 7, (257, 511), 33)  # wide input, odd widths, ldw padding
W3 = (True, 300, 2, (64, ), 17)       # only the input is wide
W4 = (True, 9, 32, (512, ), 24)       # widest head x widest layer (64 KB block)
W5 = (False, 376, 17, (512, 512, 512), 40)  # C5's network
W6 = (False, 12, 4, (260, ) * 7, 16)  # eight layers, tile ping-pong
NAMES = {W1: 'w1', W2: 'w2', W3: 'w3', W4: 'w4', W5: 'w5', W6: 'w6'}

CASES = (
    [(s, {}) for s in (W1, W2, W3, W4, W5, W6)] +
    [(W2, dict(hidden_nonlinearity=torch.relu)),
     (W2, dict(hidden_nonlinearity=F.softplus)),
     (W2, dict(hidden_nonlinearity=torch.tanh, **LN)),
     (W2, dict(hidden_nonlinearity=torch.relu, output_nonlinearity=torch.tanh,
               **LN)),
     (W5, dict(hidden_nonlinearity=F.elu, **LN)),
     (W1, dict(output_nonlinearity=torch.sigmoid))])


def _case_id(case):
    shape, options = case
    name = NAMES[shape]
    for key, val in options.items():
        name += '-' + key.split('_')[0] + '_' + (
            getattr(val, '__name__', str(val)))
    return name


def _predicates(net):
    from garage_amd import _lib
    lib = _lib.load()
    return (int(lib.ga_policy_step_fused_supported(C.byref(net._desc))),
            int(lib.ga_policy_step_wide_supported(C.byref(net._desc))))


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_wide_step_matches_per_layer_path(case):
    (discrete, O, A, hidden, n), options = case
    P = 9
    torch.manual_seed(3)
    noise = torch.rand(40, n, 32) if discrete else torch.randn(40, n, 20)
    args = (discrete, O, A, hidden, n, P, noise, options)
    sa, pa = _sampler(True, *args)
    assert sa._workers[0]._fused_ok()
    assert _predicates(pa.net) == (0, 1)
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
    # the first step of both paths against fp64.  TOL_FORWARD is the suite's
    # figure for fp32 results that differ in summation order only (relative to
    # the largest reference value); the factor 2 on the per-layer path's own
    # error allows for another order of the same terms where that error is
    # already larger
    obs_w, head_w, want = _first_step(True, *args)
    obs_p, head_p, _ = _first_step(False, *args)
    assert np.array_equal(obs_w, obs_p)
    err_w = float(np.abs(head_w - want).max())
    err_p = float(np.abs(head_p - want).max())
    print('rollout wide %s: wide %.3e per-layer %.3e' %
          (_case_id(case), err_w, err_p))
    assert np.isfinite(head_w).all()
    bound = max(TOL_FORWARD * max(1.0, float(np.abs(want).max())), 2 * err_p)
    assert err_w <= bound, (err_w, err_p, bound)


@pytest.mark.parametrize('kind,hidden,options', [
    ('point', (320, 320), {}),
    ('point', (257, 511), dict(hidden_nonlinearity=torch.relu, **LN)),
    ('4x4', (512, ), {}),
    ('multitask', (272, 272), dict(hidden_nonlinearity=F.leaky_relu, **LN)),
], ids=['point-320', 'point-257-511-relu-ln', 'grid4x4-512',
        'multitask-272-leaky_relu-ln'])
def test_one_wide_launch_equals_the_per_step_path(kind, hidden, options):
    from garage_amd import _lib
    lib = _lib.load()
    (sa, wa), (sb, wb) = (_make(kind, hidden, options),
                          _make(kind, hidden, options))
    assert wb._fused_ok()
    assert _predicates(wb.agent.net) == (0, 1)
    num = 3 * 48 * 20 // 2
    got = _stepwise(wa, num)
    before = [int(lib.ga_launch_count(k))
              for k in (GA_PROF_ROLLOUT_WIDE, GA_PROF_ROLLOUT)]
    whole = wb.rollout_samples(num).to_host()
    torch.cuda.synchronize()
    after = [int(lib.ga_launch_count(k))
             for k in (GA_PROF_ROLLOUT_WIDE, GA_PROF_ROLLOUT)]
    assert after[0] - before[0] == 1
    assert after[1] - before[1] == 0
    _same(got, whole)
    assert np.isfinite(whole.agent_infos[
        'prob' if kind == '4x4' else 'mean']).all()
    if kind in ('point', 'multitask'):
        # (the reset path inside the launch is exercised)
        assert whole.env_infos['success'].any()
    if kind == 'multitask':
        assert sorted(set(whole.env_infos['task_id'])) == [0, 1, 2, 3]


def test_normalized_env_statistics_inside_the_wide_launch():
    """NormalizedVecEnv(normalize_obs, normalize_reward) over the ragged
    synthetic env with 300-wide observations behind a (272,) relu + LayerNorm
    policy: ``ga_rollout_env_steps`` against Python-driven steps, bit for bit,
    twice in a row (the second call exercises the partial reset and the odd /
    even buffer parity)."""
    from garage_amd.envs import NormalizedVecEnv, SyntheticVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker

    class PythonSteps(GpuVecWorker):

        def _native_steps(self, b, col, n_steps):
            return False

    n, P, O, A = 70, 11, 300, 3
    out = []
    for cls in (GpuVecWorker, PythonSteps):
        torch.manual_seed(4)
        env = SyntheticVecEnv(n, O, A, P, min_len=3, seed=8)
        env = NormalizedVecEnv(env, normalize_obs=True, normalize_reward=True,
                               scale_reward=0.5, obs_alpha=0.05,
                               reward_alpha=0.05)
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=(272, ),
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
        assert _predicates(pol.net) == (0, 1)
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


# D: bounds on |wide launch - oracle| for means, actions and rewards.  1e-5, the
# bound of test_c3_whole_rollout_launch_matches_oracle_vecworker, holds as long
# as the per-layer path (the same case with fused_policy_step=False) stays
# within 5e-6 of the oracle; see the test's docstring for what it measured.
C5_ATOL = {'mean': 1e-5, 'actions': 1e-5, 'rewards': 1e-5}


def test_c5_whole_rollout_launch_matches_oracle_vecworker():
    """The rollout of C5's policy -- MLP(512, 512, 512), obs 376, act 17, ragged
    episodes L ~ U{8..64}, 24 envs, device Philox action noise -- with its
    first ``ceil(num / n)`` steps in ONE ``policy_step_fused_kernel<512>`` launch
    against the oracle's ``VecWorker`` (``sampler/vec_worker.py:176-204``)
    stepping the per-env CPU twins with the same noise stream: observations /
    last observations / lengths / step types bit for bit, means / actions /
    rewards to ``C5_ATOL``.  The per-layer path runs the same case first.

    Measured on an MI355X, max |difference to the oracle| (mean / actions /
    rewards): per-layer path 2.03e-6 / 2.03e-6 / 5.7e-7, wide launch 1.61e-6 /
    1.61e-6 / 4.8e-7.  The per-layer path is within 5e-6 in all three, so the
    bound is 1e-5 for each."""
    import bench
    from garage_amd import _lib
    from garage_amd.envs import SyntheticVecEnv
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    from oracle import envs as oenvs
    from oracle import networks as nets
    from oracle import sampler as osamp
    lib = _lib.load()
    cfg = bench.CONFIGS['c5']
    n, O, A, P, min_len = 24, cfg['obs_dim'], cfg['act_dim'], 64, 8
    assert (O, A, tuple(cfg['hidden'])) == (376, 17, (512, 512, 512))
    seed = 9
    noise_seed = seed + 7919  # GpuVecWorker: seed + 7919 (worker_number + 1)

    def gpu_run(fused):
        torch.manual_seed(seed)
        env = SyntheticVecEnv(n, O, A, P, min_len=min_len, seed=seed)
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=cfg['hidden'])
        sampler = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                                worker_class=GpuVecWorker, seed=seed,
                                worker_args=dict(n_envs=n,
                                                 fused_policy_step=fused))
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT_WIDE))
        eps = sampler.obtain_samples(0, n * P, None)
        torch.cuda.synchronize()
        launched = int(lib.ga_launch_count(GA_PROF_ROLLOUT_WIDE)) - before
        return eps, pol.state_dict(), launched

    per_layer, params, launched = gpu_run(False)
    assert launched == 0
    wide, params_w, launched = gpu_run(True)
    assert launched == 1
    for key in params:
        assert np.array_equal(np.asarray(params[key]), np.asarray(params_w[key]))

    class CpuPolicy:
        calls = 0

        def reset(self, do_resets=None):
            pass

        def get_actions(self, obs):
            with torch.no_grad():
                dist, info = nets.policy_forward(
                    params, torch.from_numpy(np.asarray(obs, np.float32)))
            z = oenvs.action_noise(noise_seed, np.arange(n), self.calls, A)
            a = dist.mean + dist.stddev * torch.from_numpy(z)
            self.calls += 1
            return a.numpy(), {'mean': info['mean'].numpy()}

    ref = osamp.OracleLocalSampler(
        CpuPolicy(),
        [[oenvs.SyntheticEnv(i, O, A, P, min_len=min_len, seed=seed)
          for i in range(n)]], max_episode_length=P, n_workers=1,
        worker_class=osamp.OracleVecWorker, worker_args=dict(n_envs=n))
    want = ref.obtain_samples(0, n * P, None)

    def deviations(eps):
        assert np.array_equal(eps.lengths, want.lengths)
        assert np.array_equal([int(s) for s in eps.step_types],
                              [int(s) for s in want.step_types])
        assert np.array_equal(eps.observations, want.observations)  # bit exact
        assert np.array_equal(eps.last_observations, want.last_observations)
        return {
            'mean': float(np.abs(eps.agent_infos['mean'] -
                                 want.agent_infos['mean']).max()),
            'actions': float(np.abs(eps.actions - want.actions).max()),
            'rewards': float(np.abs(eps.rewards - want.rewards).max())}

    lens = np.asarray(want.lengths)
    assert lens.min() >= min_len and lens.max() <= P and len(set(lens)) > 10
    dev_p, dev_w = deviations(per_layer), deviations(wide)
    print('c5 rollout vs oracle: per-layer %s wide %s' % (dev_p, dev_w))
    for key, atol in C5_ATOL.items():
        assert dev_w[key] <= atol, (key, dev_w[key], dev_p[key])
    # the draws are standard normal: a wrong stream would still pass "close"
    z = (wide.actions - wide.agent_infos['mean']) / np.exp(
        wide.agent_infos['log_std'])
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02


def _wide_net(M):
    from garage_amd.engine import FlatMLP, pad_rows, require_gpu
    O, A, hidden = 300, 7, (257, 511)
    dev = require_gpu()
    rng = np.random.RandomState(0)
    net = FlatMLP(O, A, hidden, dev)
    for l in range(len(hidden) + 1):
        net.weight(l).copy_(torch.from_numpy(
            (rng.randn(net.dims[l + 1], net.dims[l]) *
             (1.0 / np.sqrt(net.dims[l]))).astype(np.float32)))
        net.bias(l).copy_(torch.from_numpy(
            (rng.randn(net.dims[l + 1]) * 0.2).astype(np.float32)))
    X = pad_rows(rng.randn(M, O).astype(np.float32))
    return net, X


def test_training_forward_of_a_wide_network_stays_on_the_per_layer_gemms():
    """The wide rollout predicate does not leak into ga_mlp_forward_f32's
    dispatch to the fused training forward (256-wide tiles)."""
    from garage_amd._lib import load
    M = 333
    net, X = _wide_net(M)
    lib = load()
    assert _predicates(net) == (0, 1)
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
    assert np.isfinite(got.cpu().numpy()).all()


def test_fused_training_forward_refuses_a_wide_network():
    from garage_amd._lib import GarageAmdError, call, dptr, stream_ptr
    M = 333
    net, X = _wide_net(M)
    net._workspace(M)
    out = torch.zeros(M, net.ld_out, device=X.device)
    with pytest.raises(GarageAmdError, match='unsupported'):
        call('ga_mlp_forward_fused_f32', C.byref(net._desc), dptr(net.params),
             dptr(X), X.stride(0), None, M, dptr(net._acts), dptr(out),
             out.stride(0), stream_ptr())


def _zero_padded_pair(make_env, nonlinearity, n, P):
    """[(worker, policy)] of a (256, 256) Gaussian policy and of a (272, 272) one
    that holds the first's parameters in the leading blocks and exactly zero
    elsewhere, each over its own env batch from ``make_env()``, same seeds,
    device RNG."""
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    out = []
    for hidden in ((256, 256), (272, 272)):
        torch.manual_seed(6)
        env = make_env()
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden, init_std=0.1,
                                hidden_nonlinearity=nonlinearity)
        with torch.no_grad():
            if not out:  # biases away from zero
                for l in range(3):
                    pol.net.bias(l).add_(
                        torch.randn_like(pol.net.bias(l)) * 0.05)
            else:
                src = out[0][1].net
                pol.net.params.zero_()
                pol.net.params[:4].copy_(src.params[:4])  # log_std
                for l in range(3):
                    rows, cols = src.dims[l + 1], src.dims[l]
                    pol.net.weight(l)[:rows, :cols].copy_(src.weight(l))
                    pol.net.bias(l)[:rows].copy_(src.bias(l))
        s = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                          worker_class=GpuVecWorker, seed=2,
                          worker_args=dict(n_envs=n))
        assert s._workers[0]._fused_ok()
        out.append((s._workers[0], pol))
    assert _predicates(out[0][1].net) == (1, 1)
    assert _predicates(out[1][1].net) == (0, 1)
    return out


# launches of (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE) by the 256 side / the wide side
@pytest.mark.parametrize('nonlinearity', [torch.tanh, torch.relu],
                         ids=['tanh', 'relu'])
@pytest.mark.parametrize('kind,whole,counts', [
    ('point', True, ((1, 0), (0, 1))),
    ('synthetic', True, ((0, 0), (0, 1))),
    ('synthetic', False, ((0, 0), (0, 0))),
], ids=['a-resident', 'b-streamed', 'c-streamed-per-step'])
def test_zero_padding_across_the_256_boundary_keeps_the_bits(
        kind, whole, counts, nonlinearity):
    """A (256, 256) policy against its zero-padded (272, 272) twin: with tanh and
    with relu f(0) = 0, so the twin's extra products are zeros added in ascending
    k after the same terms, and the rollouts agree bit for bit -- (a) PointVecEnv,
    P = 6 steps in one launch, the resident WIDTH = 256 kernel against WIDTH =
    512; (b) SyntheticVecEnv with O = 40, A = 3, the streamed WIDTH = 256 kernel
    against WIDTH = 512; (c) as (b), one step per launch.  20 envs: one full and
    one partial workgroup.  No LayerNorm: it depends on the width."""
    from garage_amd import _lib
    from garage_amd.envs import PointVecEnv, SyntheticVecEnv
    lib = _lib.load()
    n, P = 20, 6

    def make_env():
        if kind == 'point':
            return PointVecEnv(n, goal=(0.1, 0.1), done_bonus=0.5,
                               max_episode_length=P)
        return SyntheticVecEnv(n, 40, 3, P, min_len=2, seed=5)

    got = []
    for (worker, pol), want in zip(
            _zero_padded_pair(make_env, nonlinearity, n, P), counts):
        assert pol.net.in_dim <= 32 if kind == 'point' else pol.net.in_dim == 40
        before = [int(lib.ga_launch_count(k))
                  for k in (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)]
        if whole:
            eps = worker.rollout_samples(n * P).to_host()
        else:
            eps = _stepwise(worker, n * P)
        torch.cuda.synchronize()
        after = [int(lib.ga_launch_count(k))
                 for k in (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)]
        assert tuple(x - y for x, y in zip(after, before)) == want
        got.append(eps)
    a, b = got
    mean = a.agent_infos['mean']
    assert np.isfinite(mean).all() and np.abs(mean).max() > 0
    assert np.array_equal(a.observations, b.observations)
    assert np.array_equal(a.actions, b.actions)
    assert np.array_equal(mean, b.agent_infos['mean'])
    assert np.array_equal(a.lengths, b.lengths)
    assert np.array_equal([int(s) for s in a.step_types],
                          [int(s) for s in b.step_types])
