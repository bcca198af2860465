"""VPG, PPO and TRPO with a ``LinearFeatureBaseline`` as ``value_function``
(PointVecEnv, 16 envs, MLP(32, 32), max_episode_length 20), against the fp64
numpy twin of ``_linear_baseline_cases.py``.

Bounds, as in ``test_linear_baseline_gpu.py``: an fp32 result of an fp64 sum is
held to 2^-23 * max(|x|, 1); the coefficients of a fit may move the predictions
by 100 times the twin's own permutation spread (at least 1e-9 * max |v|),
measured on the features they are applied to.  The advantages are checked
twice: the numpy GAE fed the device's own (fp32, exactly representable)
baselines must agree at the fp32 bound, and fed the TWIN's baselines at that
bound plus what the baselines' own allowance can move an advantage by -- an
advantage is a sum of c^k (r + gamma v' - v), so at most 2 / (1 - c) times it.
"""
import pickle

import numpy as np
import pytest
import torch

import _linear_baseline_cases as lc

pytestmark = pytest.mark.gpu

N_ENVS, P = 16, 20
DISCOUNT, GAE_LAMBDA = 0.99, 0.95
EPS32 = 2.0 ** -23


def _build(name, linear=True, **extra):
    from garage_amd import algos
    from garage_amd.baselines import LinearFeatureBaseline
    from garage_amd.envs import PointVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(0)
    env = PointVecEnv(N_ENVS, max_episode_length=P)
    # goals at different distances: some episodes end early, the lengths differ
    env.set_tasks([{'goal': (0.15 * (i % 4), 0.1 * (i // 4))}
                   for i in range(N_ENVS)])
    pol = GaussianMLPPolicy(env.spec, hidden_sizes=(32, 32))
    if linear:
        vf = LinearFeatureBaseline(env.spec)
    else:
        vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(32, 32))
    sampler = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                            worker_class=GpuVecWorker, seed=3,
                            worker_args=dict(n_envs=N_ENVS))
    kwargs = dict(env_spec=env.spec, policy=pol, value_function=vf,
                  sampler=sampler, discount=DISCOUNT, gae_lambda=GAE_LAMBDA,
                  center_adv=False)
    adam = (torch.optim.Adam, dict(lr=1e-3))
    if name != 'TRPO':
        kwargs['policy_optimizer'] = OptimizerWrapper(adam, pol, 2, 64)
        if not linear:
            kwargs['vf_optimizer'] = OptimizerWrapper(adam, vf, 2, 64)
    kwargs.update(extra)
    return getattr(algos, name)(**kwargs)


def _iterate(algo, itr):
    eps = algo._sampler.obtain_samples(itr, N_ENVS * P, None)
    np.random.seed(100 + itr)
    algo._train_once(itr, eps)
    return eps


def _host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _twin_fit(eps, returns):
    """(phi, coefficients, allowance of the fit's predictions) of the twin on a
    batch's fp32 observations and the device's fp32 returns."""
    O = eps.env_spec.observation_space.flat_dim
    phi = lc.features(_host(eps.obs_dev[:, :O]), list(eps.lengths))
    coeffs = lc.fit(phi, returns)
    spread = lc.permutation_spread(phi, returns)
    assert spread <= 1e-8  # the batch can pin something
    return phi, coeffs, spread


def _fp32_bound(x):
    return EPS32 * np.maximum(np.abs(x), 1.0)


ALGOS = ['VPG', 'PPO', 'TRPO']


@pytest.mark.parametrize('name', ALGOS)
def test_two_iterations_against_the_twin(name):
    algo = _build(name)
    vf = algo._value_function
    # ---- iteration 1: no coefficients yet
    eps1 = _iterate(algo, 0)
    lengths1 = list(eps1.lengths)
    assert len(set(lengths1)) > 1  # ragged, or the test shows less than it says
    t1 = algo.last_tensors
    assert t1['v0'] == 0.0 and not bool(t1['values'].any())
    rewards1 = _host(eps1.rewards_dev)
    adv1, ret1 = lc.gae(rewards1, np.zeros_like(rewards1), lengths1, DISCOUNT,
                        GAE_LAMBDA)
    returns1 = _host(t1['returns'])
    assert (np.abs(returns1 - ret1) <= _fp32_bound(ret1)).all()
    assert (np.abs(_host(t1['advantages']) - adv1) <= _fp32_bound(adv1)).all()
    phi1, c1, spread1 = _twin_fit(eps1, returns1)
    tab = algo.last_tabular
    before, after = np.mean(returns1 ** 2), np.mean(
        (phi1.dot(c1) - returns1) ** 2)
    assert abs(tab['vf/LossBefore'] - before) <= 1e-6 * before
    assert abs(tab['vf/LossAfter'] - after) <= 1e-6 * after
    assert tab['vf/LossAfter'] <= tab['vf/LossBefore']
    got = vf.get_param_values()
    moved = np.abs(phi1.dot(got) - phi1.dot(c1)).max()
    allow1 = max(100 * spread1, 1e-9 * np.abs(phi1.dot(c1)).max())
    print(name, 'fit 1 moved the predictions by', moved, 'of', allow1)
    assert moved <= allow1

    # ---- iteration 2: the baselines are iteration 1's fit
    eps2 = _iterate(algo, 1)
    lengths2 = list(eps2.lengths)
    t2 = algo.last_tensors
    assert t2['v0'] == 0.0
    O = eps2.env_spec.observation_space.flat_dim
    phi2 = lc.features(_host(eps2.obs_dev[:, :O]), lengths2)
    values2 = _host(t2['values'])
    # the kernel, with the coefficients the fit left: the fp32 bound
    kept = phi2.dot(got)
    assert (np.abs(values2 - kept) <= _fp32_bound(kept)).all()
    # the twin's: also what iteration 1's fit may move THIS batch's predictions
    # by -- the twin's own order sensitivity, measured on these features
    want_v = phi2.dot(c1)
    spread12 = lc.permutation_spread(phi1, returns1, eval_phi=phi2)
    allow_v = max(100 * spread12, 1e-9 * np.abs(want_v).max()) \
        + _fp32_bound(want_v)
    print(name, 'values moved by', np.abs(values2 - want_v).max(), 'of',
          allow_v.max())
    assert (np.abs(values2 - want_v) <= allow_v).all()
    rewards2 = _host(eps2.rewards_dev)
    returns2 = _host(t2['returns'])
    adv_dev = _host(t2['advantages'])
    # the numpy GAE on the device's own baselines: the fp32 bound, nothing else
    adv2, ret2 = lc.gae(rewards2, values2, lengths2, DISCOUNT, GAE_LAMBDA)
    assert (np.abs(returns2 - ret2) <= _fp32_bound(ret2)).all()
    assert (np.abs(adv_dev - adv2) <= _fp32_bound(adv2)).all()
    # ... and on the twin's
    adv_twin, _ = lc.gae(rewards2, want_v, lengths2, DISCOUNT, GAE_LAMBDA)
    c = float(np.float32(DISCOUNT * GAE_LAMBDA))
    assert (np.abs(adv_dev - adv_twin) <= _fp32_bound(adv_twin)
            + 2.0 / (1.0 - c) * allow_v.max()).all()
    _, c2, _ = _twin_fit(eps2, returns2)
    tab = algo.last_tabular
    before = np.mean((values2 - returns2) ** 2)
    before_twin = np.mean((want_v - returns2) ** 2)
    after = np.mean((phi2.dot(c2) - returns2) ** 2)
    assert abs(tab['vf/LossBefore'] - before) <= 1e-6 * before
    assert abs(tab['vf/LossBefore'] - before_twin) <= 1e-6 * before_twin
    assert abs(tab['vf/LossAfter'] - after) <= 1e-6 * after
    assert tab['vf/LossAfter'] <= tab['vf/LossBefore']
    assert abs(tab['vf/dLoss'] - (tab['vf/LossBefore'] - tab['vf/LossAfter'])) \
        <= 1e-12 * before


@pytest.mark.parametrize('name', ALGOS)
def test_the_policys_passes_are_todays(name):
    """Fed the same (batch, adv, returns, old_ll) and the same np.random state,
    the policy after ``_train`` has the bits of the same algo built with an MLP
    value function and ``overlap_updates = False``."""
    lin, mlp = _build(name), _build(name, linear=False)
    mlp.overlap_updates = False
    assert torch.equal(lin.policy.net.params, mlp.policy.net.params)
    eps = lin._sampler.obtain_samples(0, N_ENVS * P, None)
    c = lin._before_train(eps)
    mlp._before_train(eps)  # (its workspaces and its share of the batch)
    start = lin.policy.net.params.clone()
    for algo in (lin, mlp):
        np.random.seed(7)
        algo._train(c.batch, c.adv, c.returns, c.old_ll)
    torch.cuda.synchronize()
    a, b = lin.policy.net, mlp.policy.net
    assert not torch.equal(a.params, start)  # a step was taken
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.exp_avg, b.exp_avg)
    assert torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert a.adam_steps == b.adam_steps
    assert lin._value_function.get_param_values() is not None


def test_mlp_value_function_still_runs():
    algo = _build('PPO', linear=False)
    _iterate(algo, 0)
    tab = algo.last_tabular
    assert np.isfinite(tab['vf/LossBefore']) and np.isfinite(tab['vf/LossAfter'])
    assert algo._value_function.net.adam_steps > 0
    assert 'v0' in algo.last_tensors


@pytest.mark.parametrize('name', ALGOS)
def test_a_vf_optimizer_beside_a_linear_baseline_raises(name):
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPValueFunction
    probe = _build(name)
    other = GaussianMLPValueFunction(probe._env_spec, hidden_sizes=(32, 32))
    with pytest.raises(ValueError) as e:
        _build(name, vf_optimizer=OptimizerWrapper(torch.optim.Adam, other))
    assert 'vf_optimizer' in str(e.value)


def test_shard_algo_and_population_raise():
    from garage_amd.algos import PopulationPPO
    from garage_amd.distributed import shard_algo
    algo = _build('PPO')
    with pytest.raises(ValueError) as e:
        shard_algo(algo, object())
    assert 'LinearFeatureBaseline' in str(e.value)
    assert algo._comm is None
    with pytest.raises(ValueError) as e:
        PopulationPPO([algo])
    assert 'LinearFeatureBaseline' in str(e.value)


def test_snapshot_mid_run_keeps_the_coefficients():
    algo = _build('PPO')
    _iterate(algo, 0)
    blob = pickle.dumps(algo)
    coeffs = algo._value_function.get_param_values().copy()
    _iterate(algo, 1)
    resumed = pickle.loads(blob)
    assert np.array_equal(resumed._value_function.get_param_values(), coeffs)
    _iterate(resumed, 1)
    assert np.array_equal(resumed._value_function.get_param_values(),
                          algo._value_function.get_param_values())
    assert torch.equal(resumed.policy.net.params, algo.policy.net.params)
    assert resumed.last_tabular == algo.last_tabular
    assert torch.equal(resumed.last_tensors['values'],
                       algo.last_tensors['values'])
