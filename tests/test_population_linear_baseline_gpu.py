"""``PopulationPPO`` with the members of a ``LinearFeatureBaselinePopulation`` as
value functions, against lone ``PPO`` / ``VPG`` objects with lone
``LinearFeatureBaseline`` objects on the same batches.

The contract is the project's twin rule: each member gets, bit for bit, what the
lone learner gets on the narrow path (``ga_set_small_step(0)``) -- the baseline's
coefficients, the policy's parameters and both Adam moments, ``last_tabular`` and
``last_tensors`` -- with the same ``np.random`` state, the lone runs one after
another in member order.  Two iterations: the second is the first with non-zero
baselines.
"""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 3
REG = (1e-5, 1e-3, 1e-1)


@pytest.fixture
def narrow_path():
    """The lone runs take ``narrow_train_kernel``: small step off, narrow step on."""
    from garage_amd import _lib
    lib = _lib.load()
    lib.ga_set_small_step(0)
    lib.ga_set_narrow_step(1)
    try:
        yield lib
    finally:
        lib.ga_set_small_step(1)
        lib.ga_set_narrow_step(1)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _make(head, algo='PPO', joint=True):
    """(env, learners, baselines): categorical MLP(32, 32) on CartPole, where the
    episodes terminate, or Gaussian MLP(64, 64) on Pendulum with episodes of 20
    steps and 160 samples (8 x 20) asked of a member -- on 16 envs a member, the
    fewest the population rollout gives one; the members differ in ``lr``, clip
    range, seeds and ``reg_coeff``.
    ``joint``: the baselines are one population's members, else lone objects."""
    from garage_amd import algos
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    from garage_amd.envs import CartPoleVecEnv, PendulumVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    if head == 'categorical':
        env = CartPoleVecEnv(M * 16, max_episode_length=40, seed=3)
    else:
        env = PendulumVecEnv(M * 16, max_episode_length=20, seed=3)
    if joint:
        baselines = list(LinearFeatureBaselinePopulation(env.spec, M,
                                                         reg_coeff=REG))
    else:
        baselines = [LinearFeatureBaseline(env.spec, reg_coeff=r) for r in REG]
    learners = []
    for m in range(M):
        torch.manual_seed(10 + m)
        if head == 'categorical':
            pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(32, 32))
        else:
            pol = GaussianMLPPolicy(env.spec, hidden_sizes=(64, 64))
        kw = dict(lr_clip_range=0.1 + 0.05 * m) if algo == 'PPO' else {}
        learners.append(getattr(algos, algo)(
            env_spec=env.spec, policy=pol, value_function=baselines[m],
            sampler=None, policy_optimizer=OptimizerWrapper(
                (torch.optim.Adam, dict(lr=1e-3 * (m + 1))), pol, 2, 64,
                seed=m), **kw))
    return env, learners, baselines


def _population(head, algo='PPO', joint_pack=False):
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    env, learners, _ = _make(head, algo)
    pop = PopulationPPO(learners)
    horizon = 40 if head == 'categorical' else 20
    sampler = GpuPopulationSampler(learners[0].policy, env, n_members=M,
                                   max_episode_length=horizon, seed=5,
                                   joint_pack=joint_pack)
    return pop, sampler, 160


def _state(algo):
    net = algo.policy.net
    return dict(
        coeffs=algo._value_function.get_param_values().copy(),
        params=net.params.clone(), exp_avg=net.exp_avg.clone(),
        exp_avg_sq=net.exp_avg_sq.clone(), adam_steps=net.adam_steps,
        tabular=dict(algo.last_tabular),
        tensors={k: (v.clone() if torch.is_tensor(v) else v)
                 for k, v in algo.last_tensors.items()})


def _assert_same(got, want, where):
    assert np.array_equal(got['coeffs'], want['coeffs']), where
    for k in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(_bits(got[k]), _bits(want[k])), (where, k)
    assert got['adam_steps'] == want['adam_steps'], where
    assert got['tabular'] == want['tabular'], where
    assert sorted(got['tensors']) == sorted(want['tensors'])
    for k, v in want['tensors'].items():
        if torch.is_tensor(v):
            assert torch.equal(_bits(got['tensors'][k]), _bits(v)), (where, k)
        else:
            assert got['tensors'][k] == v, (where, k)


@pytest.mark.parametrize('head,algo,joint_pack', [
    ('categorical', 'PPO', False),
    ('categorical', 'PPO', True),
    ('gaussian', 'PPO', False),
    ('gaussian', 'PPO', True),
    ('categorical', 'VPG', False),
])
def test_members_equal_lone_learners_bit_for_bit(head, algo, joint_pack,
                                                 narrow_path):
    pop, sampler, n_samples = _population(head, algo, joint_pack)
    _, lones, _ = _make(head, algo, joint=False)
    assert 'vf' not in pop._rows
    for a, b in zip(pop.members, lones):  # the same initial state
        assert torch.equal(a.policy.net.params, b.policy.net.params)
    np.random.seed(7)
    batches, joint = [], []
    for itr in range(2):
        batches.append(sampler.obtain_samples(itr, n_samples, pop.member_params))
        returns = pop.train_once(itr, batches[-1])
        assert len(returns) == M
        joint.append([_state(a) for a in pop.members])
    if head == 'categorical':
        # CartPole's episodes terminate: the members' batches are ragged
        lengths = np.concatenate([np.asarray(b.lengths) for b in batches[0]])
        assert lengths.min() < lengths.max()
    np.random.seed(7)  # the lone runs draw in member order, as the joint run did
    for itr in range(2):
        for m, lone in enumerate(lones):
            lone._train_once(itr, batches[itr][m])
            _assert_same(joint[itr][m], _state(lone), (itr, m))
    # the second iteration ran with non-zero baselines; the members differ and moved
    assert not bool(joint[0][0]['tensors']['values'].any())
    assert bool(joint[1][0]['tensors']['values'].any())
    assert not torch.equal(joint[1][0]['params'], joint[1][1]['params'])
    assert not torch.equal(joint[1][0]['params'], joint[0][0]['params'])
    assert not np.array_equal(joint[1][0]['coeffs'], joint[0][0]['coeffs'])
    # the members' coefficients are the rows of the population's one tensor
    base = pop._baselines
    assert np.array_equal(base.coeffs_dev.cpu().numpy(),
                          np.stack([s['coeffs'] for s in joint[1]]))


def test_pickle_after_one_iteration_resumes_to_the_same_bits(narrow_path):
    pop, sampler, n_samples = _population('categorical')
    np.random.seed(11)
    pop.train_once(0, sampler.obtain_samples(0, n_samples, pop.member_params))
    copy = pickle.loads(pickle.dumps(pop))
    assert copy._baselines is not pop._baselines
    for m, a in enumerate(copy.members):  # one population, in member order
        assert a._value_function is copy._baselines[m]
        assert a.policy.net.params.data_ptr() == copy.member_params[m].data_ptr()
    batches = sampler.obtain_samples(1, n_samples, pop.member_params)
    state = np.random.get_state()
    pop.train_once(1, batches)
    np.random.set_state(state)
    copy.train_once(1, batches)
    for m, (a, b) in enumerate(zip(pop.members, copy.members)):
        _assert_same(_state(b), _state(a), m)
    assert torch.equal(pop.member_params, copy.member_params)


def test_a_failing_pass_cancels_the_fit(narrow_path):
    pop, sampler, n_samples = _population('categorical')
    batches = sampler.obtain_samples(0, n_samples, pop.member_params)

    def broken(ctxs):
        raise KeyError('the passes failed')

    pop._joint_passes = broken
    with pytest.raises(KeyError):
        pop.train_once(0, batches)
    assert pop._baselines._pending is None
    del pop._joint_passes
    pop.train_once(0, batches)  # the next iteration begins a fit of its own
    assert all(b.get_param_values() is not None for b in pop._baselines)


def test_refusals():
    from garage_amd.algos import PopulationPPO
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    _, lones, _ = _make('categorical', joint=False)
    with pytest.raises(ValueError) as e:  # built on their own
        PopulationPPO(lones)
    assert 'LinearFeatureBaselinePopulation' in str(e.value)
    env, learners, _ = _make('categorical')
    other = LinearFeatureBaselinePopulation(env.spec, M)

    def swap(m, vf):
        learners[m]._value_function = vf

    keep = learners[1]._value_function
    swap(1, other[1])
    with pytest.raises(ValueError) as e:  # two populations
        PopulationPPO(learners)
    assert 'another LinearFeatureBaselinePopulation' in str(e.value)
    swap(1, learners[2]._value_function)
    swap(2, keep)
    with pytest.raises(ValueError) as e:  # one population in the wrong order
        PopulationPPO(learners)
    assert 'member order' in str(e.value)
    # some linear, some MLP
    env, learners, _ = _make('categorical')
    _, mlp, _ = _mlp_learner(env)
    with pytest.raises(ValueError) as e:
        PopulationPPO(learners[:2] + [mlp])
    assert 'value function kind' in str(e.value)


def _mlp_learner(env):
    from garage_amd.algos import PPO
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy,
                                     GaussianMLPValueFunction)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(32, 32))
    vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(32, 32))
    opt = (torch.optim.Adam, dict(lr=1e-3))
    return env, PPO(env_spec=env.spec, policy=pol, value_function=vf,
                    sampler=None,
                    policy_optimizer=OptimizerWrapper(opt, pol, 2, 64, seed=0),
                    vf_optimizer=OptimizerWrapper(opt, vf, 2, 64, seed=1),
                    lr_clip_range=0.2), None
