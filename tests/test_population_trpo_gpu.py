"""``PopulationTRPO``: three TRPO members through ``GpuPopulationSampler`` for two
iterations, with MLP value functions (Pendulum, Gaussian) and with the members of a
``LinearFeatureBaselinePopulation`` (CartPole, categorical).

The accepted backtrack index is NOT compared with a lone ``TRPO``'s: the step length
puts the KL at the constraint by construction, so which side of it a candidate lands
on is a coin toss between two fp32 summation orders.  What must hold is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 3
DELTA = (0.01, 0.02, 0.005)
# 160 samples leave the Fisher matrix of some thousand parameters rank deficient: with the
# default hvp_reg_coeff = 1e-5 ten fp32 conjugate-gradient iterations are not determined
# to the bars below by ANY two summation orders (a numpy fp32 recurrence with the fp64
# product ends 5e-2 from the fp64 one on such data, 7e-7 with 0.1; with 0.1 the members
# agreed with their lone twins to 1e-3 in eleven of twelve steps here and to 7.8e-3 in
# one), so the members regularise at the scale of the Fisher matrix's own eigenvalues,
# where the recurrence converges within its ten iterations
REG = (1.0, 2.0, 1.0)


def _make(head, member_type='TRPO', **cg):
    from garage_amd import algos
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    from garage_amd.envs import CartPoleVecEnv, PendulumVecEnv
    from garage_amd.optimizers import (ConjugateGradientOptimizer,
                                       OptimizerWrapper)
    from garage_amd.policies import (CategoricalMLPPolicy, GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    hidden = cg.pop('hidden', (32, 32))
    if head == 'categorical':
        env = CartPoleVecEnv(M * 16, max_episode_length=40, seed=3)
        vfs = list(LinearFeatureBaselinePopulation(env.spec, M))
    else:
        env = PendulumVecEnv(M * 16, max_episode_length=20, seed=3)
        vfs = [GaussianMLPValueFunction(env.spec, hidden_sizes=(32, 32))
               for _ in range(M)]
    learners = []
    for m in range(M):
        torch.manual_seed(10 + m)
        cls = CategoricalMLPPolicy if head == 'categorical' else GaussianMLPPolicy
        pol = cls(env.spec, hidden_sizes=hidden)
        if member_type == 'PPO':
            learners.append(algos.PPO(env_spec=env.spec, policy=pol,
                                      value_function=vfs[m], sampler=None))
            continue
        kw = dict(max_constraint_value=DELTA[m], hvp_reg_coeff=REG[m])
        kw.update({k: (v[m] if isinstance(v, tuple) else v) for k, v in cg.items()})
        learners.append(algos.TRPO(
            env_spec=env.spec, policy=pol, value_function=vfs[m], sampler=None,
            policy_optimizer=OptimizerWrapper((ConjugateGradientOptimizer, kw), pol)))
    return env, learners


@pytest.mark.parametrize('head', ['gaussian', 'categorical'])
def test_two_iterations_end_to_end(head):
    from garage_amd.algos import PopulationTRPO
    from garage_amd.sampler import GpuPopulationSampler
    env, learners = _make(head)
    _, lones = _make(head)
    pop = PopulationTRPO(learners)
    sampler = GpuPopulationSampler(learners[0].policy, env, n_members=M,
                                   max_episode_length=40 if head == 'categorical' else 20,
                                   seed=5)
    seen, step = {}, pop._natural_step
    pop._natural_step = lambda ctxs: (seen.update(ctxs=ctxs), step(ctxs))[1]
    np.random.seed(7)
    for itr in range(2):
        batches = sampler.obtain_samples(itr, 160, pop.member_params)
        pop.train_once(itr, batches)
        for m, (algo, lone, c) in enumerate(zip(pop.members, lones, seen['ctxs'])):
            cg, h = algo.last_cg, algo._policy_optimizer._hyper
            delta, k = h['max_constraint_value'], cg['accepted']
            new, prev = algo.policy.net.params, cg['prev']
            # the parameters: exactly prev - ratio^k descent, or exactly prev
            want = prev.clone()
            if k >= 0:
                want += torch.tensor(-(h['backtrack_ratio'] ** k),
                                     dtype=torch.float32) * cg['descent_step']
            assert torch.equal(new.view(torch.int32), want.view(torch.int32)), (itr, m)
            # loss and KL at the new parameters, by the lone entry points, satisfy
            # the acceptance rule (to the bars tests/test_trpo_gpu.py holds the line
            # search's losses and constraints to: 1e-6 and 1e-4 relative + 1e-7)
            if k >= 0:
                loss0, mean_old, _ = algo._policy_loss_pass(
                    c.batch, c.adv, c.old_ll, c.S, None, params=prev)
                mean_old, loss0 = mean_old.clone(), float(loss0.item())
                loss1, mean_new, _ = algo._policy_loss_pass(c.batch, c.adv, c.old_ll,
                                                            c.S, None)
                s_old = algo._clamped(prev) if head == 'gaussian' else 0.0
                s_new = algo._clamped(new) if head == 'gaussian' else 0.0
                kl = float(algo._kl_sum(mean_old, s_old, mean_new, s_new,
                                        c.S).item()) / c.S
                assert float(loss1.item()) < loss0 + 1e-6, (itr, m)
                assert kl <= delta * (1 + 1e-4) + 1e-7, (itr, m)
            # descent_step against a lone TRPO on the same batch from the same
            # parameters (the bars of the recurrence's own test)
            lone.policy.net.params.copy_(prev)
            lone.policy.net._workspace(c.S)
            lone._train_policy(c.batch, c.adv, c.old_ll, None)
            want = lone.last_cg['descent_step']
            scale = float(want.abs().max())
            assert float((cg['descent_step'] - want).abs().max()) <= 1e-3 * scale, (itr, m)


@pytest.mark.parametrize('what,kw', [
    ('PopulationTRPO trains TRPO objects', dict(member_type='PPO')),
    ('differs from member 0 in cg_iters', dict(cg_iters=(10, 10, 5))),
    ('differs from member 0 in max_backtracks', dict(max_backtracks=(15, 10, 15))),
    ('differs from member 0 in accept_violation',
     dict(accept_violation=(False, False, True))),
    ('is unsupported', dict(hidden=(128, 128))),
])
def test_refusals(what, kw):
    from garage_amd.algos import PopulationTRPO
    _, learners = _make('gaussian', **kw)
    with pytest.raises(ValueError, match=what):
        PopulationTRPO(learners)
