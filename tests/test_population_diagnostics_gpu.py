"""``PopulationPPO(joint_diagnostics=True)``: every member's diagnostics after the
update in joint launches (``ga_*_members_f32``) leave every member, bit for bit, as
the default path -- one ``VPG._after_train`` per member -- leaves it.

Two identically seeded populations, one per path, run three iterations through
``GpuPopulationSampler(joint_pack=True)`` + ``train_once``; after every iteration
everything an iteration leaves behind is compared with ``==`` / ``array_equal``.
The shapes are the smallest that reach every branch: three members of 16 envs,
ragged episodes (padded cells, different sample counts per member), batches on
both sides of one 256-row block, both head kinds, MLP and linear value functions,
PPO and VPG, the softplus / clamped std.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 3
N_KINDS = 16  # GaProfKind (prof.h)

# name -> (env, horizon, samples per member, head, hidden, algo, value function)
CONFIGS = {
    'categorical-ragged': ('cartpole', 30, 16 * 24, 'categorical', 32, 'PPO', 'mlp'),
    'categorical-one-block': ('cartpole', 30, 16 * 8, 'categorical', 32, 'PPO', 'mlp'),
    'gaussian-terminations': ('double_pendulum', 7, 16 * 21, 'gaussian', 32, 'PPO',
                              'mlp'),
    'gaussian-linear': ('double_pendulum', 20, 16 * 20, 'gaussian', 64, 'PPO',
                        'linear'),
    'vpg-softplus-max-entropy': ('pendulum', 20, 16 * 20, 'gaussian', 64, 'VPG',
                                 'mlp'),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _population(name, joint, members=M):
    """(population, sampler, samples per member) of configuration ``name``; the
    same seeds whatever ``joint`` is."""
    from garage_amd import algos, envs
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy, GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    from garage_amd.sampler import GpuPopulationSampler
    env_name, horizon, n_samples, head, hidden, algo, vf_kind = CONFIGS[name]
    env_cls = {'cartpole': envs.CartPoleVecEnv, 'pendulum': envs.PendulumVecEnv,
               'double_pendulum': envs.DoublePendulumVecEnv}[env_name]
    env = env_cls(members * 16, max_episode_length=horizon, seed=3)
    hs = (hidden, hidden)
    baselines = None
    if vf_kind == 'linear':
        baselines = list(LinearFeatureBaselinePopulation(
            env.spec, members, reg_coeff=[1e-5 * (m + 1) for m in range(members)]))
    learners = []
    for m in range(members):
        torch.manual_seed(10 + m)
        if head == 'categorical':
            pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hs)
        elif algo == 'VPG':
            pol = GaussianMLPPolicy(env.spec, hidden_sizes=hs, min_std=0.3,
                                    std_parameterization='softplus')
        else:
            pol = GaussianMLPPolicy(env.spec, hidden_sizes=hs)
        lr = (torch.optim.Adam, dict(lr=1e-3 * (m + 1)))
        kw = dict(policy_optimizer=OptimizerWrapper(lr, pol, 2, 64, seed=m))
        if baselines is None:
            vf = GaussianMLPValueFunction(env.spec, hidden_sizes=hs)
            kw['vf_optimizer'] = OptimizerWrapper(lr, vf, 2, 64, seed=100 + m)
        else:
            vf = baselines[m]
        if algo == 'PPO':
            kw.update(lr_clip_range=0.1 + 0.05 * m, entropy_method='regularized',
                      policy_ent_coeff=0.01 * (m + 1))
        else:
            kw.update(entropy_method='max', stop_entropy_gradient=True,
                      center_adv=False, policy_ent_coeff=0.01 * (m + 1))
        learners.append(getattr(algos, algo)(
            env_spec=env.spec, policy=pol, value_function=vf, sampler=None, **kw))
    pop = algos.PopulationPPO(learners, joint_diagnostics=joint)
    sampler = GpuPopulationSampler(learners[0].policy, env, n_members=members,
                                   max_episode_length=horizon, seed=5,
                                   joint_pack=True)
    return pop, sampler, n_samples


def _snapshot(algo, records, m):
    nets = [algo.policy.net]
    if getattr(algo._value_function, 'net', None) is not None:
        nets.append(algo._value_function.net)
    prefix = 'member{}/'.format(m)
    return dict(
        tabular=dict(algo.last_tabular), performance=dict(algo.last_performance),
        tensors={k: (v.clone() if torch.is_tensor(v) else v)
                 for k, v in algo.last_tensors.items()},
        state=[t.clone() for net in nets
               for t in (net.params, net.exp_avg, net.exp_avg_sq)],
        adam_steps=[net.adam_steps for net in nets],
        old_policy=algo._old_policy.params.clone(),
        records=[(k, v) for k, v in records if k.startswith(prefix)])


def _run(name, joint):
    """Per iteration: (the members' snapshots, the returned mean returns, facts of
    the batches)."""
    from garage_amd import logger
    pop, sampler, n_samples = _population(name, joint)
    assert pop._joint_diagnostics == joint
    np.random.seed(7)
    out = []
    for itr in range(3):
        batches = sampler.obtain_samples(itr, n_samples, pop.member_params)
        logger.tabular.clear()
        returns = pop.train_once(itr, batches)
        records = list(logger.tabular.as_dict.items())  # (insertion order)
        facts = [(b.n_samples, len(b.lengths),
                  int(max(a.max_episode_length, max(b.lengths))) * len(b.lengths)
                  - b.n_samples) for a, b in zip(pop.members, batches)]
        out.append(([_snapshot(a, records, m) for m, a in enumerate(pop.members)],
                    [float(r) for r in returns], facts))
    return out


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_joint_diagnostics_leave_every_member_as_the_default_path_does(name):
    joint, default = _run(name, True), _run(name, False)
    for itr, ((got, got_r, facts), (want, want_r, facts_d)) in enumerate(
            zip(joint, default)):
        assert facts == facts_d  # the same batches
        assert got_r == want_r, itr
        for m, (g, w) in enumerate(zip(got, want)):
            where = (name, itr, m)
            assert g['tabular'] == w['tabular'], where
            assert len(w['tabular']) == 9
            assert g['performance'] == w['performance'], where
            assert sorted(g['tensors']) == sorted(w['tensors'])
            for k, v in w['tensors'].items():
                if torch.is_tensor(v):
                    assert torch.equal(_bits(g['tensors'][k]), _bits(v)), (where, k)
                else:
                    assert g['tensors'][k] == v, (where, k)
            for x, y in zip(g['state'], w['state']):
                assert torch.equal(_bits(x), _bits(y)), where
            assert g['adam_steps'] == w['adam_steps'], where
            assert torch.equal(_bits(g['old_policy']), _bits(w['old_policy'])), where
            # every record under member<m>/, in the default path's order
            assert g['records'] == w['records'], where
            assert len(w['records']) >= 9 + 8
            assert all(np.isfinite(v) for v in w['tabular'].values()), where
    # what the configuration is there to reach
    samples = [f[0] for f in joint[0][2]]
    pads = [f[2] for _, _, fs in joint for f in fs]
    if name == 'categorical-ragged':
        assert len(set(samples)) > 1 and max(samples) > 256 and max(pads) > 0
    elif name == 'categorical-one-block':
        assert max(samples) <= 256
    elif name == 'gaussian-terminations':
        assert max(pads) > 0 and max(samples) > 256
    elif name == 'vpg-softplus-max-entropy':
        assert max(pads) == 0
    # the members' scalars differ from each other: a table that handed member 0's
    # struct to everyone would have failed above
    last = [g['tabular'] for g in joint[-1][0]]
    for key in ('policy/LossAfter', 'policy/KL', 'vf/LossAfter'):
        assert len({t[key] for t in last}) == M, key
    perf = [g['performance']['AverageReturn'] for g in joint[-1][0]]
    assert len(set(perf)) > 1


def _launches(lib):
    return sum(int(lib.ga_launch_count(k)) for k in range(N_KINDS))


def _after_train_launches(joint, members):
    from garage_amd import _lib
    lib = _lib.load()
    pop, sampler, n_samples = _population('categorical-ragged', joint, members)
    np.random.seed(7)
    batches = sampler.obtain_samples(0, n_samples, pop.member_params)
    ctxs = pop._before_trains(batches)
    pop._train(ctxs)
    before = _launches(lib)
    pop._after_trains(0, ctxs)
    return _launches(lib) - before


def test_joint_launch_count_does_not_grow_with_the_member_count():
    """The launches the library COUNTS of one ``_after_trains`` call:
    ``ga_launch_count`` sees the layer products (GEMM and streaming forward
    kernels, lone or members) and nothing else.  The loss, KL, finalize and episode
    launches of the joint path carry no counter; that their number does not depend
    on the member count is the host harness's check (one launch per table,
    ``make asan-members-diag``)."""
    joint = [_after_train_launches(True, n) for n in (2, 5)]
    default = [_after_train_launches(False, n) for n in (2, 5)]
    assert joint[0] == joint[1] > 0
    assert default[1] > default[0] > joint[0]
    # (a member more costs at least a policy and a value forward of three layers)
    assert default[1] - default[0] >= 3 * 6


def _fault(joint):
    from garage_amd.engine import reduction_workspace
    pop, sampler, n_samples = _population('categorical-one-block', joint)
    np.random.seed(7)
    batches = sampler.obtain_samples(0, n_samples, pop.member_params)
    ctxs = pop._before_trains(batches)
    pop._train(ctxs)
    nets = [n for a in pop.members for n in (a.policy.net, a._value_function.net)]
    moved = [n.adam_steps for n in nets]
    dev = pop.members[0].policy.device
    # the word small_step.hip raises when a barrier gave up, set by hand: no
    # kernel faults here
    reduction_workspace(dev, 1)[-1] = 1.0
    with pytest.raises(RuntimeError) as err:
        pop._after_trains(0, ctxs)
    return pop, ctxs, nets, moved, str(err.value)


def test_a_raised_fault_word_restores_every_members_adam_steps():
    from garage_amd.engine import reduction_workspace
    texts = []
    for joint in (True, False):
        pop, ctxs, nets, moved, text = _fault(joint)
        dev = pop.members[0].policy.device
        texts.append(text)
        assert 'ga_small_step: a grid barrier timed out' in text and '[1]' in text
        # re-armed
        for tag in (0, 1):
            assert float(reduction_workspace(dev, tag)[-2:].abs().sum()) == 0.0
        restored = [n.adam_steps for n in nets]
        want = [s for c in ctxs for s in c.steps_before]
        if joint:  # every member's, not only the first one's
            assert restored == want
            assert all(a > b for a, b in zip(moved, restored))
        else:      # (the default path stops at the member that reads the word)
            assert restored[:2] == want[:2]
    assert texts[0] == texts[1]


def test_an_old_pickle_takes_the_default_path():
    import pickle
    pop, _, _ = _population('categorical-one-block', True)
    state = pop.__getstate__()
    assert '_old_rows' not in state
    del state['_joint_diagnostics']
    old = pop.__class__.__new__(pop.__class__)
    old.__setstate__(pickle.loads(pickle.dumps(state)))
    assert old._joint_diagnostics is False
    copy = pickle.loads(pickle.dumps(pop))
    assert copy._joint_diagnostics is True
    for m, a in enumerate(copy.members):
        assert a._old_policy.params.data_ptr() == copy._old_rows[m].data_ptr()


def test_a_switch_that_takes_the_forward_elsewhere_is_refused_before_the_update():
    """``ga_set_fused_forward(1)`` sends the members' networks to a kernel without a
    members twin: the constructor says so, and an iteration says so before anything
    of it has run."""
    from garage_amd import _lib
    lib = _lib.load()
    pop, sampler, n_samples = _population('categorical-one-block', True)
    batches = sampler.obtain_samples(0, n_samples, pop.member_params)
    lib.ga_set_fused_forward(1)
    try:
        with pytest.raises(ValueError, match='joint_diagnostics'):
            _population('categorical-one-block', True)
        _population('categorical-one-block', False)  # the default path is not concerned
        with pytest.raises(RuntimeError, match='ga_set_fused_forward'):
            pop.train_once(0, batches)
        assert all(a.policy.net.adam_steps == 0 for a in pop.members)
    finally:
        lib.ga_set_fused_forward(0)
    pop.train_once(0, batches)
    assert all(a.policy.net.adam_steps > 0 for a in pop.members)
