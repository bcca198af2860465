"""What ``garage_amd.baselines.LinearFeatureBaselinePopulation`` and
``PopulationPPO`` with linear baselines do without a device: constructor checks,
``set_param_values`` shapes, pickling of unfitted and set populations, the
algorithm's refusals, the ctypes records' layout and the host harness
(``make asan-linear-baseline-members``)."""
import ctypes as C
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

from garage_amd import _lib
from garage_amd._dtypes import Box, EnvSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
SPEC = EnvSpec(Box(-1, 1, (4, )), Box(-1, 1, (2, )), max_episode_length=8)
F = 2 * 4 + 4


def _population(n=3, **kw):
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    return LinearFeatureBaselinePopulation(SPEC, n, **kw)


def test_members_are_linear_feature_baselines():
    from garage_amd.baselines import LinearFeatureBaseline
    pop = _population(3, reg_coeff=[1e-5, 1e-3, 0.5], name='base')
    assert len(pop) == 3 and pop.members == list(pop) and pop[1] is pop.members[1]
    assert pop.n_features == F
    for m, member in enumerate(pop):
        assert isinstance(member, LinearFeatureBaseline)
        assert member.kind == 'linear' and member.n_features == F
        assert member.get_param_values() is None
        assert member.name == 'base/member{}'.format(m)
    assert [b._reg_coeff for b in pop] == [1e-5, 1e-3, 0.5]
    assert [b._reg_coeff for b in _population(2, reg_coeff=0.25)] == [0.25, 0.25]
    assert pop.get_param_values() == [None, None, None]
    assert pop.coeffs_dev is None


@pytest.mark.parametrize('n', [0, -1, 1025])
def test_member_count_outside_1_to_1024_raises(n):
    with pytest.raises(ValueError) as e:
        _population(n)
    assert 'n_members' in str(e.value) and str(n) in str(e.value)


def test_wrong_reg_coeff_count_and_obs_dim_raise():
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    with pytest.raises(ValueError) as e:
        _population(3, reg_coeff=[1e-5, 1e-4])
    assert '2 reg_coeff values for 3 members' in str(e.value)
    wide = EnvSpec(Box(-1, 1, (129, )), Box(-1, 1, (1, )), max_episode_length=5)
    with pytest.raises(ValueError) as e:
        LinearFeatureBaselinePopulation(wide, 2)
    assert '129' in str(e.value)


def test_set_param_values_shapes():
    pop = _population(3)
    rows = [np.arange(F) + 0.5, None, np.ones(F, np.float32)]
    pop.set_param_values(rows)
    got = pop.get_param_values()
    assert np.array_equal(got[0], rows[0]) and got[0].dtype == np.float64
    assert got[1] is None
    assert np.array_equal(got[2], np.ones(F)) and got[2].dtype == np.float64
    # a member set on its own: the population sees it
    pop[1].set_param_values(np.full(F, 2.0))
    assert np.array_equal(pop.get_param_values()[1], np.full(F, 2.0))
    pop.set_param_values(np.zeros((3, F)))  # an (M, F) array does as well
    assert all(np.array_equal(v, np.zeros(F)) for v in pop.get_param_values())
    with pytest.raises(ValueError) as e:
        pop.set_param_values(rows[:2])
    assert '2 members for 3' in str(e.value)
    with pytest.raises(ValueError) as e:
        pop.set_param_values([np.zeros(F), np.zeros(F + 1), None])
    assert '{} coefficients for {} features'.format(F + 1, F) in str(e.value)
    with pytest.raises(ValueError):
        pop[0].set_param_values(np.zeros(3))


def test_pickle_unfitted_and_set_populations():
    pop = _population(3, reg_coeff=[1e-5, 1e-3, 0.5])
    again = pickle.loads(pickle.dumps(pop))
    assert again.get_param_values() == [None, None, None]
    assert [b._reg_coeff for b in again] == [1e-5, 1e-3, 0.5]
    pop.set_param_values([np.arange(F) * 1.5, None, -np.arange(F)])
    again = pickle.loads(pickle.dumps(pop))
    for a, b in zip(pop.get_param_values(), again.get_param_values()):
        assert (a is None and b is None) or np.array_equal(a, b)
    # the members know their population and their place in it
    for m, member in enumerate(again):
        assert member._population is again and member._index == m
    assert again._pending is None and again.coeffs_dev is None
    # a member pickled through its algorithm's reference brings the population along
    member = pickle.loads(pickle.dumps(pop[2]))
    assert np.array_equal(member.get_param_values(), -np.arange(F))
    assert member._population[2] is member


def test_misuse_without_a_device():
    pop = _population(2)
    with pytest.raises(RuntimeError) as e:
        pop.finish_fit()
    assert 'finish_fit without begin_fit' in str(e.value)
    pop.cancel_fit()  # nothing begun: nothing to forget
    with pytest.raises(ValueError) as e:
        pop.predict_batches([None])
    assert '1 batches for 2 members' in str(e.value)
    with pytest.raises(ValueError) as e:
        pop.begin_fit([None, None], [None])
    assert '1 returns for 2 members' in str(e.value)


def test_ctypes_records_mirror_the_header():
    """8 fields of 8 bytes each, in the header's order."""
    for rec, names in (
            (_lib.LinearGramMember, ['obs', 'ldo', 'ep_off', 'n_eps', 'S',
                                     'returns', 'gram', 'rhs']),
            (_lib.LinearPredictMember, ['obs', 'ldo', 'ep_off', 'n_eps', 'S',
                                        'coeffs', 'values', 'ldv'])):
        assert [f[0] for f in rec._fields_] == names
        assert C.sizeof(rec) == 64
    header = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    for name in ('ga_linear_gram_member', 'ga_linear_predict_member',
                 'ga_linear_features_gram_members_f64',
                 'ga_linear_features_predict_members_f32',
                 'ga_linear_gram_members_workspace_doubles'):
        assert name in header


def test_entries_refuse_before_anything_is_read():
    lib = _lib.load()
    BASE = 0x100000  # never read: every call below is refused first
    arr = (_lib.LinearGramMember * 2)()
    for u in arr:
        u.obs, u.ldo, u.ep_off, u.n_eps, u.S = BASE, 4, BASE, 1, 10
        u.returns, u.gram, u.rhs = BASE, BASE, BASE
    for n, obs_dim, ws, doubles, message in (
            (0, 4, BASE, 1 << 20, 'n_members'),
            (1025, 4, BASE, 1 << 20, 'n_members'),
            (2, 0, BASE, 1 << 20, 'obs_dim'),
            (2, 5, BASE, 1 << 20, 'ldo'),
            (2, 4, None, 1 << 20, 'null pointer'),
            (2, 4, BASE + 4, 1 << 20, 'aligned'),
            (2, 4, BASE, 2 * 272 - 1, 'workspace too small')):
        assert lib.ga_linear_features_gram_members_f64(arr, n, obs_dim, ws,
                                                       doubles, None) < 0
        assert message in lib.ga_last_error().decode(), message
    arr[1].n_eps = 11
    assert lib.ga_linear_features_gram_members_f64(arr, 2, 4, BASE, 1 << 20,
                                                   None) < 0
    assert 'member 1' in lib.ga_last_error().decode()
    assert lib.ga_linear_features_predict_members_f32(None, 2, 4, None) < 0
    assert 'null pointer' in lib.ga_last_error().decode()


def test_members_entries_under_address_sanitizer():
    """``make asan-linear-baseline-members``: the population's host side
    (linear_baseline_members_host.cpp) compiled with ``-fsanitize=address,undefined``
    for the CPU and run against fakes of its three launches and of the HIP calls it
    makes (tests/host/linear_baseline_members_harness.cpp)."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-linear-baseline-members'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'linear baseline members ok' in out.stdout


# -- PopulationPPO's refusals ------------------------------------------------------
def _learner(vf, cls=None, lr=1e-3, seed=0):
    from garage_amd.algos import PPO
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    pol = GaussianMLPPolicy(SPEC, hidden_sizes=(32, 32), device=CPU)
    kw = {}
    if vf is None:
        vf = GaussianMLPValueFunction(SPEC, hidden_sizes=(32, 32), device=CPU)
        kw['vf_optimizer'] = OptimizerWrapper(
            (torch.optim.Adam, dict(lr=lr)), vf, 2, 64, seed=seed + 100)
    return (cls or PPO)(
        env_spec=SPEC, policy=pol, value_function=vf, sampler=None,
        policy_optimizer=OptimizerWrapper((torch.optim.Adam, dict(lr=lr)), pol,
                                          2, 64, seed=seed), **kw)


def test_population_ppo_takes_one_population_in_member_order():
    from garage_amd.algos import PopulationPPO, VPG
    base = _population(3, reg_coeff=[1e-5, 1e-4, 1e-3])
    members = [_learner(base[m], lr=1e-3 * (m + 1), seed=m) for m in range(3)]
    pop = PopulationPPO(members)
    assert pop._baselines is base
    assert sorted(pop._rows) == ['policy']  # no 'vf' network
    for m, a in enumerate(members):
        assert a.policy.net.params.data_ptr() == pop.member_params[m].data_ptr()
    base = _population(2)
    PopulationPPO([_learner(base[m], cls=VPG) for m in range(2)])


def test_population_ppo_names_what_it_refuses_of_linear_members():
    from garage_amd.algos import PopulationPPO
    from garage_amd.baselines import LinearFeatureBaseline
    with pytest.raises(ValueError) as e:  # built on its own
        PopulationPPO([_learner(LinearFeatureBaseline(SPEC))])
    assert 'LinearFeatureBaseline' in str(e.value)
    assert 'LinearFeatureBaselinePopulation' in str(e.value)
    base, other = _population(2), _population(2)
    with pytest.raises(ValueError) as e:  # some linear, some MLP
        PopulationPPO([_learner(base[0]), _learner(None)])
    assert 'value function kind' in str(e.value)
    with pytest.raises(ValueError) as e:
        PopulationPPO([_learner(None), _learner(base[1])])
    assert 'value function kind' in str(e.value)
    with pytest.raises(ValueError) as e:  # two populations
        PopulationPPO([_learner(base[0]), _learner(other[1])])
    assert 'another LinearFeatureBaselinePopulation' in str(e.value)
    with pytest.raises(ValueError) as e:  # the wrong order
        PopulationPPO([_learner(base[1]), _learner(base[0])])
    assert 'member order' in str(e.value)
    with pytest.raises(ValueError) as e:  # one member twice
        PopulationPPO([_learner(base[0]), _learner(base[0])])
    assert 'of its own' in str(e.value)
    with pytest.raises(ValueError) as e:  # fewer learners than baselines
        PopulationPPO([_learner(_population(3)[0])])
    assert '3 members' in str(e.value)
