"""``garage_amd.baselines.LinearFeatureBaselinePopulation`` against lone
``LinearFeatureBaseline`` objects on the same batches: the coefficients with
``np.array_equal``, the values with ``torch.equal`` -- the joint launches share
the lone kernels' bodies and each member's summation order, and the host solve is
the lone one, so nothing may differ by a bit."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# three uneven members of obs_dim 4: one workgroup, three (one episode across the
# slabs), and a single step
LENGTHS = ([40, 7, 100], [4500, 3], [1])
OBS_DIM = 4
REG = (1e-5, 1e-2, 3.0)


class World:
    def __init__(self):
        from garage_amd._dtypes import Box, DeviceEpisodeBatch, EnvSpec
        dev = self.dev = torch.device('cuda:0')
        self.spec = EnvSpec(Box(-np.inf, np.inf, (OBS_DIM, )),
                            Box(-np.inf, np.inf, (1, )), max_episode_length=4500)
        self.batches, self.returns = [], []
        for m, lengths in enumerate(LENGTHS):
            rng = np.random.RandomState(300 + m)
            S = sum(lengths)
            obs = rng.uniform(-3, 3, size=(S, OBS_DIM)).astype(np.float32)
            obs[rng.uniform(size=obs.shape) < 0.02] *= 5.0
            ramp = np.concatenate([100.0 * np.arange(n, 0, -1) / n
                                   for n in lengths])
            ret = (30.0 * rng.standard_normal(S) + ramp).astype(np.float32)
            off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            n = len(lengths)
            self.batches.append(DeviceEpisodeBatch(
                self.spec, lengths=lengths,
                obs_dev=torch.from_numpy(obs).to(dev),
                last_obs_dev=torch.zeros(n, OBS_DIM, device=dev),
                actions_dev=torch.zeros(S, 4, device=dev),
                rewards_dev=torch.zeros(S, device=dev),
                step_types_dev=torch.zeros(S, dtype=torch.uint8, device=dev),
                ep_off_dev=torch.from_numpy(off).to(dev)))
            self.returns.append(torch.from_numpy(ret).to(dev))
        # a second set of returns: a second fit moves the coefficients
        self.returns2 = [r * 0.5 + 1.0 for r in self.returns]

    def population(self, reg=REG):
        from garage_amd.baselines import LinearFeatureBaselinePopulation
        return LinearFeatureBaselinePopulation(self.spec, len(LENGTHS),
                                               reg_coeff=reg)

    def lones(self, reg=REG):
        from garage_amd.baselines import LinearFeatureBaseline
        return [LinearFeatureBaseline(self.spec, reg_coeff=r) for r in reg]


@pytest.fixture(scope='module')
def world():
    return World()


def _same_values(got, want):
    assert len(got) == len(want)
    for m, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape == (sum(LENGTHS[m]), 1), m
        assert x.dtype == torch.float32 and torch.equal(x, y), m


def test_joint_fit_and_predict_equal_lone_objects(world):
    w = world
    pop, lones = w.population(), w.lones()
    for returns in (w.returns, w.returns2):
        pop.fit_batches(w.batches, returns)
        for lone, batch, ret in zip(lones, w.batches, returns):
            lone.fit_batch(batch, ret)
        for m, (member, lone) in enumerate(zip(pop, lones)):
            got, want = member.get_param_values(), lone.get_param_values()
            assert got.dtype == np.float64 and got.shape == (2 * OBS_DIM + 4, )
            assert np.array_equal(got, want), m
        _same_values(pop.predict_batches(w.batches),
                     [l.predict_batch(b) for l, b in zip(lones, w.batches)])
        # a member on its own predicts the same, from the population's row
        for m, member in enumerate(pop):
            assert torch.equal(member.predict_batch(w.batches[m]),
                               lones[m].predict_batch(w.batches[m]))
            assert member._coeffs_dev.data_ptr() == pop.coeffs_dev[m].data_ptr()
        rows = pop.coeffs_dev.cpu().numpy()
        assert rows.shape == (3, 2 * OBS_DIM + 4)
        assert np.array_equal(rows, np.stack(pop.get_param_values()))
    # the members' reg_coeffs differ, and so do their fits from an equal one's
    same = w.population(reg=(1e-5, 1e-5, 1e-5))
    same.fit_batches(w.batches, w.returns2)
    assert np.array_equal(same[0].get_param_values(), pop[0].get_param_values())
    assert not np.array_equal(same[1].get_param_values(),
                              pop[1].get_param_values())


def test_predict_before_any_fit_is_zeros(world):
    w = world
    pop = w.population()
    values = pop.predict_batches(w.batches)
    for m, v in enumerate(values):
        assert v.shape == (sum(LENGTHS[m]), 1) and v.dtype == torch.float32
        assert not bool(v.any())
    # one member fitted on its own: its row counts, the others stay zeros
    lone = w.lones()[1]
    lone.fit_batch(w.batches[1], w.returns[1])
    pop[1].fit_batch(w.batches[1], w.returns[1])
    assert np.array_equal(pop[1].get_param_values(), lone.get_param_values())
    values = pop.predict_batches(w.batches)
    assert not bool(values[0].any()) and not bool(values[2].any())
    assert torch.equal(values[1], lone.predict_batch(w.batches[1]))


def test_a_member_set_between_fits(world):
    w = world
    pop, lones = w.population(), w.lones()
    pop.fit_batches(w.batches, w.returns)
    for lone, batch, ret in zip(lones, w.batches, w.returns):
        lone.fit_batch(batch, ret)
    new = np.linspace(-1.0, 1.0, 2 * OBS_DIM + 4)
    pop[0].set_param_values(new)
    lones[0].set_param_values(new)
    pop[2].set_param_values(None)
    lones[2].set_param_values(None)
    _same_values(pop.predict_batches(w.batches),
                 [l.predict_batch(b) for l, b in zip(lones, w.batches)])
    assert np.array_equal(pop.coeffs_dev[0].cpu().numpy(), new)
    # the next joint fit overwrites both
    pop.fit_batches(w.batches, w.returns2)
    for lone, batch, ret in zip(lones, w.batches, w.returns2):
        lone.fit_batch(batch, ret)
    for member, lone in zip(pop, lones):
        assert np.array_equal(member.get_param_values(),
                              lone.get_param_values())
    _same_values(pop.predict_batches(w.batches),
                 [l.predict_batch(b) for l, b in zip(lones, w.batches)])


def test_begin_twice_cancel_and_wrong_counts(world):
    w = world
    pop = w.population()
    whole = w.population()
    whole.fit_batches(w.batches, w.returns)
    with pytest.raises(RuntimeError) as e:
        pop.finish_fit()
    assert 'finish_fit without begin_fit' in str(e.value)
    pop.begin_fit(w.batches, w.returns)
    assert pop.get_param_values() == [None, None, None]  # nothing solved yet
    with pytest.raises(RuntimeError) as e:
        pop.begin_fit(w.batches, w.returns)
    assert 'begin_fit twice' in str(e.value)
    pop.cancel_fit()
    assert pop.get_param_values() == [None, None, None]
    with pytest.raises(RuntimeError):
        pop.finish_fit()
    pop.begin_fit(w.batches, w.returns)  # a cancelled fit is no obstacle
    other = torch.ones(1024, device=w.dev).sum()  # work in between
    pop.finish_fit()
    assert float(other) == 1024.0
    for member, want in zip(pop, whole):
        assert np.array_equal(member.get_param_values(),
                              want.get_param_values())
    with pytest.raises(ValueError) as e:
        pop.begin_fit(w.batches[:2], w.returns[:2])
    assert '2 batches for 3 members' in str(e.value)
    with pytest.raises(ValueError) as e:
        pop.predict_batches(w.batches + w.batches[:1])
    assert '4 batches for 3 members' in str(e.value)
    with pytest.raises(ValueError) as e:
        pop.begin_fit(w.batches, [w.returns[0], w.returns[1][:-1], w.returns[2]])
    assert 'member 1' in str(e.value) and 'returns' in str(e.value)
    assert pop._pending is None
    # a member with a fit of its own begun
    pop[2].begin_fit(w.batches[2], w.returns[2])
    with pytest.raises(RuntimeError) as e:
        pop.begin_fit(w.batches, w.returns)
    assert 'member 2' in str(e.value)
    pop[2].finish_fit()


def test_pickle_round_trip(world):
    w = world
    pop = w.population()
    pop.fit_batches(w.batches, w.returns)
    want = pop.predict_batches(w.batches)
    again = pickle.loads(pickle.dumps(pop))
    assert again.coeffs_dev is None  # device scratch is rebuilt
    assert [b._reg_coeff for b in again] == list(REG)
    for a, b in zip(pop, again):
        assert np.array_equal(a.get_param_values(), b.get_param_values())
    _same_values(again.predict_batches(w.batches), want)
    assert again.coeffs_dev.data_ptr() != pop.coeffs_dev.data_ptr()
    # and it goes on fitting to the same bits
    pop.fit_batches(w.batches, w.returns2)
    again.fit_batches(w.batches, w.returns2)
    for a, b in zip(pop, again):
        assert np.array_equal(a.get_param_values(), b.get_param_values())
