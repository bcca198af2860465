"""The narrow step for hidden nonlinearities other than tanh, with the reference and
bars of ``test_loss_paths_fp64_gpu.py`` (imported); a relu ``PopulationPPO`` against lone
``PPO``s.  Largest error measured: 0.163 of its bar (narrow), 0.062 (per layer)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _loss_path_cases as pc
import _mlp_option_cases as oc
import test_loss_paths_fp64_gpu as lp
import test_population_update_gpu as pu
from test_loss_paths_fp64_gpu import dev  # noqa: F401  (fixture)
from test_population_update_gpu import narrow_path  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ACTS = ('relu', 'none', 'sigmoid', 'elu', 'leaky_relu', 'softplus')
KINK_MARGIN = 1e-3  # relu, elu, leaky_relu: no fp64 pre-activation nearer to the kink
# Seeds of the 65-row cases at which the fp64 reference satisfies that (found on the CPU),
# H = 32: (5, cat), (5, gauss), (39, cat), (39, gauss), then H = 64; the rest pass at 0.
KINK_SEEDS = {'relu': (32, 8, 244, 18, 405, 591, 1649, 2722),
              'elu': (13, 87, 9, 43, 1980, 5752, 2874, 1748),
              'leaky_relu': (36, 123, 60, 52, 3517, 1540, 3473, 3333)}


class _Seeded(pc.P):  # (_Problem seeds its draws with the case's repr)
    seed = 0

    def __repr__(self):
        return '%s seed %d' % (super().__repr__(), self.seed)


class _ActProblem(lp._Problem):
    """``_Problem`` with the hidden nonlinearity ``act`` in network and reference."""

    def __init__(self, dev, act, H, in_w, M, kind):
        p = _Seeded(*pc._p((in_w, H, H, 8 if kind == 'gauss' else 3), M, kind))
        if act in KINK_SEEDS and M == 65:
            p.seed = KINK_SEEDS[act][4 * (H == 64) + 2 * (in_w == 39) + (kind == 'gauss')]
        self.act = act
        with self._oracle():
            super().__init__(p, dev, lp.ADAM)
        for mod in (self.algo.policy, self.algo._value_function):
            mod.net.hidden_act = act
            mod.net._desc.hidden_act = mod.net.HIDDEN_ACTS[act]
        if act in KINK_SEEDS:
            params, x = self.params64(self.p0), self.X.double()
            for l in range(2):
                base = '%s_mean_module._layers.%d.linear.' % (lp.PREFIX, l)
                z = x @ params[base + 'weight'].T + params[base + 'bias']
                assert float(z.abs().min()) > KINK_MARGIN
                x = oc.TORCH_ACT[act](z)

    def _oracle(self):
        from oracle import networks as nets
        return nets.hidden_nonlinearity(*2 * [oc.TORCH_ACT[self.act]])

    def reference(self, flat, rows=None):
        with self._oracle():
            return super().reference(flat, rows)

    def check(self, lib, acts_on, narrow_launches):
        from garage_amd import engine
        ref_loss, ref = self.reference(self.p0)
        lp._switches(lib)
        was = engine.set_narrow_activations(acts_on)
        try:
            self.reset()
            before = lp._counts(lib)
            loss, flat = self.gradient_step()
            after = lp._counts(lib)
        finally:
            engine.set_narrow_activations(was)
        assert tuple(a - b for a, b in zip(after, before)) == (0, narrow_launches, 0)
        failures = []
        lp._compare(self, self.act, loss, flat, ref_loss, ref, failures)
        assert not failures, failures


@pytest.mark.parametrize('kind', ['gauss', 'cat'])
@pytest.mark.parametrize('M', [1, 65])
@pytest.mark.parametrize('in_w', [5, 39])
@pytest.mark.parametrize('H', [32, 64])
@pytest.mark.parametrize('act', ACTS)
def test_narrow_step_gradient_against_fp64(dev, act, H, in_w, M, kind):
    from garage_amd import _lib
    lib = _lib.load()
    wide = lib.ga_narrow_wide_launches()
    _ActProblem(dev, act, H, in_w, M, kind).check(lib, True, 1)
    assert lib.ga_narrow_wide_launches() - wide == (in_w > 32)


@pytest.mark.parametrize('in_w', [5, 39])
def test_switch_off_takes_the_per_layer_kernels(dev, in_w):
    from garage_amd import _lib
    lib = _lib.load()
    prob = _ActProblem(dev, 'relu', 64, in_w, 65, 'gauss')
    assert lib.ga_narrow_acts_on() == 0
    assert lib.ga_update_members_supported(C.byref(prob.net._desc)) == 0
    prob.check(lib, False, 0)


def test_population_of_relu_members_equals_lone_ppos_bit_for_bit(narrow_path, monkeypatch):
    from functools import partial
    from garage_amd import _lib, policies
    lib = narrow_path
    for name in ('CategoricalMLPPolicy', 'GaussianMLPValueFunction'):  # relu members
        monkeypatch.setattr(policies, name, partial(getattr(policies, name),
                                                    hidden_nonlinearity=torch.relu))
    with pytest.raises(ValueError, match='unsupported'):  # the flag is off
        pu._population('categorical', 'device')
    monkeypatch.setattr(_lib, 'NARROW_ACTS', True)  # (set_narrow_activations(True))
    pop, sampler = pu._population('categorical', 'device')
    _, lones = pu._make_members('categorical', 'device')
    assert len(lones) == 3 and lones[0].policy.net.hidden_act == 'relu'
    np.random.seed(7)
    joint = lib.ga_launch_count(pu.GA_PROF_MEMBERS_STEP)
    batch = sampler.obtain_samples(0, 64, pop.member_params)
    pop.train_once(0, batch)
    assert lib.ga_launch_count(pu.GA_PROF_MEMBERS_STEP) - joint >= 4  # 2 nets x 2 epochs
    np.random.seed(7)
    for m, (member, lone) in enumerate(zip(pop.members, lones)):
        before = lib.ga_launch_count(pu.GA_PROF_NARROW_STEP)
        lone._train_once(0, batch[m])
        assert lib.ga_launch_count(pu.GA_PROF_NARROW_STEP) - before >= 4
        for x, y in zip(pu._network_state(member), pu._network_state(lone)):
            assert torch.equal(pu._bits(x), pu._bits(y)), m
        assert member.last_tabular == lone.last_tabular, m
