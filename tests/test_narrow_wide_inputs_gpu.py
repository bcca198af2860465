"""The narrow one-launch step at 33 .. 128 inputs (the wide instantiations of
``narrow_body.h``): one step against fp64 autograd of network plus objective (case
shape and tolerance rule of ``test_loss_paths_fp64_gpu.py``, whose absolute bounds do
not depend on the first layer's sum length), a ``PopulationPPO`` against lone ``PPO``
learners bit for bit, and the boundaries of the range by launch counter."""
import numpy as np
import pytest
import torch

from _loss_path_cases import _p, case_id
from test_loss_paths_fp64_gpu import ADAM, _Problem, _compare, _switches

pytestmark = pytest.mark.gpu

NARROW_STEP = 11  # GA_PROF_NARROW_STEP of csrc/prof.h: whichever instantiation
# (case, observation rows round4(in_w) + 8 floats apart); 'g': gathered row ids
WIDE = [
    (_p((33, 32, 32, 1), 1, 'gauss'), False),
    (_p((36, 64, 64, 6), 63, 'gauss', vpg=True, std='lo_active'), True),
    (_p((63, 32, 32, 3), 64, 'cat', dsm=1), False),
    (_p((64, 64, 64, 6), '65g', 'gauss', ent='reg_sp', std='sp_free'), True),
    (_p((65, 32, 32, 1), '129g', 'nll'), False),
    (_p((100, 64, 64, 3), 129, 'cat', dsm=0, ent='max_stop'), True),
    (_p((128, 64, 64, 6), '129g', 'gauss'), True),
    (_p((128, 32, 32, 1), 65, 'gauss', std='hi_active', learn_std=False), False),
    (_p((100, 32, 32, 6), '63g', 'gauss'), False),
]


def _lib_dev():
    from garage_amd import _lib
    from garage_amd.engine import require_gpu
    return _lib.load(), require_gpu()


def _step(lib, prob):
    """One gradient step -> (loss, flat gradient, launches of [the narrow step, its
    wide instantiations])."""
    def counts():
        return [int(lib.ga_launch_count(NARROW_STEP)), int(lib.ga_narrow_wide_launches())]
    prob.reset()
    before = counts()
    loss, flat = prob.gradient_step()
    return loss, flat, [a - b for a, b in zip(counts(), before)]


@pytest.mark.parametrize('p,far_rows', WIDE, ids=lambda v: case_id(v) if isinstance(
    v, tuple) else 'ld+%d' % (8 * v))
def test_wide_narrow_step_against_fp64(p, far_rows):
    from garage_amd.engine import pad_rows
    lib, dev = _lib_dev()
    prob = _Problem(p, dev, ADAM)
    if far_rows:
        prob.batch.obs_dev = pad_rows(prob.X, width=p.dims[0] + 8)
    ref_loss, ref = prob.reference(prob.p0)
    failures = []
    _switches(lib)
    loss, flat, took = _step(lib, prob)
    assert took == [1, 1]
    _compare(prob, 'narrow wide', loss, flat, ref_loss, ref, failures)
    assert not failures, failures


STEPS, ENVS = 5, (13, 26, 12)  # 65 rows (64 + a last step of ONE row), 130, 60 (no step 1)


def _learners(n, in_w, H):
    """[(PPO, its sampler)]: Gaussian MLP(H, H) learners on ``in_w``-wide observations,
    two epochs of 64-row minibatches, own learning rate, clip range and seeds."""
    from garage_amd.algos import PPO
    from garage_amd.envs import SyntheticVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    out = []
    for m in range(n):
        env = SyntheticVecEnv(ENVS[m], in_w, 2, STEPS, seed=3 + m)
        torch.manual_seed(10 + m)
        pol = GaussianMLPPolicy(env.spec, hidden_sizes=(H, H))
        vf = GaussianMLPValueFunction(env.spec, hidden_sizes=(H, H))
        opt = (torch.optim.Adam, dict(lr=1e-3 * (m + 1)))
        algo = PPO(env_spec=env.spec, policy=pol, value_function=vf, sampler=None,
                   policy_optimizer=OptimizerWrapper(opt, pol, 2, 64, 'device', m),
                   vf_optimizer=OptimizerWrapper(opt, vf, 2, 64, 'device', 100 + m),
                   lr_clip_range=0.1 + 0.05 * m)
        out.append((algo, GpuVecSampler(pol, env, max_episode_length=STEPS, n_workers=1,
                                        worker_class=GpuVecWorker,
                                        worker_args=dict(n_envs=ENVS[m]))))
    return out


def _state(algo):
    return [getattr(mod.net, name).clone() for mod in (algo.policy, algo._value_function)
            for name in ('params', 'exp_avg', 'exp_avg_sq')]


@pytest.mark.parametrize('H', [32, 64])
@pytest.mark.parametrize('in_w', [33, 64, 128])
@pytest.mark.parametrize('n', [1, 3])
def test_population_ppo_equals_lone_ppos_bit_for_bit(n, in_w, H):
    from garage_amd.algos import PopulationPPO
    lib, _ = _lib_dev()
    lones = _learners(n, in_w, H)
    batches = [s.obtain_samples(0, ENVS[m] * STEPS, a.policy.get_param_values())
               for m, (a, s) in enumerate(lones)]
    assert [int(sum(b.lengths)) for b in batches] == [e * STEPS for e in ENVS[:n]]
    pop = PopulationPPO([a for a, _ in _learners(n, in_w, H)])
    before = int(lib.ga_narrow_wide_launches())
    pop.train_once(0, batches)
    # two networks x two epochs x the steps of the longest member, all wide
    assert int(lib.ga_narrow_wide_launches()) - before == 4 * (3 if n == 3 else 2)
    for m, (lone, _) in enumerate(lones):
        start = _state(lone)
        lone._train_once(0, batches[m])
        for x, y, x0 in zip(_state(pop.members[m]), _state(lone), start):
            assert bool(torch.isfinite(y).all()) and not torch.equal(y, x0)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), m


@pytest.mark.parametrize('in_w,wide_on,want', [
    (32, 1, [1, 0]),   # the overlay instantiation, as before
    (128, 1, [1, 1]),
    (129, 1, [0, 0]),  # the per-layer launches, as before
    (64, 0, [0, 0]),   # _lib.NARROW_WIDE off: what GARAGE_AMD_NARROW_WIDE=0 gives
])
def test_which_step_a_lone_learner_takes(in_w, wide_on, want, monkeypatch):
    from garage_amd import _lib
    lib, dev = _lib_dev()
    prob = _Problem(_p((in_w, 64, 64, 6), 65, 'gauss'), dev, ADAM)
    _switches(lib)
    monkeypatch.setattr(_lib, 'NARROW_WIDE', bool(wide_on))
    loss, flat, took = _step(lib, prob)
    # the library's own setting is back to off: opt-in at the C ABI
    assert took == want and np.isfinite(loss) and lib.ga_set_narrow_wide(0) == 0


@pytest.mark.parametrize('in_w,kw,text', [
    (129, {}, '<= 128 inputs'),
    (64, {'joint_diagnostics': True}, 'joint_diagnostics'),
    (64, {'joint_before': True}, 'joint_before'),
])
def test_population_refusals_name_the_limit_or_the_switch(in_w, kw, text):
    from garage_amd.algos import PopulationPPO
    with pytest.raises(ValueError, match=text):
        PopulationPPO([a for a, _ in _learners(1, in_w, 64)], **kw)
