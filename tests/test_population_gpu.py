"""A population of policies behind one rollout launch
(``ga_policy_env_step_members_f32``, ``GpuPopulationSampler``) and CEM on it.

Every member's batch must be, bit for bit in every array, the batch a lone
``GpuVecWorker`` of the member's ``g`` envs returns with the member's
parameters, the same seed and worker number and an env batch built with
``env_id0 = m * g`` -- for each kernel shape (resident ``L == 3`` / ``L == 2``,
``GEN`` resident, streamed at ``WIDTH = 512``), with one workgroup per member
(M = 3, g = 16: a non-power-of-two population, the last member) and with two
(M = 2, g = 32: the division by the workgroups per member).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT = 13
SEED = 5
SIZES = [(3, 16), (2, 32)]


def _bits(x):
    x = np.ascontiguousarray(x)
    if x.dtype == object:
        return np.asarray([int(v) for v in x.reshape(-1)])
    return x.view(np.uint8) if x.dtype.kind == 'f' else x


# -- the cases of the issue's table ------------------------------------------
def _cartpole(n, env_id0=0):
    from garage_amd.envs import CartPoleVecEnv
    return CartPoleVecEnv(n, max_episode_length=24, seed=3, env_id0=env_id0)


def _cartpole_normalized(n, env_id0=0):
    from garage_amd.envs import NormalizedVecEnv
    return NormalizedVecEnv(_cartpole(n, env_id0), normalize_obs=True)


def _synthetic(n, env_id0=0):
    from garage_amd.envs import SyntheticVecEnv
    return SyntheticVecEnv(n, 6, 3, 12, min_len=3, seed=8, env_id0=env_id0)


def _categorical(hidden):
    def make(spec):
        from garage_amd.policies import CategoricalMLPPolicy
        return CategoricalMLPPolicy(spec, hidden_sizes=hidden)
    return make


def _gaussian(hidden, **kw):
    def make(spec):
        from garage_amd.policies import GaussianMLPPolicy
        return GaussianMLPPolicy(spec, hidden_sizes=hidden, learn_std=True,
                                 **kw)
    return make


CASES = {
    # env, policy, max_episode_length, num_samples
    'cartpole-tanh-8-8-resident-L3': (_cartpole, _categorical((8, 8)), 24, 40),
    'cartpole-tanh-8-resident-L2': (_cartpole, _categorical((8, )), 24, 40),
    'synthetic-relu-ln-8-8-gen-resident': (
        _synthetic, _gaussian((8, 8), hidden_nonlinearity=torch.relu,
                              layer_normalization=True), 12, 40),
    'synthetic-tanh-320-streamed-512': (_synthetic, _gaussian((320, )), 12,
                                        40),
    'cartpole-normalized-obs-tanh-8-8': (_cartpole_normalized,
                                         _categorical((8, 8)), 24, 40),
}


def _member_vectors(pol, M):
    """Visibly different parameters per member, the log-std included."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.5 * rng.randn(M, base.size).astype(np.float32)
    if pol.kind == 'gaussian':
        vectors[:, 0] = np.log(0.5) + 0.3 * np.arange(M)
    return vectors.astype(np.float32)


def _lone_worker_batch(make_env, make_pol, vector, m, g, P, num_samples):
    from garage_amd.sampler import GpuVecWorker
    env = make_env(g, env_id0=m * g)
    pol = make_pol(env.spec)
    pol.set_flat_param_values(vector)
    w = GpuVecWorker(seed=SEED, max_episode_length=P, worker_number=0,
                     n_envs=g)
    w.update_agent(pol)
    w.update_env(env)
    return w.rollout_samples(num_samples).to_host()


def _same_batch(a, b):
    for k in ('observations', 'last_observations', 'actions', 'rewards',
              'step_types', 'lengths'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape, k
        assert np.array_equal(_bits(x), _bits(y)), k
    assert sorted(a.agent_infos) == sorted(b.agent_infos)
    for k in a.agent_infos:
        assert np.array_equal(_bits(a.agent_infos[k]),
                              _bits(b.agent_infos[k])), k


@pytest.mark.parametrize('M,g', SIZES, ids=['3x16', '2x32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_each_member_equals_a_lone_worker_bit_for_bit(case, M, g):
    from garage_amd import _lib
    from garage_amd.sampler import GpuPopulationSampler
    make_env, make_pol, P, num_samples = CASES[case]
    lib = _lib.load()
    torch.manual_seed(1)
    env = make_env(M * g)
    pol = make_pol(env.spec)
    vectors = _member_vectors(pol, M)
    template = pol.get_flat_param_values()
    pop = GpuPopulationSampler(pol, env, n_members=M, max_episode_length=P,
                               seed=SEED)
    counts, real = [], pop._steps

    def steps(b, col, k, params):
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
        real(b, col, k, params)
        counts.append((k, int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before))

    pop._steps = steps
    batches = pop.obtain_samples(0, num_samples, pol.pack_members(vectors))
    # the first chunk: ceil(num_samples / g) columns, ONE launch of kind 13
    assert counts[0] == (-(-num_samples // g), 1)
    assert all(c == (1 if k > 1 else 0) for k, c in counts[1:])
    assert len(batches) == M
    # the template policy's own parameters are not touched
    assert np.array_equal(pol.get_flat_param_values(), template)
    head = 'mean' if pol.kind == 'gaussian' else 'prob'
    total = 0
    for m in range(M):
        got = batches[m].to_host()
        want = _lone_worker_batch(make_env, make_pol, vectors[m], m, g, P,
                                  num_samples)
        _same_batch(got, want)
        assert int(got.lengths.sum()) >= num_samples
        assert head in got.agent_infos
        total += int(got.lengths.sum())
        if pol.kind == 'gaussian':
            assert np.all(got.agent_infos['log_std'] ==
                          np.float32(vectors[m, 0]))
    assert pop.total_env_steps == total
    # the members really differ: two members' batches are not each other's
    a, b = batches[0].to_host(), batches[1].to_host()
    assert (a.actions.shape != b.actions.shape
            or not np.array_equal(a.actions, b.actions))


def test_compact_vectors_are_packed_on_the_way_in():
    """``member_params`` as an ``(M, P)`` array gives what the packed tensor
    gives (fresh samplers: same seeds, same Philox counters)."""
    from garage_amd.sampler import GpuPopulationSampler
    make_env, make_pol, P, num_samples = CASES['cartpole-tanh-8-resident-L2']
    out = []
    for packed in (True, False):
        env = make_env(48)
        torch.manual_seed(1)
        pol = make_pol(env.spec)
        vectors = _member_vectors(pol, 3)
        pop = GpuPopulationSampler(pol, env, n_members=3, max_episode_length=P,
                                   seed=SEED)
        params = pol.pack_members(vectors) if packed else vectors
        out.append([b.to_host() for b in pop.obtain_samples(0, num_samples,
                                                            params)])
    for a, b in zip(*out):
        _same_batch(a, b)


# -- the C ABI directly --------------------------------------------------------
K_STEPS = 12


def _direct(entry, n_members, params, stride, pol, n=48):
    """``K_STEPS`` rollout steps of a fresh CartPole batch through ``entry``;
    the rollout buffers."""
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.sampler import GpuVecWorker
    env = _cartpole(n)
    w = GpuVecWorker(seed=SEED, max_episode_length=24, worker_number=0,
                     n_envs=n)
    w.update_agent(pol)
    w.update_env(env)
    w._start()
    b = w._alloc_buffers(n * K_STEPS)
    a, r = w._head_args(b, 0, True), w._record_args(b, 0)
    ref, _keep = env.native_env_ref(b['dev_infos'])
    args = [C.byref(pol.net._desc), dptr(params), C.byref(a), C.byref(ref),
            C.byref(r), None, K_STEPS]
    if entry == 'ga_policy_env_step_members_f32':
        args += [n_members, stride]
    call(entry, *args, stream_ptr())
    torch.cuda.synchronize()
    out = {k: b[k][:, :K_STEPS].cpu().numpy()
           for k in ('obs', 'act', 'head', 'rew', 'st', 'lastobs')}
    out['tail'] = b['tail'][:, :K_STEPS].to(torch.int32).cpu().numpy()
    # what the launch does not write is not compared: the padding columns of a
    # row, and last observations anywhere but at an episode's end
    out['head'] = out['head'][:, :, :2]
    out['act'] = out['act'][:, :, :1]
    out['lastobs'][out['tail'] == 0] = 0
    out['step_eps'] = b['step_eps'][:K_STEPS].cpu().numpy()
    out['next_obs'] = env.obs.cpu().numpy()
    return out


def _same_buffers(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_padded_member_stride_with_a_poisoned_gap():
    torch.manual_seed(1)
    pol = _categorical((8, 8))(_cartpole(48).spec)
    M, flat = 3, pol.net.n_flat
    packed = pol.pack_members(_member_vectors(pol, M))
    compact = _direct('ga_policy_env_step_members_f32', M, packed, flat, pol)
    padded = torch.full((M, flat + 4), float('nan'), dtype=torch.float32,
                        device=packed.device)
    padded[:, :flat] = packed
    spread = _direct('ga_policy_env_step_members_f32', M, padded, flat + 4,
                     pol)
    _same_buffers(compact, spread)
    assert np.isfinite(compact['head']).all()
    assert compact['step_eps'].sum() > 0  # episodes ended inside the launch
    # the three members act differently on the same start states
    assert len({compact['act'][m * 16:(m + 1) * 16].tobytes()
                for m in range(M)}) == M


def test_one_member_is_the_single_policy_entry_point():
    torch.manual_seed(1)
    pol = _categorical((8, 8))(_cartpole(48).spec)
    flat = pol.net.n_flat
    one = _direct('ga_policy_env_step_members_f32', 1, pol.net.params, flat,
                  pol)
    ref = _direct('ga_policy_env_step_fused_f32', None, pol.net.params, None,
                  pol)
    _same_buffers(one, ref)
    # ... with a ragged last workgroup too (40 envs: 2.5 workgroups)
    one = _direct('ga_policy_env_step_members_f32', 1, pol.net.params, flat,
                  pol, n=40)
    ref = _direct('ga_policy_env_step_fused_f32', None, pol.net.params, None,
                  pol, n=40)
    _same_buffers(one, ref)


# -- what the sampler refuses ---------------------------------------------------
def test_sampler_refusals_name_their_reason():
    from garage_amd.envs import (CartPoleEnv, HostVecEnv, NormalizedVecEnv,
                                 SyntheticVecEnv)
    from garage_amd.policies import GaussianMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    env = _cartpole(48)
    pol = _categorical((8, ))(env.spec)
    kw = dict(n_members=3, max_episode_length=24, seed=SEED)
    with pytest.raises(ValueError, match='noise_fn'):
        GpuPopulationSampler(pol, env, worker_args=dict(
            noise_fn=lambda step: None), **kw)
    with pytest.raises(ValueError, match='do not split into 5 members'):
        GpuPopulationSampler(pol, env, n_members=5, max_episode_length=24)
    host = HostVecEnv([CartPoleEnv(seed=3, env_id=i, max_episode_length=24)
                       for i in range(48)])
    with pytest.raises(TypeError, match='device env batch'):
        GpuPopulationSampler(pol, host, **kw)
    bounded = SyntheticVecEnv(48, 6, 3, 12, seed=8, action_bounds=(-2., 2.))
    gpol = GaussianMLPPolicy(bounded.spec, hidden_sizes=(8, ))
    with pytest.raises(ValueError, match='rescales actions'):
        GpuPopulationSampler(gpol, NormalizedVecEnv(bounded), **kw)
    wide = GaussianMLPPolicy(bounded.spec, hidden_sizes=(600, 8))
    with pytest.raises(ValueError, match='does not take this network'):
        GpuPopulationSampler(wide, bounded, **kw)
    # 3 members of 8 envs: half a workgroup each -- the library's own refusal
    from garage_amd._lib import GarageAmdError
    small = _cartpole(24)
    pop = GpuPopulationSampler(pol, small, **kw)
    with pytest.raises(GarageAmdError, match='8 envs per member'):
        pop.obtain_samples(0, 40, _member_vectors(pol, 3))
    with pytest.raises(ValueError, match='one row per member'):
        GpuPopulationSampler(pol, env, **kw).obtain_samples(
            0, 40, _member_vectors(pol, 2))


def test_pickling_rebuilds_the_worker_and_keeps_its_counters():
    import pickle
    from garage_amd.sampler import GpuPopulationSampler
    env = _cartpole(32)
    torch.manual_seed(1)
    pol = _categorical((8, ))(env.spec)
    vectors = _member_vectors(pol, 2)
    pop = GpuPopulationSampler(pol, env, n_members=2, max_episode_length=24,
                               seed=SEED)
    pop.obtain_samples(0, 40, vectors)
    clone = pickle.loads(pickle.dumps(pop))
    assert clone.total_env_steps == pop.total_env_steps > 0
    assert clone._worker._global_step == pop._worker._global_step > 0
    a = pop.obtain_samples(1, 40, vectors)
    b = clone.obtain_samples(1, 40, vectors)
    for x, y in zip(a, b):
        _same_batch(x.to_host(), y.to_host())
    pop.shutdown_worker()


# -- CEM ----------------------------------------------------------------------
class _Trainer:
    """``step_epochs`` / ``step_itr`` / ``_train_args`` of ``garage.Trainer``."""

    def __init__(self, epochs, batch_size):
        self._epochs = epochs
        self._train_args = types.SimpleNamespace(batch_size=batch_size)
        self.step_itr = 0
        self.step_episode = None
        self.total_env_steps = 0

    def step_epochs(self):
        for epoch in range(self._epochs):
            yield epoch


CEM_MEMBERS, CEM_G, CEM_EPOCHS, CEM_BATCH, CEM_LENGTH = 32, 16, 6, 320, 200


def cem_cartpole_run(seed):
    """``(first epoch's population mean return, mean policy's return after the
    last epoch)`` of one seeded CEM run on ``CartPoleVecEnv``."""
    from garage_amd.algos import CEM
    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    n = CEM_MEMBERS * CEM_G
    torch.manual_seed(seed)
    env = CartPoleVecEnv(n, max_episode_length=CEM_LENGTH, seed=seed)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(8, ),
                               double_softmax=False)
    sampler = GpuPopulationSampler(pol, env, n_members=CEM_MEMBERS,
                                   max_episode_length=CEM_LENGTH, seed=seed)
    algo = CEM(env.spec, pol, sampler, CEM_MEMBERS, best_frac=0.25, init_std=1,
               extra_std=0)
    returns, real = [], algo._train_once

    def train_once(itr, episodes):
        real(itr, episodes)
        returns.append(float(np.mean(
            [r.sum() for r in np.split(episodes.rewards,
                                       np.cumsum(episodes.lengths)[:-1])])))

    algo._train_once = train_once
    np.random.seed(seed)
    trainer = _Trainer(CEM_EPOCHS, CEM_BATCH)
    algo.train(trainer)
    assert trainer.step_itr == CEM_EPOCHS * CEM_MEMBERS
    first = float(np.mean(returns[:CEM_MEMBERS]))
    # the mean policy, evaluated by every member's envs
    mean = np.repeat(algo._cur_mean[None], CEM_MEMBERS, axis=0)
    batches = sampler.obtain_samples(0, CEM_BATCH, mean)
    last = float(np.mean(np.concatenate([
        np.add.reduceat(b.rewards, np.cumsum(b.lengths) - b.lengths)
        for b in batches])))
    sampler.shutdown_worker()
    return first, last


# Measured on an MI355X, seeds 0 .. 4, (first epoch's
# population mean, mean policy after the last epoch) -> gain:
#   0: (19.73, 197.92) -> 178.19    1: (13.56, 43.11) -> 29.56
#   2: (13.82,  59.89) ->  46.07    3: (17.02, 55.59) -> 38.57
#   4: (14.29,  57.98) ->  43.69
# margin = half the smallest gain seen (29.56); the test runs seed 0, whose run
# repeats exactly on a given build (Philox noise, seeded np.random)
CEM_MARGIN = 14.78


def test_cem_learns_cartpole():
    first, last = cem_cartpole_run(0)
    print('CEM CartPole seed 0: first epoch population mean %.3f, mean policy '
          'after the last epoch %.3f' % (first, last))
    assert last - first > CEM_MARGIN
