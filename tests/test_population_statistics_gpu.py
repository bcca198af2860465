"""``GpuPopulationSampler.obtain_statistics``: a population scored on the device
from the raw rollout buffers (``ga_member_progress``,
``ga_member_episode_statistics``), nothing packed.

The reference of every case is the existing path: a second, identically built
and seeded ``GpuPopulationSampler`` whose ``obtain_samples`` batches
(``test_population_gpu.py`` pins them bit for bit to lone workers) are reduced on
the host.  Lengths, termination and success flags must be equal, the
undiscounted returns bit-equal to ``ga_episode_sums_f32``'s, the discounted
returns bit-equal to ``log_performance_host``'s fp64 recurrence and, rounded to
fp32, within one fp32 ulp of the parallel scan's.  Each case also asserts, on the
twin, the conditions it exists for.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_ROLLOUT = 13
SEED = 5
DISCOUNT = 0.99  # not exact in binary


def _cartpole(n):
    from garage_amd.envs import CartPoleVecEnv
    return CartPoleVecEnv(n, max_episode_length=24, seed=3)


def _cartpole_normalized(n):
    from garage_amd.envs import NormalizedVecEnv
    return NormalizedVecEnv(_cartpole(n), normalize_obs=True)


def _synthetic(n):
    from garage_amd.envs import SyntheticVecEnv
    return SyntheticVecEnv(n, 6, 3, 12, min_len=1, seed=8)


def _point(n):
    """Per-env goals: every eighth env's at the origin (success within a step
    or two), the others' out of reach within 12 steps of at most 0.1."""
    from garage_amd.envs import PointVecEnv
    env = PointVecEnv(n, max_episode_length=12)
    env.set_tasks([dict(goal=(0., 0.) if i % 8 == 0 else (4., 4.))
                   for i in range(n)])
    return env


def _categorical(spec):
    from garage_amd.policies import CategoricalMLPPolicy
    return CategoricalMLPPolicy(spec, hidden_sizes=(8, ))


def _gaussian(spec):
    from garage_amd.policies import GaussianMLPPolicy
    return GaussianMLPPolicy(spec, hidden_sizes=(8, ), learn_std=True)


CASES = {
    # env, policy, (M, g), max_episode_length, num_samples
    'cartpole-3x16': (_cartpole, _categorical, (3, 16), 24, 40),
    'cartpole-2x32': (_cartpole, _categorical, (2, 32), 24, 40),
    'synthetic-3x16': (_synthetic, _gaussian, (3, 16), 12, 40),
    'synthetic-2x48': (_synthetic, _gaussian, (2, 48), 12, 40),
    'synthetic-2x272': (_synthetic, _gaussian, (2, 272), 12, 600),
    'point-success-2x32': (_point, _gaussian, (2, 32), 12, 100),
    'cartpole-normalized-2x32': (_cartpole_normalized, _categorical, (2, 32),
                                 24, 40),
}


# (seed, scale) of the member vectors where a case's conditions need another
# draw than test_population_gpu.py's (17, 0.5): at that scale no CartPole policy
# keeps its poles up for the 24 steps a TIMEOUT takes; with this one a member does
# (c_m = 24) while another is done by column 12 to 15
# ; the PointEnv members stay close to the initial policy, whose small means let
# the action noise decide: at 0.5 both members walked straight out of reach of the
# origin and no episode was successful
DRAWS = {'cartpole-3x16': (2, 2.0), 'cartpole-2x32': (2, 2.0),
         'cartpole-normalized-2x32': (2, 2.0),
         'point-success-2x32': (17, 0.05)}


def _member_vectors(pol, M, seed=17, scale=0.5):
    """``test_population_gpu.py``'s: visibly different parameters per member,
    the log-std included."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(seed)
    vectors = base[None] + scale * rng.randn(M, base.size).astype(np.float32)
    if pol.kind == 'gaussian':
        vectors[:, 0] = np.log(0.5) + 0.3 * np.arange(M)
    return vectors.astype(np.float32)


def _sampler(case, **kw):
    from garage_amd.sampler import GpuPopulationSampler
    make_env, make_pol, (M, g), P, _ = CASES[case]
    torch.manual_seed(1)
    env = make_env(M * g)
    pol = make_pol(env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=M, max_episode_length=P,
                               seed=SEED, **kw)
    return pop, pol.pack_members(_member_vectors(pol, M,
                                                 *DRAWS.get(case, ())))


def _spy_on_packing(pop):
    """Records, per ``_pack`` call of the twin, the member's ``c_m`` and its
    rows of the ``tail`` buffer."""
    seen, real = [], pop._worker._pack

    def pack(b, n_steps, first_step=0, member=None):
        lo, hi = member[0], member[1]
        seen.append((int(n_steps), b['tail'][lo:hi].to(torch.int32).cpu()
                     .numpy()))
        return real(b, n_steps, first_step, member)

    pop._worker._pack = pack
    return seen


def _counted_rollout_launches(pop):
    """``(k, launches of kind 13)`` per ``_steps`` call."""
    from garage_amd import _lib
    lib, counts, real = _lib.load(), [], pop._steps

    def steps(b, col, k, params):
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
        real(b, col, k, params)
        counts.append((k, int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before))

    pop._steps = steps
    return counts


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_member(stats, batch, label=''):
    """``stats`` against the twin's device batch of the same member, reduced by
    the existing code."""
    from garage_amd._dtypes import EpisodeStatistics, StepType
    from garage_amd.functions import episode_statistics
    assert isinstance(stats, EpisodeStatistics)
    assert stats.discount == DISCOUNT
    host = batch.to_host()
    lengths = np.asarray(host.lengths, dtype=np.int64)
    assert stats.lengths.dtype == np.int64
    assert np.array_equal(stats.lengths, lengths), label
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    types = np.asarray([int(s) for s in host.step_types])
    term = np.logical_or.reduceat(types == int(StepType.TERMINAL), starts)
    assert stats.terminated.dtype == np.float64
    assert np.array_equal(stats.terminated, term.astype(np.float64)), label
    if 'success' in host.env_infos:
        succ = np.logical_or.reduceat(
            np.asarray(host.env_infos['success']).astype(bool), starts)
        assert np.array_equal(stats.success, succ.astype(np.float64)), label
    else:
        assert stats.success is None
    und, scan, _, _ = episode_statistics(batch, DISCOUNT)
    assert stats.undiscounted_returns.dtype == np.float64
    assert (stats.undiscounted_returns.tobytes() == und.tobytes()), label
    want = []
    for s, L in zip(starts, lengths):
        ret = 0.0
        for x in host.rewards[s:s + L][::-1]:
            ret = float(x) + DISCOUNT * ret
        want.append(ret)
    want = np.asarray(want, dtype=np.float64)
    diff = np.abs(stats.discounted_returns - want).max()
    got32 = stats.discounted_returns.astype(np.float32).astype(np.float64)
    off = np.abs(got32 - scan) / _ulp32(scan)
    print('%s: %d episodes, discounted vs host recurrence max |diff| %.3g, vs '
          'the fp32 scan %.3g ulp' % (label, len(lengths), diff, off.max()))
    assert stats.discounted_returns.tobytes() == want.tobytes(), label
    assert (off <= 1.0).all(), label
    return host


def _run_case(case):
    """``obtain_statistics`` of one sampler, ``obtain_samples`` of its twin."""
    _, _, (M, g), _, num_samples = CASES[case]
    pop, params = _sampler(case)
    twin, twin_params = _sampler(case)
    packed = _spy_on_packing(twin)
    counts, twin_counts = (_counted_rollout_launches(pop),
                           _counted_rollout_launches(twin))
    stats = pop.obtain_statistics(0, num_samples, params, DISCOUNT)
    batches = twin.obtain_samples(0, num_samples, twin_params)
    assert len(stats) == len(batches) == M
    hosts = [_check_member(stats[m], batches[m], '%s member %d' % (case, m))
             for m in range(M)]
    assert pop.total_env_steps == twin.total_env_steps > 0
    assert pop._worker._global_step == twin._worker._global_step > 0
    # same stepping schedule, same launches
    assert counts == twin_counts
    # (a launch of one column is not of kind 13)
    first = -(-num_samples // g)
    assert counts[0] == (first, 1 if first > 1 else 0)
    assert len(counts) >= 2 or case.startswith(('synthetic', 'point'))
    return dict(pop=pop, twin=twin, params=params, twin_params=twin_params,
                hosts=hosts, packed=packed,
                stepped=pop._worker._global_step)


def _absent_episodes(run):
    """Episodes of the twin that ended in a stepped column ``>= c_m``."""
    return sum(int((tail[:, c:run['stepped']] != 0).sum())
               for c, tail in run['packed'])


def _last_step_types(hosts):
    from garage_amd._dtypes import StepType
    out = set()
    for h in hosts:
        ends = np.cumsum(h.lengths) - 1
        out |= {StepType(int(s)) for s in np.asarray(h.step_types)[ends]}
    return out


@pytest.mark.parametrize('case', ['cartpole-3x16', 'cartpole-2x32',
                                  'cartpole-normalized-2x32'])
def test_cartpole_members_with_different_c_m(case):
    from garage_amd._dtypes import StepType
    run = _run_case(case)
    c = [c_m for c_m, _ in run['packed']]
    print(case, 'c_m', c, 'stepped', run['stepped'], 'absent',
          _absent_episodes(run))
    if case != 'cartpole-normalized-2x32':  # (exists for the wrapped env path)
        assert len(set(c)) >= 2
        assert _last_step_types(run['hosts']) == {StepType.TERMINAL,
                                                  StepType.TIMEOUT}
    if case == 'cartpole-3x16':
        # a member that was done early kept stepping: what it finished at or
        # after its c_m is not in its statistics
        assert _absent_episodes(run) > 0


@pytest.mark.parametrize('case', ['synthetic-3x16', 'synthetic-2x48',
                                  'synthetic-2x272'])
def test_synthetic_rewards_and_one_step_episodes(case):
    run = _run_case(case)
    lengths = np.concatenate([h.lengths for h in run['hosts']])
    print(case, 'episodes', len(lengths), 'shortest', lengths.min(), 'c_m',
          [c for c, _ in run['packed']], 'stepped', run['stepped'])
    assert lengths.min() == 1
    # ... one of them in the very first column
    assert any((tail[:, 0] == 1).any() for _, tail in run['packed'])
    if case == 'synthetic-2x272':
        # episodes of envs past the first 256 of a member end in one column
        # together with episodes of envs before them
        assert any(((tail[:256, :c] != 0).any(0) & (tail[256:, :c] != 0).any(0))
                   .any() for c, tail in run['packed'])


def test_point_env_success_plane():
    run = _run_case('point-success-2x32')
    flags = []
    for h in run['hosts']:
        starts = np.cumsum(h.lengths) - h.lengths
        flags.append(np.logical_or.reduceat(
            np.asarray(h.env_infos['success']).astype(bool), starts))
    flags = np.concatenate(flags)
    print('point: episodes', len(flags), 'successful', int(flags.sum()))
    assert flags.any() and not flags.all()


def test_a_second_call_on_the_same_sampler():
    """Envs with progress are reset and the Philox counter goes on: the second
    call equals the twin's second ``obtain_samples``."""
    case = 'cartpole-3x16'
    run = _run_case(case)
    M, num_samples = CASES[case][2][0], CASES[case][4]
    first = run['stepped']
    stats = run['pop'].obtain_statistics(1, num_samples, run['params'],
                                         DISCOUNT)
    batches = run['twin'].obtain_samples(1, num_samples, run['twin_params'])
    for m in range(M):
        _check_member(stats[m], batches[m], 'second call, member %d' % m)
    assert run['pop'].total_env_steps == run['twin'].total_env_steps
    assert (run['pop']._worker._global_step
            == run['twin']._worker._global_step > first)


def test_no_packing_and_no_gathers(monkeypatch):
    import garage_amd.sampler as sampler_module
    case = 'point-success-2x32'
    pop, params = _sampler(case, statistics_only=True)
    assert pop.statistics_only is True
    assert _sampler(case)[0].statistics_only is False
    names, real = [], sampler_module.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(sampler_module, 'call', call)
    pop.obtain_statistics(0, CASES[case][4], params, DISCOUNT)
    assert set(names) == {'ga_policy_env_step_members_f32',
                          'ga_member_progress',
                          'ga_member_episode_statistics'}
    for name in ('ga_pack_episodes', 'ga_pack_src_index', 'ga_gather_rows_f32',
                 'ga_gather_f32', 'ga_gather_u8'):
        assert name not in names
    # one progress check per launch, one ending
    assert names.count('ga_member_progress') == names.count(
        'ga_policy_env_step_members_f32')
    assert names.count('ga_member_episode_statistics') == 1


# -- CEM --------------------------------------------------------------------------
class _Trainer:

    def __init__(self, epochs, batch_size):
        self._epochs = epochs
        self._train_args = types.SimpleNamespace(batch_size=batch_size)
        self.step_itr = 0
        self.step_episode = None
        self.total_env_steps = 0

    def step_epochs(self):
        for epoch in range(self._epochs):
            yield epoch


# test_population_gpu.py's CartPole CEM
CEM_MEMBERS, CEM_G, CEM_EPOCHS, CEM_BATCH, CEM_LENGTH = 32, 16, 6, 320, 200


def _cem_run(statistics_only, seed=0):
    from garage_amd._dtypes import EpisodeStatistics
    from garage_amd.algos import CEM
    from garage_amd.envs import CartPoleVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuPopulationSampler
    torch.manual_seed(seed)
    env = CartPoleVecEnv(CEM_MEMBERS * CEM_G, max_episode_length=CEM_LENGTH,
                         seed=seed)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(8, ),
                               double_softmax=False)
    sampler = GpuPopulationSampler(pol, env, n_members=CEM_MEMBERS,
                                   max_episode_length=CEM_LENGTH, seed=seed,
                                   statistics_only=statistics_only)
    algo = CEM(env.spec, pol, sampler, CEM_MEMBERS, best_frac=0.25, init_std=1,
               extra_std=0)
    returned, kinds, real = [], set(), algo._train_once

    def train_once(itr, episodes):
        rtn = real(itr, episodes)
        returned.append(rtn)
        kinds.add(isinstance(episodes, EpisodeStatistics))
        return rtn

    algo._train_once = train_once
    np.random.seed(seed)
    trainer = _Trainer(CEM_EPOCHS, CEM_BATCH)
    algo.train(trainer)
    assert kinds == {statistics_only}
    assert trainer.step_itr == CEM_EPOCHS * CEM_MEMBERS
    sampler.shutdown_worker()
    return dict(mean=np.array(algo._cur_mean), std=np.array(algo._cur_std),
                returned=np.asarray(returned, dtype=np.float64),
                steps=trainer.total_env_steps, params=algo._cur_params)


def test_cem_is_the_same_run_on_statistics():
    stats, packed = _cem_run(True), _cem_run(False)
    assert stats['returned'].shape == (CEM_EPOCHS * CEM_MEMBERS, )
    for k in ('mean', 'std', 'returned', 'params'):
        assert stats[k].tobytes() == packed[k].tobytes(), k
    assert stats['steps'] == packed['steps'] > 0
