"""A population's episodes packed in one pass (``ga_member_pack_index``,
``ga_member_pack_gather``, ``GpuPopulationSampler.obtain_population``).

Two twins: the entries themselves against the numpy twin of the header's statement
(``_member_pack_ref.py``), exactly, with sentinels behind what they may write and
poison where they must; and the sampler's joint path against its per-member path
(``joint_pack=False``: one ``GpuVecWorker._pack`` per member), every array of every
member bit for bit.
"""
import numpy as np
import pytest
import torch

import _member_pack_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
SENTINEL = 0x5A5A5A5A
GUARD = 24  # entries behind every output


def _L():
    from garage_amd import _lib
    return _lib


def _stream():
    return _L().stream_ptr()


def _guarded(count, dtype):
    """``count`` entries followed by ``GUARD`` sentinels, all of them poisoned."""
    t = torch.full((count + GUARD, ), SENTINEL, dtype=dtype, device='cuda')
    return t


def _intact(t, count):
    return bool((t[count:] == SENTINEL).all())


def _progress_on_device(tail_dev, M, n_cols, num_samples):
    L = _L()
    n, tcap = tail_dev.shape
    prog = torch.zeros(M, 3, dtype=torch.int32, device='cuda')
    col_base = torch.zeros(M, tcap, dtype=torch.int32, device='cuda')
    L.call('ga_member_progress', L.dptr(tail_dev), n, tcap, n_cols, M, num_samples,
           L.dptr(prog), L.dptr(col_base), _stream())
    return prog, col_base


def _run_index(tail_dev, M, n_cols, prog, col_base, max_eps, max_samples):
    L = _L()
    n, tcap = tail_dev.shape
    i32, i64 = torch.int32, torch.int64
    out = dict(ep_env=_guarded(max_eps, i32), ep_end=_guarded(max_eps, i32),
               ep_len=_guarded(max_eps, i32), ep_off=_guarded(max_eps + M, i64),
               member_samples=_guarded(M, i64), member_off=_guarded(M + 1, i64),
               src=_guarded(max_samples, i32))
    L.call('ga_member_pack_index', L.dptr(tail_dev), n, tcap, n_cols, M,
           L.dptr(prog), L.dptr(col_base), max_eps, max_samples,
           L.dptr(out['ep_env']), L.dptr(out['ep_end']), L.dptr(out['ep_len']),
           L.dptr(out['ep_off']), L.dptr(out['member_samples']),
           L.dptr(out['member_off']), L.dptr(out['src']), _stream())
    torch.cuda.synchronize()
    return out


# ---- the two entries against the twin -------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_index_equals_the_twin_and_stays_inside_its_arrays(name):
    tail, M, n_cols, num_samples = CASES[name]
    tail_dev = torch.from_numpy(tail.view(np.int16)).cuda().view(torch.uint16)
    want_prog, want_base = ref.member_progress(tail, M, n_cols, num_samples)
    prog, col_base = _progress_on_device(tail_dev, M, n_cols, num_samples)
    assert np.array_equal(prog.cpu().numpy(), want_prog)
    assert np.array_equal(col_base.cpu().numpy()[:, :n_cols],
                          want_base[:, :n_cols])
    want = ref.pack_index(tail, M, want_prog)
    N, R = len(want['ep_env']), len(want['src'])
    assert N >= 1 and R >= 16
    sizes = dict(ep_env=N, ep_end=N, ep_len=N, ep_off=N + M, member_samples=M,
                 member_off=M + 1, src=R)
    got = _run_index(tail_dev, M, n_cols, prog, col_base, N, R)
    for key, count in sizes.items():
        assert np.array_equal(got[key][:count].cpu().numpy(), want[key]), key
        assert _intact(got[key], count), key
    # arrays that are too small: what fits is written, nothing behind it
    if N > 2 and R > 32:
        small = _run_index(tail_dev, M, n_cols, prog, col_base, N - 2, R - 32)
        for key in ('ep_env', 'ep_end', 'ep_len'):
            assert np.array_equal(small[key][:N - 2].cpu().numpy(),
                                  want[key][:N - 2]), key
            assert _intact(small[key], N - 2), key
        assert _intact(small['ep_off'], N - 2 + M)
        assert _intact(small['src'], R - 32)
        src = small['src'][:R - 32].cpu().numpy()
        # a row holds its cell or -1 (the episodes that did not fit), never another
        assert ((src == want['src'][:R - 32]) | (src == -1)).all()
    # more room than needed: the rows behind the last member read -1
    roomy = _run_index(tail_dev, M, n_cols, prog, col_base, N + 3, R + 40)
    src = roomy['src'][:R + 40].cpu().numpy()
    assert np.array_equal(src[:R], want['src']) and (src[R:] == -1).all()
    assert _intact(roomy['src'], R + 40)
    assert (roomy['ep_env'][N:N + 3] == SENTINEL).all()  # no episode was invented


# (elem bytes, width, row stride, per episode): the planes of a batch -- 16-byte rows,
# rows of two quads, a stride wider than the row, rewards, step types, the terminal
# observations, an env_info per sample and at the episode's end -- and the shapes only
# the by-element path takes
PLANES = [(4, 4, 4, False), (4, 8, 8, False), (4, 4, 8, False), (4, 1, 1, False),
          (1, 1, 1, False), (4, 4, 4, True), (1, 1, 1, False), (1, 1, 1, True),
          (4, 3, 3, False), (1, 5, 8, False), (4, 1, 2, True), (4, 12, 12, True)]


@pytest.mark.parametrize('name', list(CASES))
def test_gather_equals_the_twin_and_zeroes_the_padding(name):
    L = _L()
    tail, M, n_cols, num_samples = CASES[name]
    n, tcap = tail.shape
    prog, _ = ref.member_progress(tail, M, n_cols, num_samples)
    idx = ref.pack_index(tail, M, prog)
    # three rows of room behind the last member: -1 there too
    src = np.concatenate([idx['src'], np.full(3, -1)]).astype(np.int32)
    N, R = len(idx['ep_env']), len(src)
    cell_end = idx['ep_env'] * tcap + idx['ep_end']
    rng = np.random.default_rng(3)
    table, checks, keep = [], [], []
    for elem, width, ld, per_episode in PLANES:
        np_dtype, dtype = ((np.float32, torch.float32) if elem == 4 else
                           (np.uint8, torch.uint8))
        host = rng.integers(1, 250, size=(n * tcap, ld)).astype(np_dtype)
        rows = N if per_episode else R
        cells = cell_end if per_episode else src
        want = np.where((cells >= 0)[:, None], host[np.maximum(cells, 0), :width],
                        0).astype(np_dtype)
        source = torch.from_numpy(host).cuda()
        # poisoned, with a guard row behind
        dst = torch.full((rows + 1, ld), 77, dtype=dtype, device='cuda')
        table.append(L.PackPlane(src=source.data_ptr(), dst=dst.data_ptr(),
                                 ld_src=ld, ld_dst=ld, elem_size=elem, width=width,
                                 per_episode=int(per_episode)))
        keep.append(source)
        checks.append((dst, want, rows, width))
    src_dev = torch.from_numpy(src).cuda()
    env_dev = torch.from_numpy(idx['ep_env'].astype(np.int32)).cuda()
    end_dev = torch.from_numpy(idx['ep_end'].astype(np.int32)).cuda()
    L.call('ga_member_pack_gather', (L.PackPlane * len(table))(*table), len(table),
           L.dptr(src_dev), R, L.dptr(env_dev), L.dptr(end_dev), N, tcap,
           _stream())
    torch.cuda.synchronize()
    padding = src < 0
    assert padding.any()
    for i, (dst, want, rows, width) in enumerate(checks):
        got = dst.cpu().numpy()
        assert np.array_equal(got[:rows, :width], want), PLANES[i]
        assert (got[rows] == 77).all(), PLANES[i]           # the guard row
        assert (got[:rows, width:] == 77).all(), PLANES[i]  # between the rows
        if not PLANES[i][3]:
            assert (got[:rows, :width][padding] == 0).all(), PLANES[i]


# ---- the joint path against the per-member path ------------------------------------
SEED = 5


def _cartpole(n, P=24):
    from garage_amd.envs import CartPoleVecEnv
    return CartPoleVecEnv(n, max_episode_length=P, seed=3)


def _pendulum(n, P=20):
    from garage_amd.envs import PendulumVecEnv
    return PendulumVecEnv(n, max_episode_length=P, seed=3)


def _point(n, P=12):
    from garage_amd.envs import PointVecEnv
    env = PointVecEnv(n, max_episode_length=P)
    # a goal of its own per env: the episode_infos say which env an episode ran in
    env.set_tasks([{'goal': (0.05 * i - 1., 1. - 0.03 * i)} for i in range(n)])
    return env


def _multi_point(n, P=12):
    from garage_amd.envs import MultiTaskPointVecEnv
    return MultiTaskPointVecEnv(n, [(1., 1.), (-1., 0.5), (0.2, -0.9)],
                                env_names=['a', 'b', 'c'], start='spread', seed=4,
                                max_episode_length=P)


def _normalized(n, P=24):
    from garage_amd.envs import NormalizedVecEnv
    return NormalizedVecEnv(_cartpole(n, P), normalize_obs=True)


def _one_step(n, P=1):
    return _cartpole(n, P)


def _policy(spec):
    from garage_amd._dtypes import is_discrete
    from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy
    if is_discrete(spec.action_space):
        return CategoricalMLPPolicy(spec, hidden_sizes=(8, 8))
    return GaussianMLPPolicy(spec, hidden_sizes=(8, 8), learn_std=True)


# env, max_episode_length, num_samples
PATHS = {'cartpole-categorical': (_cartpole, 24, 150),
         'pendulum-gaussian': (_pendulum, 20, 90),
         'point-success-goal': (_point, 12, 70),
         'multi-task-point-task-id': (_multi_point, 12, 70),
         'cartpole-normalized': (_normalized, 24, 150),
         'max-episode-length-1': (_one_step, 1, 40)}
SIZES = [(3, 16), (2, 32), (1, 5)]


def _member_vectors(pol, M):
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + 0.5 * rng.randn(M, base.size).astype(np.float32)
    if pol.kind == 'gaussian':
        vectors[:, 0] = np.log(0.5) + 0.3 * np.arange(M)
    return vectors.astype(np.float32)


def _bits(t):
    if t is None:
        return None
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_array(x, y, what):
    assert (x is None) == (y is None), what
    if x is not None:
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert torch.equal(_bits(x), _bits(y)), what


def _same_dict(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def _same_member(a, b, m):
    for k in ('obs_dev', 'actions_dev', 'rewards_dev', 'step_types_dev',
              'last_obs_dev', 'ep_off_dev'):
        _same_array(getattr(a, k), getattr(b, k), (m, k))
    # the head's rows are padded to a quad and the rollout writes the A columns of
    # the head only: what lies behind them is whatever the rollout buffer held,
    # another allocation in each sampler
    A = a.env_spec.action_space.flat_dim
    assert a.head_dev.shape == b.head_dev.shape
    _same_array(a.head_dev[:, :A], b.head_dev[:, :A], (m, 'head_dev'))
    assert a.lengths.dtype == b.lengths.dtype
    assert np.array_equal(a.lengths, b.lengths), m
    assert a.n_samples == b.n_samples == int(a.lengths.sum())
    _same_dict(a.agent_infos, b.agent_infos, (m, 'agent_infos'))
    _same_dict(a.env_infos, b.env_infos, (m, 'env_infos'))
    _same_dict(a.episode_infos_by_episode, b.episode_infos_by_episode,
               (m, 'episode_infos'))
    assert a._discrete == b._discrete and a._head_name == b._head_name
    assert a.env_spec == b.env_spec


def _pair(path, M, g):
    """(joint sampler, per-member sampler, member vectors): same seed, env batches
    built alike, the same template policy."""
    from garage_amd.sampler import GpuPopulationSampler
    make_env, P, num_samples = PATHS[path]
    out = []
    for joint in (True, False):
        torch.manual_seed(1)
        env = make_env(M * g, P)
        pol = _policy(env.spec)
        out.append(GpuPopulationSampler(pol, env, n_members=M,
                                        max_episode_length=P, seed=SEED,
                                        joint_pack=joint))
    return out[0], out[1], _member_vectors(out[0]._agent, M), num_samples


@pytest.mark.parametrize('M,g', SIZES, ids=['3x16', '2x32', '1x5'])
@pytest.mark.parametrize('path', list(PATHS))
def test_joint_pack_equals_the_per_member_path_bit_for_bit(path, M, g):
    from garage_amd._dtypes import DevicePopulationBatch
    joint, single, vectors, num_samples = _pair(path, M, g)
    assert joint._joint_pack and not single._joint_pack
    for itr in range(2):  # the second call starts from envs in flight
        a = joint.obtain_samples(itr, num_samples, vectors)
        b = single.obtain_samples(itr, num_samples, vectors)
        assert isinstance(a, list) and len(a) == len(b) == M
        for m in range(M):
            _same_member(a[m], b[m], m)
            assert a[m].n_samples >= num_samples
        assert joint.total_env_steps == single.total_env_steps > 0
    if path == 'cartpole-categorical' and M > 1:
        # the members stop in different columns
        assert len({x.n_samples for x in a}) > 1
    if path == 'pendulum-gaussian':
        assert a[0].obs_dev.shape[1] == 4  # three wide, padded to a quad
        assert len({float(x.agent_infos['log_std'][0, 0]) for x in a}) == M
    if path == 'point-success-goal':
        assert a[0].env_infos['success'].dtype == np.bool_
        goals = np.concatenate([x.episode_infos_by_episode['goal'] for x in a])
        assert len(np.unique(goals[:, 0])) > M  # by the episode's own env
    if path == 'multi-task-point-task-id':
        assert a[0].env_infos['task_id'].dtype == np.int64
        assert 'task_name' in a[0].env_infos
        assert len(np.unique(np.concatenate(
            [x.env_infos['task_id'] for x in a]))) == 3
    if path == 'max-episode-length-1':
        assert all((x.lengths == 1).all() for x in a)
    # the population batch behind the list
    pop = joint.obtain_population(2, num_samples, vectors)
    assert isinstance(pop, DevicePopulationBatch) and len(pop) == M
    assert (pop.member_off % 16 == 0).all()
    assert pop.obs_dev.shape[0] == pop.member_off[M]
    assert np.array_equal(pop.member_samples,
                          [x.n_samples for x in pop.members])
    used = torch.zeros(int(pop.member_off[M]), dtype=torch.bool, device='cuda')
    for m in range(M):
        lo = int(pop.member_off[m])
        used[lo:lo + int(pop.member_samples[m])] = True
    assert pop.head_dev is not None
    for t in (pop.obs_dev, pop.actions_dev, pop.head_dev, pop.rewards_dev,
              pop.step_types_dev, *pop.env_info_planes.values()):
        assert not t[~used].any()  # the rows between the members are zeros


@pytest.mark.parametrize('path', ['cartpole-categorical', 'pendulum-gaussian',
                                  'multi-task-point-task-id'])
def test_every_member_view_starts_on_a_16_byte_boundary(path):
    joint, _, vectors, num_samples = _pair(path, 3, 16)
    pop = joint.obtain_population(0, num_samples, vectors)
    for m, b in enumerate(pop.members):
        for k in ('obs_dev', 'actions_dev', 'head_dev', 'rewards_dev',
                  'step_types_dev', 'last_obs_dev'):
            assert getattr(b, k).data_ptr() % 16 == 0, (m, k)
            assert getattr(b, k).is_contiguous(), (m, k)
    for plane in pop.env_info_planes.values():
        for m in range(3):
            assert plane[int(pop.member_off[m]):].data_ptr() % 16 == 0


def test_population_batch_pickles_to_views_of_one_set_of_arrays():
    import pickle
    joint, _, vectors, num_samples = _pair('point-success-goal', 2, 32)
    pop = joint.obtain_population(0, num_samples, vectors)
    copy = pickle.loads(pickle.dumps(pop))
    for m, (a, b) in enumerate(zip(copy.members, pop.members)):
        _same_member(a, b, m)
    lo = int(copy.member_off[1])
    assert copy.members[1].obs_dev.data_ptr() == copy.obs_dev[lo].data_ptr()


# ---- the views feed the joint update ---------------------------------------------------
def _make_members(head):
    """``test_population_update_gpu._make_members``: 3 categorical MLP(32, 32) PPOs on
    CartPole or 2 Gaussian MLP(64, 64) PPOs on Pendulum, 16 envs each, with their own
    learning rate, clip range and permutation seeds."""
    from garage_amd.algos import PPO
    from garage_amd.envs import CartPoleVecEnv, PendulumVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy, GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    if head == 'categorical':
        M, hidden = 3, (32, 32)
        env = CartPoleVecEnv(M * 16, max_episode_length=20, seed=3)
    else:
        M, hidden = 2, (64, 64)
        env = PendulumVecEnv(M * 16, max_episode_length=20, seed=3)
    members = []
    for m in range(M):
        torch.manual_seed(10 + m)
        if head == 'categorical':
            pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hidden)
        else:
            pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden)
        vf = GaussianMLPValueFunction(env.spec, hidden_sizes=hidden)
        opt = (torch.optim.Adam, dict(lr=1e-3 * (m + 1)))
        members.append(PPO(
            env_spec=env.spec, policy=pol, value_function=vf, sampler=None,
            policy_optimizer=OptimizerWrapper(opt, pol, 2, 64,
                                              permutation='device', seed=m),
            vf_optimizer=OptimizerWrapper(opt, vf, 2, 64, permutation='device',
                                          seed=100 + m),
            lr_clip_range=0.1 + 0.05 * m))
    return env, members


def _network_state(algo):
    out = []
    for mod in (algo.policy, algo._value_function):
        out += [mod.net.params.clone(), mod.net.exp_avg.clone(),
                mod.net.exp_avg_sq.clone()]
    return out


@pytest.mark.parametrize('head', ['categorical', 'gaussian'])
def test_population_ppo_trains_on_the_views_as_on_batches_of_their_own(head):
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    runs = []
    for joint in (True, False):
        env, members = _make_members(head)
        pop = PopulationPPO(members)
        sampler = GpuPopulationSampler(members[0].policy, env,
                                       n_members=len(members),
                                       max_episode_length=20, seed=5,
                                       joint_pack=joint)
        np.random.seed(7)
        log = []
        for itr in range(2):
            batches = sampler.obtain_samples(itr, 64, pop.member_params)
            pop.train_once(itr, batches)
            log.append([(_network_state(a), dict(a.last_tabular),
                         a.policy.net.adam_steps,
                         a._value_function.net.adam_steps) for a in pop.members])
        runs.append(log)
    for itr in range(2):
        for m, (a, b) in enumerate(zip(runs[0][itr], runs[1][itr])):
            for x, y in zip(a[0], b[0]):
                assert torch.equal(_bits(x), _bits(y)), (itr, m)
            assert a[1] == b[1] and a[1], (itr, m)
            assert a[2:] == b[2:]
    # the members moved and differ from each other
    assert not torch.equal(runs[0][1][0][0][0], runs[0][0][0][0][0])
    assert not torch.equal(runs[0][1][0][0][0], runs[0][1][1][0][0])


# ---- the calls of a pack do not depend on the number of members ------------------------
def _calls_after_the_last_launch(M, monkeypatch):
    import garage_amd.sampler as sampler_module
    from garage_amd.sampler import GpuPopulationSampler
    torch.manual_seed(1)
    env = _cartpole(M * 16)
    pol = _policy(env.spec)
    pop = GpuPopulationSampler(pol, env, n_members=M, max_episode_length=24,
                               seed=SEED, joint_pack=True)
    names, real_call, real_cpu = [], sampler_module.call, torch.Tensor.cpu

    def call(name, *args):
        names.append(name)
        return real_call(name, *args)

    def cpu(self, *args, **kw):
        names.append('copy to the host')
        return real_cpu(self, *args, **kw)

    with monkeypatch.context() as patch:
        patch.setattr(sampler_module, 'call', call)
        patch.setattr(torch.Tensor, 'cpu', cpu)
        batches = pop.obtain_samples(0, 150, _member_vectors(pol, M))
    assert len(batches) == M
    last = max(i for i, name in enumerate(names)
               if name == 'ga_policy_env_step_members_f32')
    return names[last + 1:]


def test_calls_after_the_rollout_do_not_depend_on_the_number_of_members(
        monkeypatch):
    two = _calls_after_the_last_launch(2, monkeypatch)
    six = _calls_after_the_last_launch(6, monkeypatch)
    assert two == six == ['ga_member_progress', 'copy to the host',
                          'ga_member_pack_index', 'ga_member_pack_gather',
                          'copy to the host']
