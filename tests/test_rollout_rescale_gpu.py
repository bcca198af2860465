"""``NormalizedVecEnv``'s action rescale inside the one-launch rollout.

The env thread of the fused step rescales the action row it sampled and steps the
wrapped env on it (``rollout_dev.h: action_rescale_row``).  Every check is an
exact twin: the same rollout (a) under ``ga_set_fused_env_step(0)`` -- policy step,
``ga_action_rescale_f32``, ``ga_env_step_record`` per step -- and (b) with every
step driven from Python."""
import ctypes as C

import numpy as np
import pytest
import torch

from _state_env_helpers import GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE, _bits, _np

pytestmark = pytest.mark.gpu

N, O, A, P = 70, 5, 3, 12
LOW = np.asarray([-0.3, -1.0, 0.0], dtype=np.float32)
HIGH = np.asarray([0.2, 2.0, 0.5], dtype=np.float32)
NUMS = (N * P, N * P + 17)
KINDS = (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)

# name -> (hidden sizes, policy keywords, whole-rollout launches (13, 14) of one
# native call; None: the kernel has no counter)
VARIANTS = {
    'resident3': ((32, 32), {}, (1, 0)),
    'resident2': ((32, ), {}, (1, 0)),
    'resident_general': ((32, 32), 'relu-ln', (1, 0)),
    'streamed': ((32, 32, 32), {}, None),
    'wide': ((320, 16), {}, (0, 1)),
}


def _lib():
    from garage_amd import _lib
    return _lib


def _policy(spec, hidden, kw):
    from garage_amd.policies import GaussianMLPPolicy
    if kw == 'relu-ln':
        kw = dict(hidden_nonlinearity=torch.relu, layer_normalization=True)
    return GaussianMLPPolicy(spec, hidden_sizes=hidden, **kw)


def _sampler(env, hidden, kw, worker=None, worker_args=None):
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    torch.manual_seed(2)
    pol = _policy(env.spec, hidden, kw)
    s = GpuVecSampler(pol, env, max_episode_length=env.spec.max_episode_length,
                      n_workers=1, worker_class=worker or GpuVecWorker, seed=4,
                      worker_args=dict(n_envs=env.n_envs, **(worker_args or {})))
    return s, s._workers[0]


def _synthetic(bounds, norm, act_dim=A, scale=1.5):
    from garage_amd.envs import NormalizedVecEnv, SyntheticVecEnv
    return NormalizedVecEnv(
        SyntheticVecEnv(N, O, act_dim, P, min_len=3, seed=6,
                        action_bounds=bounds),
        normalize_obs=norm, normalize_reward=norm, expected_action_scale=scale)


def _counts():
    lib = _lib().load()
    return [int(lib.ga_launch_count(k)) for k in KINDS]


def _run(env, hidden, kw, mode, nums=NUMS):
    """The batches of ``nums`` calls in a row, what the wrapper holds after them
    and the whole-rollout launches counted; ``mode``: 'native', 'per_step' (a)
    or 'python' (b)."""
    lib = _lib().load()
    s, w = _sampler(env, hidden, kw)
    assert w._fused_ok()
    if mode == 'python':
        w._native_steps = lambda *a: False
    before = _counts()
    try:
        if mode == 'per_step':
            lib.ga_set_fused_env_step(0)
        batches = [s.obtain_samples(itr, num, None).to_host()
                   for itr, num in enumerate(nums)]
        torch.cuda.synchronize()
    finally:
        lib.ga_set_fused_env_step(1)
    launches = tuple(c - b for c, b in zip(_counts(), before))
    state = {k: _np(getattr(env, k)) for k in
             ('_obs_mean', '_obs_var', '_reward_mean', '_reward_var')}
    if env._scaled is not None:
        state['_scaled'] = _np(env._scaled)
    return batches, state, launches


def _equal(a, b, equal_nan=False):
    """The same shape, type and bits; ``equal_nan``: or a NaN on both sides."""
    if a.dtype.kind != 'f':
        return np.array_equal(a, b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    words = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = (np.ascontiguousarray(a).view(words) ==
            np.ascontiguousarray(b).view(words))
    if equal_nan:
        same |= np.isnan(a) & np.isnan(b)
    return bool(same.all())


def _same_batch(a, b, equal_nan=False):
    assert np.array_equal(a.lengths, b.lengths)
    assert np.array_equal([int(s) for s in a.step_types],
                          [int(s) for s in b.step_types])
    for k in ('observations', 'last_observations', 'actions', 'rewards'):
        assert _equal(np.asarray(getattr(a, k), dtype=np.float32),
                      np.asarray(getattr(b, k), dtype=np.float32),
                      equal_nan), k
    for infos in ('agent_infos', 'env_infos'):
        da, db = getattr(a, infos), getattr(b, infos)
        assert sorted(da) == sorted(db)
        for k in da:
            assert _equal(np.asarray(da[k]), np.asarray(db[k]), equal_nan), k


def _same_run(got, want, equal_nan=False):
    for a, b in zip(got[0], want[0]):
        _same_batch(a, b, equal_nan)
    assert sorted(got[1]) == sorted(want[1])
    for k in got[1]:
        assert _equal(got[1][k], want[1][k], equal_nan), k


@pytest.mark.parametrize('norm', [True, False], ids=['norm', 'plain'])
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_synthetic_env_every_kernel_variant(variant, norm):
    """Two calls in a row (episodes end and reset inside the launch): batches,
    the scratch rows and the statistics equal (a) and (b) bit for bit; one
    whole-rollout launch per native call; the batch keeps the policy's own
    actions; the rescale acted."""
    hidden, kw, launches = VARIANTS[variant]
    native = _run(_synthetic((LOW, HIGH), norm), hidden, kw, 'native')
    per_step = _run(_synthetic((LOW, HIGH), norm), hidden, kw, 'per_step')
    python = _run(_synthetic((LOW, HIGH), norm), hidden, kw, 'python')
    if launches is not None:
        assert native[2] == tuple(len(NUMS) * c for c in launches)
    assert per_step[2] == (0, 0) and python[2] == (0, 0)
    _same_run(native, per_step)
    _same_run(native, python)
    for eps, num in zip(native[0], NUMS):
        assert int(eps.lengths.sum()) >= num
        assert eps.lengths.min() < P  # episodes ended early: resets in the launch
        acts = eps.actions[:, :A]
        assert (acts > HIGH).any() and (acts < LOW).any()
    # what the env stepped on last lies inside the box
    scaled = native[1]['_scaled'][:, :A]
    assert (scaled >= LOW).all() and (scaled <= HIGH).all()
    # no bounds declared: the same observations and actions (the synthetic env's
    # observations do not depend on the action), other rewards -- the rescale acted
    unbounded = _run(_synthetic(None, norm), hidden, kw, 'native')
    assert np.array_equal(unbounded[0][0].actions, native[0][0].actions)
    assert not np.array_equal(unbounded[0][0].rewards, native[0][0].rewards)


WIDTH_CASES = {
    'A1': (np.asarray([-0.5], np.float32), np.asarray([0.25], np.float32)),
    'A32': (np.linspace(-1.5, -0.1, 32).astype(np.float32),
            np.linspace(0.1, 2.0, 32).astype(np.float32)),
    'half_open': (LOW, np.asarray([0.2, np.inf, 0.5], np.float32)),
}


@pytest.mark.parametrize('case', sorted(WIDTH_CASES))
def test_action_width_and_half_open_box(case):
    """One column, MAX_OUT = 32 columns, and a column with ``high = +inf`` (the
    reference's bound test lets it through; its rows hold inf and NaN)."""
    low, high = WIDTH_CASES[case]
    runs = [_run(_synthetic((low, high), True, act_dim=low.size), (32, 32), {},
                 mode) for mode in ('native', 'per_step')]
    assert runs[0][2] == (len(NUMS), 0) and runs[1][2] == (0, 0)
    _same_run(runs[0], runs[1], equal_nan=True)
    if case == 'half_open':
        assert not np.isfinite(runs[0][1]['_scaled'][:, 1]).all()


def _device_kind(name, n):
    from garage_amd import envs
    if name == 'pendulum':
        return envs.PendulumVecEnv(n, max_episode_length=P, seed=21, env_id0=3)
    if name == 'double_pendulum':
        return envs.DoublePendulumVecEnv(n, max_episode_length=P, seed=21,
                                         env_id0=3)
    if name == 'mountain_car_continuous':
        return envs.MountainCarVecEnv(n, continuous=True, max_episode_length=P,
                                      seed=21, env_id0=3)
    if name == 'point':
        return envs.PointVecEnv(n, goal=(0.3, 0.2), max_episode_length=P)
    if name == 'multi_task_point':
        return envs.MultiTaskPointVecEnv(
            n, [(0.3, 0.2), (-0.2, 0.1), (0.1, -0.3)], max_episode_length=P)
    assert name == 'cartpole'
    return envs.CartPoleVecEnv(n, max_episode_length=P, seed=21, env_id0=3)


@pytest.mark.parametrize('name', ['pendulum', 'double_pendulum',
                                  'mountain_car_continuous', 'point',
                                  'multi_task_point'])
def test_every_continuous_device_kind(name):
    from garage_amd.envs import NormalizedVecEnv
    runs = []
    for mode in ('native', 'per_step'):
        env = NormalizedVecEnv(_device_kind(name, N))
        assert env._act_low is not None
        runs.append(_run(env, (64, 64), {}, mode, nums=(N * P, )))
    # the first steps of the call: one whole-rollout launch
    assert runs[0][2] == (1, 0) and runs[1][2] == (0, 0)
    _same_run(runs[0], runs[1])
    assert int(runs[0][0][0].lengths.sum()) >= N * P


def test_a_discrete_kind_under_the_wrapper_is_not_touched():
    from garage_amd.envs import NormalizedVecEnv
    from garage_amd.policies import CategoricalMLPPolicy
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    env = NormalizedVecEnv(_device_kind('cartpole', N))
    assert env._act_low is None and env._scaled is None
    assert not env.norm_args().act_low
    torch.manual_seed(2)
    pol = CategoricalMLPPolicy(env.spec, hidden_sizes=(64, 64))
    s = GpuVecSampler(pol, env, max_episode_length=P, n_workers=1,
                      worker_class=GpuVecWorker, seed=4,
                      worker_args=dict(n_envs=N))
    before = _counts()
    eps = s.obtain_samples(0, N * P, None).to_host()
    torch.cuda.synchronize()
    assert tuple(c - b for c, b in zip(_counts(), before)) == (1, 0)
    assert int(eps.lengths.sum()) >= N * P


def test_fragment_worker_under_the_rescale():
    """``GpuFragmentWorker`` steps from Python, one ``ga_action_rescale_f32``
    launch per step: its fragments do not depend on the switch."""
    from garage_amd.sampler import GpuFragmentWorker
    lib = _lib().load()
    out = []
    for fused in (1, 0):
        env = _synthetic((LOW, HIGH), True)
        s, w = _sampler(env, (32, 32), {}, worker=GpuFragmentWorker,
                        worker_args=dict(timesteps_per_call=5))
        try:
            lib.ga_set_fused_env_step(fused)
            out.append([w.rollout().to_host() for _ in range(3)])
            torch.cuda.synchronize()
        finally:
            lib.ga_set_fused_env_step(1)
    for a, b in zip(*out):
        _same_batch(a, b)
        assert int(a.lengths.sum()) == 5 * N


SENTINEL = 777.25


class _Direct:
    """A worker's buffers and the C arguments of a rollout of the bounded
    synthetic env at column 0, with guarded scratch rows: ``scaled`` is
    ``[N + 2, 4]`` of SENTINEL, the wrapper's ``_scaled`` its first N rows."""

    def __init__(self, n_steps):
        self.env = env = _synthetic((LOW, HIGH), True)
        self.scaled = torch.full((N + 2, 4), SENTINEL, dtype=torch.float32,
                                 device=env.device)
        env._scaled = self.scaled[:N]
        self.s, self.w = _sampler(env, (32, 32), {})
        w = self.w
        w._start()
        self.b = w._alloc_buffers(N * n_steps)
        for k in ('obs', 'act', 'head', 'lastobs', 'rew', 'st'):
            self.b[k].zero_()  # (allocated uninitialised)
        self.n_steps = n_steps
        self.ref, self._keep = env._env.native_env_ref(self.b['dev_infos'])
        self.desc = C.byref(w.agent.net._desc)
        self.params = w.agent.net.params.data_ptr()

    def args(self, s, swapped):
        """Head, record and norm arguments of step ``s`` reading the current
        buffers, or the other ones when ``swapped``."""
        env, inner, w = self.env, self.env._env, self.w
        a = w._head_args(self.b, s, True)
        a.step = s
        r = w._record_args(self.b, s)
        nm = env.norm_args()
        cur, nxt, raw_cur, raw_nxt = (env.obs, env.next_obs, inner.obs,
                                      inner.next_obs)
        if swapped:
            cur, nxt, raw_cur, raw_nxt = nxt, cur, raw_nxt, raw_cur
        a.obs, r.next_obs = cur.data_ptr(), nxt.data_ptr()
        nm.raw_obs, nm.raw_next_obs = raw_cur.data_ptr(), raw_nxt.data_ptr()
        return a, r, nm, cur

    def fused(self):
        a, r, nm, _ = self.args(0, False)
        _lib().call('ga_policy_env_step_fused_f32', self.desc, self.params,
                    C.byref(a), C.byref(self.ref), C.byref(r), C.byref(nm),
                    self.n_steps, None)

    def three_launches(self):
        call = _lib().call
        for s in range(self.n_steps):
            a, r, nm, cur = self.args(s, s % 2 == 1)
            call('ga_policy_step_fused_f32', self.desc, self.params, C.byref(a),
                 None)
            call('ga_action_rescale_f32', N, A, a.action, a.lda, nm.act_low,
                 nm.act_high, nm.expected_action_scale, nm.scaled_action, a.lda,
                 None)
            call('ga_env_step_record', C.byref(self.ref), C.byref(r),
                 C.byref(nm), nm.scaled_action, a.lda, cur.data_ptr(), None)

    def state(self):
        torch.cuda.synchronize()
        env, inner, b = self.env, self.env._env, self.b
        out = {k: _np(b[k]) for k in ('obs', 'act', 'head', 'lastobs', 'rew',
                                      'st', 'tail', 'step_eps', 'step_samples',
                                      'action', 'done')}
        out.update(scaled=_np(self.scaled), ep_t=_np(self.w._ep_t),
                   reward=_np(env.reward), step_type=_np(env.step_type))
        for k, t in (('obs_a', env.obs), ('obs_b', env.next_obs),
                     ('raw_a', inner.obs), ('raw_b', inner.next_obs)):
            out['env_' + k] = _np(t)
        for k in ('_obs_mean', '_obs_var', '_reward_mean', '_reward_var'):
            out[k] = _np(getattr(env, k))
        return out


@pytest.mark.parametrize('n_steps', [1, 5])
def test_the_fused_entry_honours_the_bounds(n_steps):
    """``ga_policy_env_step_fused_f32`` with ``act_low`` set against
    ``ga_policy_step_fused_f32`` -> ``ga_action_rescale_f32`` ->
    ``ga_env_step_record`` on twin buffers: every buffer the same, and neither
    writes the scratch's padding column or behind its last row."""
    one, three = _Direct(n_steps), _Direct(n_steps)
    one.fused()
    three.three_launches()
    got, want = one.state(), three.state()
    assert sorted(got) == sorted(want)
    for k in got:
        assert _equal(got[k], want[k]), k
    scaled = got['scaled']
    assert (scaled[:N, A:] == SENTINEL).all() and (scaled[N:] == SENTINEL).all()
    assert (scaled[:N, :A] >= LOW).all() and (scaled[:N, :A] <= HIGH).all()
    # the env stepped on the scaled rows, the buffers keep the policy's own
    acts = got['act'][:, :n_steps, :A]
    assert (acts > HIGH).any() and (acts < LOW).any()
    assert np.array_equal(_bits(got['action']),
                          _bits(got['act'][:, n_steps - 1]))
