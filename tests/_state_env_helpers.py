"""What the tests of the seeded state-vector envs share and that names no kind:
bit comparison, guard rows, the twin steppers, samplers built from a table row
(``_state_env_kinds.py``), the Python restatement of Philox and the ctypes
layout program.  A helper that takes a ``row`` reads only the row's fields."""
import ctypes
import types

import numpy as np

GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE = 13, 14  # csrc/prof.h
TERMINAL, TIMEOUT = 2, 3
GUARD = 3
POISON = 12345.0


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mask(flags, device):
    import torch
    return torch.from_numpy(np.asarray(flags, dtype=np.uint8)).to(device)


def _poison(env, n):
    for t in (env._state, env.obs, env.next_obs, env.reward):
        t[n:] = POISON
    env.step_type[n:] = 77
    env._t[n:] = 1234567
    env._resets[n:] = 7654321


def _guards_intact(env, n):
    for t in (env._state, env.obs, env.next_obs, env.reward):
        assert (_np(t[n:]) == np.float32(POISON)).all()
    assert (_np(env.step_type[n:]) == 77).all()
    assert (_np(env._t[n:]) == 1234567).all()
    assert (_np(env._resets[n:]) == 7654321).all()


def _same(a, b):
    assert np.array_equal(a.lengths, b.lengths)
    assert np.array_equal([int(s) for s in a.step_types],
                          [int(s) for s in b.step_types])
    for k in ('observations', 'last_observations', 'actions', 'rewards'):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert sorted(a.agent_infos) == sorted(b.agent_infos)
    for k in a.agent_infos:
        assert np.array_equal(_bits(a.agent_infos[k]),
                              _bits(b.agent_infos[k])), k
    assert sorted(a.env_infos) == sorted(b.env_infos) == []


def _ends(eps):
    """The step types of a batch and the index of each episode's last step."""
    types_ = np.asarray([int(s) for s in eps.step_types])
    return types_, np.cumsum(eps.lengths) - 1


def _ending_types(eps):
    types_, ends = _ends(eps)
    return set(types_[ends].tolist())


def draws(row, seed, id0, n, counter=0):
    """The reset draws of members ``id0 .. id0 + n - 1`` at ``counter``."""
    return np.stack([row.reset_draw(seed, id0 + i, counter) for i in range(n)])


def rescaled(a, low, high):
    """``NormalizedVecEnv``'s rescale of the policy's action to the box
    ``[low, high]`` (``ga_action_rescale_f32``: fp32, one rounding per
    operation)."""
    f = np.float32
    a = np.asarray(a, dtype=f)
    slope = (f(0.5) * (f(high) - f(low))) / f(1.0)
    v = f(low) + (a + f(1.0)) * slope
    return np.clip(v, f(low), f(high)).astype(f)


class _Twins:
    """``n`` twins stepped together: the row's vectorised ``advance`` plus the
    episode bookkeeping of the twin's ``step`` / ``reset``."""

    def __init__(self, row, seed, id0, n, P, states):
        self.row, self.seed, self.id0, self.P = row, seed, id0, P
        self.state = states.copy()
        self.t = np.zeros(n, dtype=np.int64)
        self.resets = np.ones(n, dtype=np.int64)

    def step(self, actions):
        self.state, obs, rew, done = self.row.advance(self.state, actions)
        self.t += 1
        types_ = np.where(self.t >= self.P, TIMEOUT,
                          np.where(done, TERMINAL,
                                   np.where(self.t == 1, 0, 1)))
        return obs, rew, types_

    def reset(self, which):
        """Resets the members of ``which``; their new observations."""
        for i in np.nonzero(which)[0]:
            self.state[i] = self.row.reset_draw(self.seed, self.id0 + i,
                                                self.resets[i])
            self.resets[i] += 1
            self.t[i] = 0
        return self.row.observe(self.state[which])


class _TwinObjects:
    """``_Twins``' interface over ``n`` twin objects, each driven through its
    own ``step`` / ``reset``: for a kind with no vectorised ``advance`` that
    returns ``done``."""

    def __init__(self, row, seed, id0, n, P, states):
        self.row = row
        self.twins = [row.new_twin(seed=seed, env_id=id0 + i,
                                   max_episode_length=P) for i in range(n)]
        for i, twin in enumerate(self.twins):
            twin.resets = 1
            twin.state = states[i].copy()
        self.resets = np.ones(n, dtype=np.int64)

    @property
    def state(self):
        return np.stack([twin.state for twin in self.twins])

    @property
    def t(self):
        return np.asarray([twin._t for twin in self.twins])

    def step(self, actions):
        steps = [twin.step(actions[i:i + 1])
                 for i, twin in enumerate(self.twins)]
        return (np.stack([s.observation for s in steps]),
                np.asarray([s.reward for s in steps], dtype=np.float32),
                np.asarray([int(s.step_type) for s in steps]))

    def reset(self, which):
        self.resets += which
        obs = [self.twins[i].reset()[0] for i in np.nonzero(which)[0]]
        return np.stack(obs) if obs else np.zeros((0, self.row.obs_dim),
                                                  np.float32)


class _PythonSteps:
    """Mixed into a worker class: every step driven from Python."""

    def _native_steps(self, b, col, n_steps):
        return False


def scripted_starts(row, n, seed, id0):
    """The first states of a rollout of ``n`` envs: the reset draws, but the
    row's ``SCRIPTED`` states one step from an episode end in front."""
    states = draws(row, seed, id0, n)
    states[:row.SCRIPTED] = row.near_end(row.SCRIPTED)
    return states


def make(row, hidden, options=None, n=None, native=True, wrap=None,
         env_seed=21, id0=3, worker=None, worker_args=None, scripted=False):
    """A one-worker sampler over the row's batch and its worker.  ``scripted``:
    after the worker's own reset, which the next call then skips, the envs get
    ``scripted_starts``."""
    import torch
    from garage_amd.sampler import GpuVecSampler, GpuVecWorker
    n = row.N if n is None else n
    torch.manual_seed(5)
    env = inner = row.new_batch(n, max_episode_length=row.P, seed=env_seed,
                                env_id0=id0)
    if wrap is not None:
        env = wrap(env)
    pol = row.policy(env.spec, hidden_sizes=hidden, **row.rollout_policy_kw,
                     **(options or {}))
    with torch.no_grad():  # gamma / beta (the buffer's tail) away from (1, 0)
        if pol.net.ln_off:
            lo = pol.net.ln_off[0]
            pol.net.params[lo:].add_(
                torch.randn_like(pol.net.params[lo:]) * 0.05)
    base = worker or GpuVecWorker
    cls = base if native else type('PythonSteps', (_PythonSteps, base), {})
    s = GpuVecSampler(pol, env, max_episode_length=row.P, n_workers=1,
                      worker_class=cls, seed=2,
                      worker_args=dict(n_envs=n, **(worker_args or {})))
    w = s._workers[0]
    if scripted:
        w._start()
        inner.set_state(scripted_starts(row, n, env_seed, id0))
    return s, w


def host_batch(row):
    """A ``wrap`` for ``make``: the batch's task as a ``HostVecEnv`` of twins
    with its seed and member ids."""
    def wrap(env):
        from garage_amd.envs import HostVecEnv
        return HostVecEnv([row.new_twin(seed=env.seed, env_id=env.env_id0 + i,
                                        max_episode_length=row.P)
                           for i in range(env.n_envs)])
    return wrap


def normalized(**kw):
    """A ``wrap`` for ``make``: ``NormalizedVecEnv(env, **kw)``."""
    def wrap(env):
        from garage_amd.envs import NormalizedVecEnv
        return NormalizedVecEnv(env, **kw)
    return wrap


def one_launch_rollout(row, hidden, options, launches):
    """The native rollout of a fresh sampler (its batch on the host) after
    checking the whole-rollout launches of kinds (13, 14)."""
    import torch
    from garage_amd import _lib
    lib = _lib.load()
    s, w = make(row, hidden, options, scripted=bool(row.SCRIPTED))
    assert w._fused_ok()
    kinds = (GA_PROF_ROLLOUT, GA_PROF_ROLLOUT_WIDE)
    before = [int(lib.ga_launch_count(k)) for k in kinds]
    whole = w.rollout_samples(row.NUM).to_host()
    torch.cuda.synchronize()
    got = tuple(int(lib.ga_launch_count(k)) - b for k, b in zip(kinds, before))
    assert got == launches
    return whole


def normalized_statistics_inside_the_launch(row, n, nums):
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around a batch
    with a discrete action space: no rescale, so each call's first steps stay
    one launch; native against Python-driven steps, the calls of ``nums`` in a
    row.  The native batches, each already compared with its stepped one."""
    import torch
    from garage_amd import _lib
    lib = _lib.load()
    wrap = normalized(normalize_obs=True, normalize_reward=True,
                      obs_alpha=0.05, reward_alpha=0.05)
    out, counts = [], []
    for native in (True, False):
        s, w = make(row, (64, 64), n=n, native=native, wrap=wrap)
        assert w.env._act_low is None and w._fused_ok()
        before = int(lib.ga_launch_count(GA_PROF_ROLLOUT))
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate(nums)])
        torch.cuda.synchronize()
        counts.append(int(lib.ga_launch_count(GA_PROF_ROLLOUT)) - before)
    assert counts == [2, 0]  # one whole-rollout launch per native call
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
    return out[0]


def _member_vectors(pol, M, scale, log_std=None):
    """Visibly different parameters per member; ``log_std = (first, step)``
    sets the members' log-std (parameter 0 of a Gaussian policy)."""
    base = pol.get_flat_param_values()
    rng = np.random.RandomState(17)
    vectors = base[None] + scale * rng.randn(M, base.size).astype(np.float32)
    if log_std is not None and pol.kind == 'gaussian':
        vectors[:, 0] = np.log(log_std[0]) + log_std[1] * np.arange(M)
    return vectors.astype(np.float32)


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


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    m32 = 0xffffffff
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & m32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & m32)
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


def unit(word):
    """A Philox word as a float32 in (0, 1): its high 24 bits, centred."""
    f = np.float32
    return (f(word >> 8) + f(0.5)) * f(2.0**-24)


def reset_draw_py(row, seed, env_id, counter):
    """The row's reset draw restated on Python integers: ``draw_blocks``
    Philox blocks at ``(env_id, counter, block, stream << 16)`` under the key
    ``seed``, their words mapped to a state by ``draw_from_words``."""
    key = (seed & 0xffffffff, seed >> 32)
    words = ()
    for block in range(row.draw_blocks):
        words += philox4x32_10((env_id & 0xffffffff, counter, block,
                                row.stream << 16), key)
    return np.asarray(row.draw_from_words(words), dtype=np.float32)


def random_draw_cases():
    """Five hand-picked ``(seed, env_id, counter)`` and 400 random ones with
    seeds above 2^32."""
    rng = np.random.RandomState(2)
    cases = [(0, 0, 0), (0, 1, 0), (0, 0, 1), ((7 << 32) | 11, 5, 3),
             (3, (1 << 32) + 2, 9)]
    cases += [(int(rng.randint(0, 1 << 30)) << 20 | int(rng.randint(1 << 20)),
               int(rng.randint(0, 1 << 20)), int(rng.randint(0, 1 << 16)))
              for _ in range(400)]
    assert any(seed >> 32 for seed, _, _ in cases)
    return cases


def grid_draw_cases():
    """Two seeds x three env ids x three counters, the ends of each range
    included."""
    return [(seed, env_id, counter) for seed in (0, (7 << 32) | 11)
            for env_id in (0, 1, 1 << 31)
            for counter in (0, 1, (1 << 32) - 1)]


def _layout_lines(cname, py, kind_macro):
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%d\\n", {});'.format(kind_macro),
             'printf("{0} %zu\\n", sizeof({0}));'.format(cname)]
    want = ['{} {}'.format(cname, ctypes.sizeof(py))]
    for field, ftype in py._fields_:
        lines.append('printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                     'sizeof((({0}*)0)->{1}));'.format(cname, field))
        want.append('{}.{} {} {}'.format(cname, field,
                                         getattr(py, field).offset,
                                         ctypes.sizeof(ftype)))
    lines += ['return 0;', '}']
    return lines, want
