"""GPU sampler and worker with garage's Sampler / Worker plugin surface.

Replaces ``LocalSampler`` + ``VecWorker`` (``sampler/local_sampler.py:13-232``,
``sampler/vec_worker.py:12-228``, ``sampler/worker_factory.py:24-116``,
``sampler/_functions.py:6-40``).  The per-env Python loop becomes a handful of
kernel launches per step over env-major ``(n_envs, Tcap)`` rollout buffers in
HBM; episode bookkeeping (lengths, completion order, step types, the reset of
finished envs, the discard of in-flight episodes at each ``obtain_samples``)
follows the reference exactly and is verified bit for bit against it.
"""
import copy
import warnings
import ctypes as C

import numpy as np
import torch

from garage_amd import _lib
from garage_amd._dtypes import (DeviceEpisodeBatch, DevicePopulationBatch,
                               EpisodeBatch, EpisodeStatistics, is_discrete)
from garage_amd._lib import call, dptr, stream_ptr
from garage_amd.engine import require_gpu, round4
from garage_amd.envs import (HostVecEnv, NormalizedVecEnv, VecEnv,
                             _DeviceVecEnv)


def _identity(value):
    return value


class WorkerFactory:
    """``sampler/worker_factory.py:24-116`` (picklable worker constructor)."""

    def __init__(self, *, max_episode_length, is_tf_worker=False, seed=None,
                 n_workers=1, worker_class=None, worker_args=None):
        if is_tf_worker:
            raise NotImplementedError('TensorFlow workers are out of scope')
        self.n_workers = n_workers
        self._seed = seed
        self._max_episode_length = max_episode_length
        self._worker_class = worker_class or GpuVecWorker
        self._worker_args = {} if worker_args is None else worker_args

    def prepare_worker_messages(self, objs, preprocess=_identity):
        if isinstance(objs, list):
            if len(objs) != self.n_workers:
                raise ValueError(
                    'Length of list doesn\'t match number of workers')
            return [preprocess(obj) for obj in objs]
        return [preprocess(objs) for _ in range(self.n_workers)]

    def __call__(self, worker_number):
        if worker_number >= self.n_workers:
            raise ValueError('Worker number is too big')
        return self._worker_class(worker_number=worker_number,
                                  seed=self._seed,
                                  max_episode_length=self._max_episode_length,
                                  **self._worker_args)


class EnvUpdate:
    """``sampler/env_update.py:5-33``: a callable ``old_env -> env``; the caller
    uses what it returns and forgets ``old_env``.  The base class keeps it."""

    def __call__(self, old_env=None):
        return old_env


class NewEnvUpdate(EnvUpdate):
    """``env_update.py:36-63``: closes the old environment and constructs a new
    one with ``env_constructor()`` at every update."""

    def __init__(self, env_constructor):
        self._env_constructor = env_constructor

    def __call__(self, old_env=None):
        if old_env:
            old_env.close()
        return self._env_constructor()


class SetTaskUpdate(EnvUpdate):
    """``env_update.py:66-121``: ``set_task(task)`` on an environment of type
    ``env_type``, constructing (and wrapping) one when the old environment is
    missing or of another type."""

    def __init__(self, env_type, task, wrapper_constructor):
        if not isinstance(env_type, type):
            raise ValueError('env_type should be a type, not '
                             f'{type(env_type)!r}')
        self._env_type = env_type
        self._task = task
        self._wrapper_cons = wrapper_constructor

    def _make_env(self):
        env = self._env_type()
        env.set_task(self._task)
        if self._wrapper_cons is not None:
            env = self._wrapper_cons(env, self._task)
        return env

    def __call__(self, old_env=None):
        if old_env is None:
            return self._make_env()
        if not isinstance(getattr(old_env, 'unwrapped', old_env),
                          self._env_type):
            warnings.warn('SetTaskEnvUpdate is closing an environment. This '
                          'may indicate a very slow TaskSampler setup.')
            old_env.close()
            return self._make_env()
        old_env.set_task(self._task)
        return old_env


class ExistingEnvUpdate(EnvUpdate):
    """``env_update.py:124-159``: hands over an environment that already
    exists; the old one is not closed."""

    def __init__(self, env):
        self._env = env

    def __call__(self, old_env=None):
        return self._env

    def __getstate__(self):
        warnings.warn('ExistingEnvUpdate is generally not the most efficient '
                      'method of transmitting environments to other '
                      'processes.')
        return self.__dict__


def _is_environment(obj):
    return hasattr(obj, 'step') and hasattr(obj, 'reset')


def _apply_env_update(old_env, env_update):
    """``sampler/_functions.py:6-40``: ``(env, updated)``; ``None`` keeps the
    environment, an :class:`EnvUpdate` is called on it, an environment replaces
    it (the old one is closed), anything else is a ``TypeError``."""
    if env_update is None:
        return old_env, False
    if isinstance(env_update, EnvUpdate):
        return env_update(old_env), True
    if _is_environment(env_update):
        if old_env is not None:
            old_env.close()
        return env_update, True
    raise TypeError('Unknown environment update type.')


def check_cells_int32(n_envs, tcap):
    """The packing path addresses the cell ``env * tcap + column`` of a rollout
    buffer in int32 (``ga_pack_src_index``, the gathers, ``ep_cell``): refuse
    buffers with ``2^31`` cells or more before anything is allocated."""
    n_envs, tcap = int(n_envs), int(tcap)
    if n_envs * tcap >= 2**31:
        raise ValueError(
            'rollout buffers too large: {} envs x {} columns = {} cells, and '
            'cells are addressed in int32 (fewer than 2^31); use fewer envs or '
            'ask for fewer samples per call'.format(n_envs, tcap,
                                                    n_envs * tcap))


def _copy_env(env):
    """``copy.deepcopy`` for per-env objects; device batches are shared."""
    return env if isinstance(env, VecEnv) else copy.deepcopy(env)


class GpuVecWorker:
    """``VecWorker`` whose ``n_envs`` environments live on the GPU.

    ``update_env`` accepts a :class:`~garage_amd.envs.VecEnv` (used as is), a
    list of exactly ``n_envs`` per-env objects or a single per-env object that
    is deep-copied ``n_envs`` times (``vec_worker.py:75-105``) -- the latter two
    are wrapped in :class:`~garage_amd.envs.HostVecEnv`.
    """

    DEFAULT_N_ENVS = 8

    def __init__(self, *, seed, max_episode_length, worker_number,
                 n_envs=DEFAULT_N_ENVS, noise_fn=None, store_agent_infos=True,
                 fused_policy_step=True):
        self._use_fused = bool(fused_policy_step)
        self._seed = seed
        self._max_episode_length = max_episode_length
        self._worker_number = worker_number
        self._n_envs = n_envs
        self._noise_fn = noise_fn  # test hook: step -> (n, A) noise tensor
        self._store_infos = store_agent_infos
        self.agent = None
        self.env = None
        self._needs_agent_reset = True
        self._needs_env_reset = True
        self._ep_t = None
        self._global_step = 0
        self._pending = []  # API-compat path: completed episode batches
        self.device = require_gpu()
        if seed is not None:
            # default_worker.py:50-53: seed the *global* RNGs per worker
            import random
            s = seed + worker_number
            random.seed(s)
            np.random.seed(s)
            torch.manual_seed(s)

    # -- updates --------------------------------------------------------------
    def update_agent(self, agent_update):
        """``default_worker.py:55-69`` + ``vec_worker.py:61-73``."""
        if isinstance(agent_update, (dict, tuple, np.ndarray)):
            self.agent.set_param_values(agent_update)
        elif agent_update is not None:
            self.agent = agent_update
        self._needs_agent_reset = True

    def update_env(self, env_update):
        """``vec_worker.py:75-105``.  A :class:`~garage_amd.envs.VecEnv` replaces
        the batch as a whole (so does a plain callable ``VecEnv -> VecEnv``, for
        device-resident batches); a list holds one update per environment --
        ``None``, an environment or an :class:`EnvUpdate` each; a single
        environment or :class:`EnvUpdate` is deep-copied ``n_envs`` times."""
        if env_update is None:
            return
        n = self._n_envs
        if isinstance(env_update, VecEnv) or (
                callable(env_update) and not isinstance(env_update, EnvUpdate)
                and not _is_environment(env_update)):
            new_env = (env_update if isinstance(env_update, VecEnv) else
                       env_update(self.env))
            if new_env.n_envs != n:
                raise ValueError('If separate environments are passed for '
                                 'each worker, there must be exactly n_envs '
                                 '({}) environments, but received {} '
                                 'environments.'.format(n, new_env.n_envs))
            if self.env is not None and self.env is not new_env:
                self.env.close()
            self.env = new_env
            self._needs_env_reset = True
            return
        if isinstance(env_update, list):
            if len(env_update) != n:
                raise ValueError('If separate environments are passed for '
                                 'each worker, there must be exactly n_envs '
                                 '({}) environments, but received {} '
                                 'environments.'.format(n, len(env_update)))
        else:
            env_update = [copy.deepcopy(env_update) for _ in range(n)]
        old = (list(self.env.envs) if isinstance(self.env, HostVecEnv)
               else [None] * n)
        members, updated = [], False
        for old_env, env_up in zip(old, env_update):
            env, up = _apply_env_update(old_env, env_up)
            members.append(env)
            updated = updated or up
        if not updated:
            return
        if any(m is None for m in members):
            raise TypeError('Unknown environment update type.')
        if self.env is not None and not isinstance(self.env, HostVecEnv):
            self.env.close()  # a device batch gives way to per-env objects
        # (the members of a previous HostVecEnv were kept, replaced or closed
        # one by one above: the batch object itself owns only staging buffers)
        self.env = HostVecEnv(members)
        self._needs_env_reset = True

    # -- rollout buffers ------------------------------------------------------
    def _alloc_buffers(self, num_samples, n_share=None):
        """Rollout buffers of all the envs; ``n_share``: how many of them work
        towards one ``num_samples`` target (default: all; a population member's
        envs)."""
        env, n = self.env, self._n_envs
        P = int(self._max_episode_length)
        # the last step t* satisfies t* <= ceil(num_samples / n) + P - 2
        tcap = -(-int(num_samples) // (n_share or n)) + P - 1
        tcap = round4(max(tcap, 1))
        if tcap > 65535 * 4:
            raise ValueError('rollout too long for one obtain_samples call')
        check_cells_int32(n, tcap)
        dev = self.device
        ldo = round4(env.obs_dim)
        lda = round4(env.act_width)
        ldh = round4(self.agent.net.out_dim)
        f32 = torch.float32
        b = {
            'Tcap': tcap,
            'obs': torch.empty(n, tcap, ldo, dtype=f32, device=dev),
            'act': torch.empty(n, tcap, lda, dtype=f32, device=dev),
            'head': (torch.empty(n, tcap, ldh, dtype=f32, device=dev)
                     if self._store_infos else None),
            'lastobs': torch.empty(n, tcap, ldo, dtype=f32, device=dev),
            'rew': torch.empty(n, tcap, dtype=f32, device=dev),
            'st': torch.empty(n, tcap, dtype=torch.uint8, device=dev),
            'tail': torch.zeros(n, tcap, dtype=torch.uint16, device=dev),
            'step_eps': torch.zeros(tcap, dtype=torch.int32, device=dev),
            'step_samples': torch.zeros(tcap, dtype=torch.int32, device=dev),
            'action': torch.zeros(n, lda, dtype=f32, device=dev),
            'done': torch.zeros(n, dtype=torch.uint8, device=dev),
            # per column: the n ``env_info`` dicts of a CPU env batch (or None)
            'infos': [None] * tcap,
            # column -> {env index: episode_info} for the episodes that ended
            # there (CPU env batches whose resets report any)
            'ep_infos': {},
            # per-step env_infos a device env batch writes on the GPU
            'dev_infos': {k: torch.zeros(n, tcap, dtype=torch.uint8, device=dev)
                          for k in env.env_info_specs},
        }
        if ldo != env.obs_dim:
            b['obs'].zero_()      # padding columns feed the GEMMs: keep them 0
            b['lastobs'].zero_()
        if lda != env.act_width:
            b['act'].zero_()
        return b

    def _start(self):
        """``vec_worker.py:107-137``: reset on agent / env update."""
        if not (self._needs_agent_reset or self._needs_env_reset):
            return
        self.agent.reset([True] * self._n_envs)
        if self._needs_env_reset or self._ep_t is None:
            self.env.reset_all()
            self._ep_t = torch.zeros(self._n_envs, dtype=torch.int32,
                                     device=self.device)
        else:
            # only environments with progress are reset (vec_worker.py:122-126)
            progress = (self._ep_t > 0).to(torch.uint8)
            self.env.hold()
            self.env.reset_where(progress)
            self.env.advance()
            self._ep_t.zero_()
        pop = getattr(self.env, 'pop_finished_episode_infos', None)
        if pop is not None:
            pop()  # episodes dropped by the reset are not part of any batch
        self._needs_agent_reset = False
        self._needs_env_reset = False

    def _step(self, b, col):
        """One vectorised step into column ``col`` of the rollout buffers."""
        env, pol, n = self.env, self.agent, self._n_envs
        fused = self._fused_ok()
        a = self._head_args(b, col, fused)
        s = stream_ptr()
        if fused:
            call('ga_policy_step_fused_f32', C.byref(pol.net._desc),
                 dptr(pol.net.params), C.byref(a), s)
        else:
            call('ga_policy_head_sample', C.byref(a), s)
        env.step_all(b['action'])
        b['infos'][col] = getattr(env, 'last_env_infos', None)
        for key, val in env.step_env_infos().items():
            b['dev_infos'][key][:, col] = val
        r = self._record_args(b, col)
        call('ga_record_step', C.byref(r), s)
        env.reset_where(b['done'])
        pop = getattr(env, 'pop_finished_episode_infos', None)
        if pop is not None:
            finished = pop()
            if finished:
                b['ep_infos'][col] = dict(finished)
        env.advance()
        self._global_step += 1

    def _fused_ok(self):
        # (layer inputs up to 256: the resident-weights kernels; up to 512: the
        # wide one)
        lib, desc = _lib.load(), C.byref(self.agent.net._desc)
        return self._use_fused and bool(
            lib.ga_policy_step_fused_supported(desc)
            or lib.ga_policy_step_wide_supported(desc))

    def _head_args(self, b, col, fused):
        env, pol, n = self.env, self.agent, self._n_envs
        a = _lib.HeadArgs()
        a.n, a.env_id0 = n, getattr(env, 'env_id0', 0)
        a.kind = 0 if pol.kind == 'gaussian' else 1
        a.A = pol.net.out_dim
        if fused:
            a.ldh = round4(pol.net.out_dim)
        else:
            head = pol.net.forward(env.obs, n)
            a.head, a.ldh = head.data_ptr(), head.stride(0)
        if pol.kind == 'gaussian':
            a.log_std = pol.net.log_std.data_ptr()
            a.has_min, a.min_log_std, a.has_max, a.max_log_std = \
                pol._std_args()
        else:
            a.double_softmax = int(pol.double_softmax)
        noise = self._noise_fn(self._global_step) if self._noise_fn else None
        if noise is not None:
            self._noise_keepalive = noise
            a.noise, a.ldn = noise.data_ptr(), noise.stride(0)
        a.seed = (self._seed or 0) + 7919 * (self._worker_number + 1)
        a.step = self._global_step & 0xFFFFFFFF
        a.obs, a.ldo, a.obs_dim = (env.obs.data_ptr(), env.obs.stride(0),
                                   env.obs_dim)
        a.col, a.Tcap = col, b['Tcap']
        a.action, a.lda = b['action'].data_ptr(), b['action'].stride(0)
        a.obs_buf, a.act_buf = b['obs'].data_ptr(), b['act'].data_ptr()
        a.head_buf = b['head'].data_ptr() if b['head'] is not None else None
        return a

    def _record_args(self, b, col):
        env, n = self.env, self._n_envs
        r = _lib.RecordArgs()
        r.n, r.col, r.Tcap = n, col, b['Tcap']
        r.max_episode_length = int(self._max_episode_length)
        r.reward, r.step_type = env.reward.data_ptr(), env.step_type.data_ptr()
        r.next_obs, r.ldo, r.obs_dim = (env.next_obs.data_ptr(),
                                        env.next_obs.stride(0), env.obs_dim)
        r.ep_t = self._ep_t.data_ptr()
        r.rew_buf, r.st_buf = b['rew'].data_ptr(), b['st'].data_ptr()
        r.tail_buf, r.lastobs_buf = (b['tail'].data_ptr(),
                                     b['lastobs'].data_ptr())
        r.done = b['done'].data_ptr()
        r.step_eps = b['step_eps'].data_ptr()
        r.step_samples = b['step_samples'].data_ptr()
        r.terminal_only = getattr(self, '_terminal_only', 0)
        return r

    def _native_steps(self, b, col, n_steps):
        """``n_steps`` steps enqueued by ``ga_rollout_env_steps`` (device env
        batches): fused policy step, device RNG; False when not applicable."""
        from garage_amd.envs import NormalizedVecEnv
        env = self.env
        inner, norm = env, None
        if type(env) is NormalizedVecEnv:  # statistics fused into the env step
            inner, norm = env._env, env.norm_args()
        ref = inner.native_env_ref(b['dev_infos'])
        if (n_steps <= 0 or ref is None or self._noise_fn is not None
                or not self._fused_ok()):
            return False
        env_ref, _keepalive = ref
        a = self._head_args(b, col, True)
        r = self._record_args(b, col)
        raw = norm is not None and norm.normalize_obs
        call('ga_rollout_env_steps', C.byref(self.agent.net._desc),
             dptr(self.agent.net.params), C.byref(a), C.byref(env_ref),
             C.byref(r), dptr(env.obs), dptr(env.next_obs),
             None if norm is None else C.byref(norm),
             dptr(inner.obs) if raw else None,
             dptr(inner.next_obs) if raw else None, n_steps, stream_ptr())
        if n_steps % 2:
            env.advance()
        self._global_step += n_steps
        return True

    def rollout_samples(self, num_samples):
        """Everything ``LocalSampler.obtain_samples`` collects from one worker.

        Steps until the episodes completed so far hold ``>= num_samples``
        transitions, exactly like the ``while True: worker.rollout()`` loop of
        ``local_sampler.py:157-166`` (in-flight episodes at that point are
        dropped by the next call's reset).
        """
        self._start()
        n = self._n_envs
        # the reference loop runs at least one rollout(), i.e. until an episode
        # completes, whatever the target (local_sampler.py:157-166)
        num_samples = max(int(num_samples), 1)
        b = self._alloc_buffers(num_samples)
        col = 0
        # the target cannot be reached before step ceil(num_samples / n): those
        # steps need no host check and are enqueued natively when possible
        first_check = min(-(-int(num_samples) // n), b['Tcap'])
        if self._native_steps(b, 0, first_check):
            col = first_check
        while True:
            if col > 0 and col * n >= num_samples:  # cannot be reached any earlier
                done_samples = int(b['step_samples'][:col].sum().item())
                if done_samples >= num_samples:
                    break
            if col >= b['Tcap']:
                raise RuntimeError('rollout buffer exhausted: an environment '
                                   'ran past max_episode_length')
            self._step(b, col)
            col += 1
        return self._pack(b, col)

    @staticmethod
    def _env_rows(b, lo, hi, step_eps):
        """The rollout buffers of the envs ``[lo, hi)`` alone (views), with the
        episodes THEY finished per column (``step_eps``, counted from their
        ``tail`` rows by the caller)."""
        out = dict(b)
        for k in ('obs', 'act', 'head', 'lastobs', 'rew', 'st', 'tail'):
            if b[k] is not None:
                out[k] = b[k][lo:hi]
        out['dev_infos'] = {k: v[lo:hi] for k, v in b['dev_infos'].items()}
        out['step_eps'] = step_eps
        return out

    def _pack(self, b, n_steps, first_step=0, member=None):
        """Episodes that ended in columns ``[first_step, n_steps)`` -> batch; with
        ``member = (lo, hi, step_eps, log_std)`` those of the envs ``[lo, hi)``
        only: a population member's, with its own episode counts per column (a
        host tensor) and its own clamped log-std."""
        lo, hi, log_std = 0, self._n_envs, None
        if member is not None:
            lo, hi, step_eps, log_std = member
            b = self._env_rows(b, lo, hi, step_eps)
        dev, n, tcap = self.device, hi - lo, b['Tcap']
        step_eps = b['step_eps'][:n_steps].cpu().numpy().astype(np.int64)
        step_eps[:first_step] = 0
        ep_base = np.concatenate([[0], np.cumsum(step_eps)[:-1]])
        n_eps = int(step_eps.sum())
        s = stream_ptr()
        ep_env = torch.empty(n_eps, dtype=torch.int32, device=dev)
        ep_end = torch.empty_like(ep_env)
        ep_len = torch.empty_like(ep_env)
        base_dev = torch.from_numpy(ep_base.astype(np.int32)).to(dev)
        # columns before first_step are skipped by offsetting the column base
        tail = b['tail'][:, first_step:]
        call('ga_pack_episodes', dptr(tail), n, tcap, n_steps - first_step,
             dptr(base_dev[first_step:]), dptr(ep_env), dptr(ep_end),
             dptr(ep_len), s)
        if first_step:
            ep_end += first_step
        lengths = ep_len.cpu().numpy().astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lengths)])
        S = int(off[-1])
        off_dev = torch.from_numpy(off).to(dev)
        src = torch.empty(S, dtype=torch.int32, device=dev)
        call('ga_pack_src_index', dptr(ep_env), dptr(ep_end), dptr(ep_len),
             dptr(off_dev), n_eps, tcap, dptr(src), s)
        ep_cell = (ep_env.long() * tcap + ep_end.long()).to(torch.int32)

        def rows(buf, idx, count):
            w = buf.shape[-1]
            out = torch.empty(count, w, dtype=torch.float32, device=dev)
            call('ga_gather_rows_f32', dptr(buf), w, dptr(idx), count, w,
                 dptr(out), w, s)
            return out

        obs = rows(b['obs'], src, S)
        act = rows(b['act'], src, S)
        head = rows(b['head'], src, S) if b['head'] is not None else None
        last = rows(b['lastobs'], ep_cell, n_eps)
        rew = torch.empty(S, dtype=torch.float32, device=dev)
        call('ga_gather_f32', dptr(b['rew']), dptr(src), S, dptr(rew), s)
        st = torch.empty(S, dtype=torch.uint8, device=dev)
        call('ga_gather_u8', dptr(b['st']), dptr(src), S, dptr(st), s)
        pol = self.agent
        gaussian = pol.kind == 'gaussian'
        env_infos, episode_infos = self._device_infos(
            b, src, ep_env, ep_end, self._packed_env_infos(b, src, tcap),
            self._packed_episode_infos(b, ep_env, ep_end), env0=lo)
        if gaussian and log_std is None:
            log_std = pol.clamped_log_std()
        return DeviceEpisodeBatch(
            self.env.spec, lengths=lengths, obs_dev=obs, last_obs_dev=last,
            actions_dev=act, rewards_dev=rew, step_types_dev=st,
            ep_off_dev=off_dev, head_dev=head,
            head_name='mean' if gaussian else 'prob',
            log_std=log_std if gaussian else None,
            discrete=is_discrete(self.env.spec.action_space),
            env_infos=env_infos, episode_infos=episode_infos)

    def _device_infos(self, b, src, ep_env, ep_end, env_infos, episode_infos,
                      env0=0):
        """Adds the env_infos a device env batch recorded (gathered by the
        samples' cells ``src``), the keys the batch derives from them on the
        host, and its episode_infos (by member ``ep_env``; a batch may ask for
        a recorded env_info at each episode's or fragment's last cell
        ``(ep_env, ep_end)``, gathered only then).  ``env0``: the batch member
        that row 0 of ``b`` belongs to."""
        specs, s = self.env.env_info_specs, stream_ptr()

        def gather(key, idx):
            count = int(idx.numel())
            out = torch.empty(count, dtype=torch.uint8, device=self.device)
            if count:
                call('ga_gather_u8', dptr(b['dev_infos'][key]), dptr(idx),
                     count, dptr(out), s)
            return out.cpu().numpy().astype(specs[key])

        def info_at_end(key):
            cell = (ep_env.long() * b['Tcap'] + ep_end.long()).to(torch.int32)
            return gather(key, cell)

        for key in b['dev_infos']:
            env_infos[key] = gather(key, src)
        if b['dev_infos']:
            self.env.finish_env_infos(env_infos)
        episode_infos.update(self.env.episode_infos_of(
            ep_env + env0 if env0 else ep_env, info_at_end))
        return env_infos, episode_infos

    @staticmethod
    def _packed_episode_infos(b, ep_env, ep_end):
        """``episode_infos`` of the packed batch: per key an ``(N, ...)`` array,
        row ``e`` = what ``reset()`` reported for episode ``e``
        (``default_worker.py:94-96,158-161``; the reference's ``VecWorker`` loses
        them after an env's first episode, SURVEY.md Q23 -- the intended
        ``DefaultWorker`` layout is kept here)."""
        log = b.get('ep_infos')
        if not log or not any(info for col in log.values()
                              for info in col.values()):
            return {}
        envs = ep_env.cpu().numpy()
        ends = ep_end.cpu().numpy()
        rows = [log.get(int(c), {}).get(int(e), {})
                for e, c in zip(envs, ends)]
        keys = next(r for r in rows if r).keys()
        for e, r in enumerate(rows):
            missing = [k for k in keys if k not in r]
            if missing:
                # (the reference's EpisodeBatch.concatenate needs every episode
                # to carry the same episode_info keys, _dtypes.py:592-632)
                raise ValueError(
                    'episode {} (env {}, ended at step {}) reports no '
                    'episode_info {!r}; every reset() of a batch must report '
                    'the same keys'.format(e, int(envs[e]), int(ends[e]),
                                           missing))
        return {k: np.asarray([r[k] for r in rows]) for k in keys}

    @staticmethod
    def _packed_env_infos(b, src, tcap):
        """``env_infos`` of the packed batch: per key an ``(S, ...)`` array in the
        same sample order as the device arrays (``vec_worker.py:146-147,192-193``
        builds the same arrays per episode).  Only CPU env batches report any."""
        log = b.get('infos')
        if not log or all(entry is None for entry in log):
            return {}
        cells = src.cpu().numpy().astype(np.int64)  # env * tcap + column
        envs, cols = cells // tcap, cells % tcap
        first = log[int(cols[0])][int(envs[0])] if cells.size else {}
        out = {}
        for key in first:
            out[key] = np.asarray([log[int(c)][int(e)][key]
                                   for e, c in zip(envs, cols)])
        return out

    # -- reference-shaped API (sampler/worker.py:46-77) -------------------------
    # start_episode / step_episode / collect_episode run on one persistent
    # rollout buffer: a step is the same launches as everywhere else plus ONE
    # device sync (the count of episodes that ended in it), collect_episode packs
    # the columns stepped since the last collection.  rollout() is the three
    # calls in the reference's order (default_worker.py:176-186).
    def start_episode(self):
        """``vec_worker.py:107-137``."""
        self._start()

    def _api_buffer(self):
        if getattr(self, '_api_buf', None) is None:
            P = int(self._max_episode_length)
            self._api_buf = self._alloc_buffers(self._n_envs * P)
            self._api_col = 0    # next column to step into
            self._api_first = 0  # first column not yet handed out
        return self._api_buf

    def step_episode(self):
        """``vec_worker.py:176-204``: one vectorised step of every environment;
        True iff at least one episode completed in it."""
        if self._ep_t is None:
            self._start()
        b = self._api_buffer()
        if self._api_col >= b['Tcap']:
            b = self._api_buf = self._grown(b, self._api_col)
        col = self._api_col
        self._step(b, col)
        self._api_col = col + 1
        return int(b['step_eps'][col].item()) > 0

    def collect_episode(self):
        """``vec_worker.py:206-219``: the episodes completed since the last call,
        in (completion step, env) order."""
        b = self._api_buffer()
        first, col = self._api_first, self._api_col
        if col <= first or int(b['step_eps'][first:col].sum().item()) == 0:
            # (the reference falls into EpisodeBatch.concatenate() of nothing)
            raise ValueError('collect_episode(): no episode has completed '
                             'since the last call')
        batch = self._pack(b, col, first_step=first)
        self._api_first = col
        if col + int(self._max_episode_length) >= b['Tcap']:
            self._rebase_api_buffer()
        return batch

    def rollout(self):
        """``default_worker.py:176-186``: step until an episode completes."""
        self.start_episode()
        while not self.step_episode():
            pass
        return self.collect_episode()

    def _rebase_api_buffer(self):
        """Move the in-flight tails of the API buffer back to column 0 (every
        completed episode has been handed out: called by collect_episode)."""
        old, col = self._api_buf, self._api_col
        P = int(self._max_episode_length)
        new = self._alloc_buffers(self._n_envs * P)
        keep = min(col, P)
        for k in ('obs', 'act', 'head', 'lastobs', 'rew', 'st'):
            if old[k] is not None:
                new[k][:, :keep] = old[k][:, col - keep:col]
        new['infos'][:keep] = old['infos'][col - keep:col]
        for k, v in old['dev_infos'].items():
            new['dev_infos'][k][:, :keep] = v[:, col - keep:col]
        new['ep_infos'] = {c - (col - keep): v
                           for c, v in old['ep_infos'].items()
                           if c >= col - keep}
        self._api_buf, self._api_col, self._api_first = new, keep, keep

    def _grown(self, old, col):
        """A rollout buffer of twice the columns holding columns ``[0, col)`` of
        ``old`` (steps taken without a collection in between)."""
        new = self._alloc_buffers(self._n_envs * 2 * old['Tcap'])
        for k in ('obs', 'act', 'head', 'lastobs', 'rew', 'st', 'tail'):
            if old[k] is not None:
                new[k][:, :col] = old[k][:, :col]
        for k in ('step_eps', 'step_samples'):
            new[k][:col] = old[k][:col]
        new['infos'][:col] = old['infos'][:col]
        for k, v in old['dev_infos'].items():
            new['dev_infos'][k][:, :col] = v[:, :col]
        new['ep_infos'] = dict(old['ep_infos'])
        return new

    def shutdown(self):
        if self.env is not None:
            self.env.close()

    def __getstate__(self):
        """Workers are not picklable (``sampler/worker.py:79-87``)."""
        raise ValueError('Workers are not pickleable. '
                         'Please pickle the WorkerFactory instead.')


class GpuFragmentWorker(GpuVecWorker):
    """``FragmentWorker`` (``sampler/fragment_worker.py:11-156``) on the GPU.

    Each ``rollout()`` advances every env by ``timesteps_per_call`` steps and
    returns *fragments*: the pieces of episodes collected during the call, cut
    at episode ends and at the end of the call.  Fragments that ended with their
    episode come first, in (step, env) order; the still-running ones follow in
    env order (``collect_episode``, ``:121-138``).  Episodes continue across
    calls (``update_agent`` does not reset them) and only TERMINAL -- not
    TIMEOUT -- or ``max_episode_length`` ends one (``:114-115``).
    """

    def __init__(self, *, seed, max_episode_length, worker_number,
                 n_envs=GpuVecWorker.DEFAULT_N_ENVS, timesteps_per_call=1,
                 noise_fn=None, store_agent_infos=True):
        super().__init__(seed=seed, max_episode_length=max_episode_length,
                         worker_number=worker_number, n_envs=n_envs,
                         noise_fn=noise_fn,
                         store_agent_infos=store_agent_infos)
        self._timesteps_per_call = int(timesteps_per_call)
        self._terminal_only = 1

    def update_agent(self, agent_update):
        """``default_worker.py:55-69``: no reset flag for fragment workers."""
        if isinstance(agent_update, (dict, tuple, np.ndarray)):
            self.agent.set_param_values(agent_update)
        elif agent_update is not None:
            self.agent = agent_update

    def _start(self):
        """``fragment_worker.py:89-96``: only an env update restarts episodes."""
        if self._needs_env_reset or self._ep_t is None:
            self.agent.reset([True] * self._n_envs)
            self.env.reset_all()
            self._ep_t = torch.zeros(self._n_envs, dtype=torch.int32,
                                     device=self.device)
        self._needs_agent_reset = False
        self._needs_env_reset = False

    def rollout_samples(self, num_samples):
        raise NotImplementedError('fragment workers are driven by rollout()')

    def start_episode(self):
        """``fragment_worker.py:85-91``."""
        self._start()

    def step_episode(self):
        """``fragment_worker.py:93-119``: one step of every environment; True
        iff an episode ended (TERMINAL or ``max_episode_length``) in it."""
        if self._ep_t is None:
            self._start()
        b = getattr(self, '_frag_buf', None)
        if b is None:
            b = self._frag_buf = self._alloc_buffers(
                self._n_envs * self._timesteps_per_call)
            self._frag_col = 0
        if self._frag_col >= b['Tcap']:
            b = self._frag_buf = self._grown(b, self._frag_col)
        col = self._frag_col
        self._step(b, col)
        self._frag_col = col + 1
        return int(b['step_eps'][col].item()) > 0

    def collect_episode(self):
        """``fragment_worker.py:121-138``: the fragments closed by an episode end
        since the last call in (step, env) order, then the still-running ones
        in env order."""
        b, tpc = getattr(self, '_frag_buf', None), getattr(self, '_frag_col', 0)
        if b is None or tpc == 0:
            raise ValueError('collect_episode(): no step has been taken since '
                             'the last call')
        n = self._n_envs
        self._frag_buf, self._frag_col = None, 0
        # fragment table on the host: the (n, tpc) tail matrix is tiny
        tail = b['tail'][:, :tpc].to(torch.int32).cpu().numpy()
        env_id, end, length = [], [], []
        cut = np.zeros(n, dtype=np.int64)  # first column of the open fragment
        for t in range(tpc):               # fragments closed by an episode end
            for i in np.nonzero(tail[:, t])[0]:
                env_id.append(i)
                end.append(t)
                length.append(t - cut[i] + 1)
                cut[i] = t + 1
        n_closed = len(env_id)
        for i in range(n):                 # still-running fragments, env order
            if cut[i] < tpc:
                env_id.append(i)
                end.append(tpc - 1)
                length.append(tpc - cut[i])
        return self._pack_fragments(b, np.asarray(env_id), np.asarray(end),
                                    np.asarray(length), n_closed)

    def rollout(self):
        """``fragment_worker.py:140-151``."""
        self.start_episode()
        for _ in range(self._timesteps_per_call):
            self.step_episode()
        return self.collect_episode()

    def _pack_fragments(self, b, env_id, end, length, n_closed):
        dev, tcap = self.device, b['Tcap']
        s = stream_ptr()
        n_frag = len(env_id)
        ep_env = torch.from_numpy(env_id.astype(np.int32)).to(dev)
        ep_end = torch.from_numpy(end.astype(np.int32)).to(dev)
        ep_len = torch.from_numpy(length.astype(np.int32)).to(dev)
        off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
        S = int(off[-1])
        off_dev = torch.from_numpy(off).to(dev)
        src = torch.empty(S, dtype=torch.int32, device=dev)
        call('ga_pack_src_index', dptr(ep_env), dptr(ep_end), dptr(ep_len),
             dptr(off_dev), n_frag, tcap, dptr(src), s)

        def rows(buf, idx, count, ld=None):
            w = buf.shape[-1]
            out = torch.empty(count, w, dtype=torch.float32, device=dev)
            call('ga_gather_rows_f32', dptr(buf), w, dptr(idx), count, w,
                 dptr(out), w, s)
            return out

        obs = rows(b['obs'], src, S)
        act = rows(b['act'], src, S)
        head = rows(b['head'], src, S) if b['head'] is not None else None
        # last observation: the terminal one for closed fragments, the env's
        # current observation for the running ones
        last = torch.empty(n_frag, obs.shape[1], dtype=torch.float32,
                           device=dev)
        if n_closed:
            cell = (ep_env[:n_closed].long() * tcap +
                    ep_end[:n_closed].long()).to(torch.int32)
            last[:n_closed] = rows(b['lastobs'], cell, n_closed)
        if n_frag > n_closed:
            last[n_closed:] = rows(self.env.obs, ep_env[n_closed:].contiguous(),
                                   n_frag - n_closed)
        rew = torch.empty(S, dtype=torch.float32, device=dev)
        call('ga_gather_f32', dptr(b['rew']), dptr(src), S, dptr(rew), s)
        st = torch.empty(S, dtype=torch.uint8, device=dev)
        call('ga_gather_u8', dptr(b['st']), dptr(src), S, dptr(st), s)
        pol = self.agent
        gaussian = pol.kind == 'gaussian'
        env_infos, episode_infos = self._device_infos(
            b, src, ep_env, ep_end, self._packed_env_infos(b, src, tcap),
            self._packed_episode_infos(b, ep_env, ep_end))
        return DeviceEpisodeBatch(
            self.env.spec, lengths=length.astype(np.int64), obs_dev=obs,
            last_obs_dev=last, actions_dev=act, rewards_dev=rew,
            step_types_dev=st, ep_off_dev=off_dev, head_dev=head,
            head_name='mean' if gaussian else 'prob',
            log_std=pol.clamped_log_std() if gaussian else None,
            discrete=is_discrete(self.env.spec.action_space),
            env_infos=env_infos, episode_infos=episode_infos)


class GpuVecSampler:
    """``LocalSampler`` (``sampler/local_sampler.py:13-232``) for GPU workers.

    Same constructor keywords, ``from_worker_factory``, ``obtain_samples``,
    ``obtain_exact_episodes``, ``shutdown_worker``, ``total_env_steps`` and
    pickling behaviour; ``envs`` may be a :class:`~garage_amd.envs.VecEnv`.
    Returns :class:`~garage_amd._dtypes.DeviceEpisodeBatch`.
    """

    def __init__(self, agents, envs, *, worker_factory=None,
                 max_episode_length=None, is_tf_worker=False, seed=None,
                 n_workers=1, worker_class=GpuVecWorker, worker_args=None):
        if worker_factory is None and max_episode_length is None:
            raise TypeError('Must construct a sampler from WorkerFactory or'
                            'parameters (at least max_episode_length)')
        if isinstance(worker_factory, WorkerFactory):
            self._factory = worker_factory
        else:
            self._factory = WorkerFactory(
                max_episode_length=max_episode_length,
                is_tf_worker=is_tf_worker, seed=seed, n_workers=n_workers,
                worker_class=worker_class, worker_args=worker_args)
        self._agents = self._factory.prepare_worker_messages(agents)
        self._envs = self._factory.prepare_worker_messages(
            envs, preprocess=_copy_env)
        self._build_workers()
        self.total_env_steps = 0

    def _build_workers(self):
        self._workers = [
            self._factory(i) for i in range(self._factory.n_workers)
        ]
        for worker, agent, env in zip(self._workers, self._agents, self._envs):
            worker.update_agent(agent)
            worker.update_env(env)

    @classmethod
    def from_worker_factory(cls, worker_factory, agents, envs):
        return cls(agents, envs, worker_factory=worker_factory)

    def start_worker(self):
        """No-op, as in ``sampler/sampler.py``."""

    def _update_workers(self, agent_update, env_update):
        agent_updates = self._factory.prepare_worker_messages(agent_update)
        env_updates = self._factory.prepare_worker_messages(
            env_update, preprocess=_copy_env)
        for worker, a, e in zip(self._workers, agent_updates, env_updates):
            worker.update_agent(a)
            worker.update_env(e)

    def obtain_samples(self, itr, num_samples, agent_update, env_update=None):
        """``local_sampler.py:134-166``."""
        del itr
        self._update_workers(agent_update, env_update)
        if len(self._workers) == 1 and not isinstance(self._workers[0],
                                                      GpuFragmentWorker):
            samples = self._workers[0].rollout_samples(num_samples)
        else:
            batches, done = [], 0
            while done < num_samples:
                for worker in self._workers:
                    batch = worker.rollout()
                    done += len(batch.actions)
                    batches.append(batch.to_host())
                    if done >= num_samples:
                        break
            samples = EpisodeBatch.concatenate(*batches)
        self.total_env_steps += int(np.sum(samples.lengths))
        return samples

    def obtain_exact_episodes(self, n_eps_per_worker, agent_update,
                              env_update=None):
        """``local_sampler.py:168-200`` (worker order)."""
        self._update_workers(agent_update, env_update)
        batches = []
        for worker in self._workers:
            for _ in range(n_eps_per_worker):
                batches.append(worker.rollout().to_host())
        samples = EpisodeBatch.concatenate(*batches)
        self.total_env_steps += int(np.sum(samples.lengths))
        return samples

    def shutdown_worker(self):
        for worker in self._workers:
            worker.shutdown()

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_workers'] = None  # local_sampler.py:207-217
        # what a worker carries from one rollout to the next: the Philox step
        # counter of the action noise and which envs have an episode in flight
        # (only those are reset at the next rollout, vec_worker.py:122-126), so
        # that a resumed run (trainer.py:263-341) continues like the
        # uninterrupted one
        state['_worker_state'] = [
            dict(global_step=getattr(w, '_global_step', 0),
                 ep_t=None if getattr(w, '_ep_t', None) is None else
                 w._ep_t.cpu().numpy())
            for w in self._workers]
        return state

    def __setstate__(self, state):
        saved = state.pop('_worker_state', None)
        self.__dict__.update(state)
        self._build_workers()
        for w, st in zip(self._workers, saved or []):
            w._global_step = st['global_step']
            if st['ep_t'] is not None:
                w._ep_t = torch.from_numpy(st['ep_t']).to(w.device)
                w._needs_env_reset = False  # the env came back with its state


class GpuPopulationSampler:
    """Rolls out a POPULATION of policies in one launch per chunk of steps.

    ``env`` is one device :class:`~garage_amd.envs.VecEnv` of ``n_members * g``
    envs (optionally inside :class:`~garage_amd.envs.NormalizedVecEnv` for
    observation / reward statistics); member ``m`` owns the envs
    ``[m * g, (m + 1) * g)`` and steps them with its own parameter vector
    (``ga_policy_env_step_members_f32``).  ``agent`` is the template policy:
    network shape, head options and -- where the std is not learned -- the
    log-std every member uses.  There is no reference counterpart: its samplers
    give each worker its own ``agent_update`` and step them one after another.

    A host env, ``noise_fn``, an action-rescaling ``NormalizedVecEnv`` or a
    network the fused step does not take raise here; nothing falls back to the
    stepwise path.

    :meth:`obtain_samples` packs every member's episodes into a batch -- with
    ``joint_pack=True`` all members in one pass over the rollout buffers
    (:meth:`obtain_population`), otherwise one ``GpuVecWorker._pack`` per member;
    :meth:`obtain_statistics` returns per-episode statistics of the same
    episodes without packing anything.  ``statistics_only=True`` tells an
    algorithm that reads a score per member and nothing else to call the latter.
    """

    def __init__(self, agent, env, *, n_members, max_episode_length, seed=None,
                 worker_args=None, statistics_only=False, joint_pack=False):
        self._agent = agent
        # True: obtain_samples packs all members in one pass
        # (obtain_population); False: one GpuVecWorker._pack per member, the
        # path the joint one is tested against
        self._joint_pack = bool(joint_pack)
        # what an algorithm that only scores its members (CEM) reads to call
        # obtain_statistics instead of obtain_samples; nothing here depends on it
        self.statistics_only = bool(statistics_only)
        self._n_members = int(n_members)
        if self._n_members < 1:
            raise ValueError('n_members must be at least 1')
        self._max_episode_length = max_episode_length
        self._seed = seed
        self._worker_args = dict(worker_args or {})
        if self._worker_args.get('noise_fn') is not None:
            raise ValueError('GpuPopulationSampler: noise_fn (teacher-forced '
                             'noise) is per step and per policy; the '
                             'population rollout draws its noise on the device')
        if not self._worker_args.get('fused_policy_step', True):
            raise ValueError('GpuPopulationSampler: the population rollout IS '
                             'the fused policy step (fused_policy_step=False)')
        self._worker_args.pop('n_envs', None)
        self._check_env(env)
        lib, desc = _lib.load(), C.byref(agent.net._desc)
        if not lib.ga_policy_step_wide_supported(desc):
            raise ValueError('GpuPopulationSampler: the fused rollout step does '
                             'not take this network (layer inputs up to 512, '
                             'outputs up to 32)')
        self._env = env
        self._build_worker()
        self.total_env_steps = 0

    def _check_env(self, env):
        inner = env._env if type(env) is NormalizedVecEnv else env
        if not isinstance(inner, _DeviceVecEnv):
            raise TypeError('GpuPopulationSampler needs a device env batch '
                            '(a host env steps on the CPU, one policy at a '
                            'time); got {!r}'.format(type(inner).__name__))
        if type(env) is NormalizedVecEnv and env._act_low is not None:
            raise ValueError('GpuPopulationSampler: this NormalizedVecEnv '
                             'rescales actions, which is a launch of its own '
                             'between policy and env; declare the action space '
                             'unbounded or wrap the statistics only')
        if env.n_envs % self._n_members:
            raise ValueError('{} envs do not split into {} members'.format(
                env.n_envs, self._n_members))

    def _build_worker(self):
        self._worker = GpuVecWorker(
            seed=self._seed, max_episode_length=self._max_episode_length,
            worker_number=0, n_envs=self._env.n_envs, **self._worker_args)
        self._worker.update_agent(self._agent)
        self._worker.update_env(self._env)

    n_members = property(lambda self: self._n_members)

    def start_worker(self):
        """No-op, as in ``sampler/sampler.py``."""

    def _packed(self, member_params):
        """``pack_members``' tensor as it is, anything else through it."""
        net, M = self._agent.net, self._n_members
        if torch.is_tensor(member_params) and member_params.is_cuda:
            p = member_params
            if (p.dtype != torch.float32 or p.dim() != 2 or p.stride(1) != 1
                    or p.shape != (M, net.n_flat)):
                raise ValueError(
                    'member_params on the device must be pack_members\' '
                    '({}, {}) float32 tensor, got {}'.format(
                        M, net.n_flat, tuple(p.shape)))
            return p
        vectors = np.asarray(member_params)
        if vectors.ndim != 2 or vectors.shape[0] != M:
            raise ValueError('member_params needs one row per member ({}), got '
                             'shape {}'.format(M, vectors.shape))
        return self._agent.pack_members(vectors)

    def _steps(self, b, col, k, params):
        """``k`` rollout steps of every member into columns ``[col, col + k)``:
        one launch."""
        w = self._worker
        env = w.env
        inner, norm = env, None
        if type(env) is NormalizedVecEnv:  # statistics fused into the env step
            inner, norm = env._env, env.norm_args()
            if norm.normalize_obs:
                norm.raw_obs = inner.obs.data_ptr()
                norm.raw_next_obs = inner.next_obs.data_ptr()
        env_ref, _keepalive = inner.native_env_ref(b['dev_infos'])
        a = w._head_args(b, col, True)
        r = w._record_args(b, col)
        call('ga_policy_env_step_members_f32', C.byref(self._agent.net._desc),
             dptr(params), C.byref(a), C.byref(env_ref), C.byref(r),
             None if norm is None else C.byref(norm), k, self._n_members,
             params.stride(0), stream_ptr())
        if k % 2:
            env.advance()
        w._global_step += k

    def _rollout(self, num_samples, member_params, env_update, progress):
        """The stepping both ``obtain_*`` methods share: one first launch of
        ``ceil(num_samples / g)`` columns -- no member can be done before --
        then as many steps at a time as the member that is furthest behind
        needs at the very least.  ``progress(b, col)``, after every launch:
        ``(samples each member has completed, whatever the caller keeps of the
        check)``.  Returns ``(b, params, what the last check kept)``."""
        w = self._worker
        if env_update is not None:
            w.update_env(env_update)
            self._check_env(w.env)
            self._env = w.env
        w._needs_agent_reset = True  # every call brings new parameters
        params = self._packed(member_params)
        w._start()
        g = w._n_envs // self._n_members
        b = w._alloc_buffers(num_samples, n_share=g)
        tcap = b['Tcap']
        col, k = 0, min(-(-num_samples // g), tcap)
        while True:
            self._steps(b, col, k, params)
            col += k
            done, kept = progress(b, col)
            if (done >= num_samples).all():
                return b, params, kept
            if col >= tcap:
                raise RuntimeError('rollout buffer exhausted: an environment '
                                   'ran past max_episode_length')
            short = int(num_samples - done.min())
            k = min(-(-short // g), tcap - col)

    def obtain_samples(self, itr, num_samples, member_params, env_update=None):
        """One :class:`~garage_amd._dtypes.DeviceEpisodeBatch` per member: the
        episodes a lone ``GpuVecWorker`` of the member's ``g`` envs with the
        member's parameters returns from ``rollout_samples(num_samples)`` --
        those completed before the first column ``c_m`` at which the member's
        completed episodes hold ``>= num_samples`` steps.  ``member_params``:
        what ``policy.pack_members`` returns, or an ``(M, P)`` array of compact
        vectors."""
        if self._joint_pack:
            return self.obtain_population(itr, num_samples, member_params,
                                          env_update).members
        del itr
        w, M = self._worker, self._n_members
        num_samples = max(int(num_samples), 1)

        def progress(b, col):
            # per member and column: samples and episodes completed there
            ended = b['tail'][:, :col].to(torch.int32).reshape(M, -1, col)
            host = torch.stack([torch.cumsum(ended.sum(1), 1),
                                (ended != 0).sum(1)]).cpu()
            done, eps = host[0].numpy(), host[1].to(torch.int32)  # (M, col)
            return done[:, -1], (done, eps)

        b, params, (done, eps) = self._rollout(num_samples, member_params,
                                               env_update, progress)
        # c_m: the columns a member keeps stepping past it are dropped here
        c = (done >= num_samples).argmax(1) + 1
        pol = self._agent
        log_std = [None] * M
        if pol.kind == 'gaussian':
            raw = params[:, 0].cpu().numpy()
            log_std = [pol.log_std_of(float(v))[0] for v in raw]
        g = w._n_envs // M
        batches = [w._pack(b, int(c[m]), member=(m * g, (m + 1) * g, eps[m],
                                                 log_std[m]))
                   for m in range(M)]
        self.total_env_steps += int(
            sum(int(np.sum(x.lengths)) for x in batches))
        return batches

    def _progress_check(self, num_samples):
        """The check after every launch that :meth:`obtain_statistics` and
        :meth:`obtain_population` share: one ``ga_member_progress`` launch and
        a copy of three integers per member.  Returns ``(progress, work)``;
        ``work`` holds ``prog`` and, once called, ``col_base`` on the device."""
        w, M = self._worker, self._n_members
        s = stream_ptr()
        work = {'prog': torch.empty(M, 3, dtype=torch.int32, device=w.device)}

        def progress(b, col):
            if 'col_base' not in work:  # sized by the rollout buffers
                work['col_base'] = torch.empty(M, b['Tcap'], dtype=torch.int32,
                                               device=w.device)
            call('ga_member_progress', dptr(b['tail']), w._n_envs, b['Tcap'],
                 col, M, num_samples, dptr(work['prog']),
                 dptr(work['col_base']), s)
            host = work['prog'].cpu().numpy()
            return host[:, 2], (col, host)

        return progress, work

    def obtain_population(self, itr, num_samples, member_params,
                          env_update=None):
        """A :class:`~garage_amd._dtypes.DevicePopulationBatch`: every member's
        batch of :meth:`obtain_samples` as a view of ONE set of packed arrays.
        After the last progress check (``obtain_statistics``' own) the whole
        pack is ``ga_member_pack_index``, ``ga_member_pack_gather`` and one
        copy to the host -- the lengths, the members' sample counts and rows,
        their log-stds and the recorded env_infos -- whatever the number of
        members.  The arrays are sized before the index runs from what the
        check already told the host: ``S_m <= g * c_m``."""
        del itr
        num_samples = max(int(num_samples), 1)
        progress, work = self._progress_check(num_samples)
        b, params, (col, host) = self._rollout(num_samples, member_params,
                                               env_update, progress)
        pop = self._pack_population(b, params, col, host, work)
        self.total_env_steps += int(pop.member_samples.sum())
        return pop

    def _pack_population(self, b, params, n_cols, host, work):
        """The joint pack of the columns ``[0, n_cols)``; ``host``: the last
        check's ``(M, 3)`` progress, ``work`` its device side."""
        w, M, pol = self._worker, self._n_members, self._agent
        env, dev, tcap, n = w.env, w.device, b['Tcap'], w._n_envs
        g, s = n // M, stream_ptr()
        counts = host[:, 1].astype(np.int64)  # every member reached its c_m
        episode_start = np.concatenate([[0], np.cumsum(counts)])
        N = int(episode_start[-1])
        # rows of the packed arrays: a member's slice starts on a multiple of
        # 16 rows and holds at most g * c_m samples
        R = int((-(-(g * host[:, 0].astype(np.int64)) // 16) * 16).sum())
        gaussian = pol.kind == 'gaussian'
        specs, keys = env.env_info_specs, list(b['dev_infos'])
        i32, i64, u8, f32 = (torch.int32, torch.int64, torch.uint8,
                             torch.float32)
        # everything the host reads lies in one buffer: one copy
        fields = [('member_samples', i64, M), ('member_off', i64, M + 1),
                  ('ep_len', i32, N)]
        if gaussian:
            fields.append(('raw_std', f32, M))
        fields += [('info/' + k, u8, R) for k in keys]
        fields += [('end/' + k, u8, N) for k in keys]
        at, total = {}, 0
        for name, dtype, count in fields:
            total = -(-total // 16) * 16
            at[name] = (total, dtype, count * dtype.itemsize)
            total += count * dtype.itemsize
        blob = torch.empty(total, dtype=u8, device=dev)
        out = {name: blob[lo:lo + size].view(dtype)
               for name, (lo, dtype, size) in at.items()}
        ep_env = torch.empty(N, dtype=i32, device=dev)
        ep_end = torch.empty_like(ep_env)
        ep_off = torch.empty(N + M, dtype=i64, device=dev)
        src = torch.empty(R, dtype=i32, device=dev)
        call('ga_member_pack_index', dptr(b['tail']), n, tcap, n_cols, M,
             dptr(work['prog']), dptr(work['col_base']), N, R, dptr(ep_env),
             dptr(ep_end), dptr(out['ep_len']), dptr(ep_off),
             dptr(out['member_samples']), dptr(out['member_off']), dptr(src),
             s)
        planes = []

        def plane(buf, dst, per_episode=False):
            width = buf.shape[2] if buf.dim() == 3 else 1
            planes.append(_lib.PackPlane(
                src=buf.data_ptr(), dst=dst.data_ptr(), ld_src=width,
                ld_dst=width, elem_size=buf.element_size(), width=width,
                per_episode=int(per_episode)))
            return dst

        def rows(buf, count):
            return plane(buf, torch.empty((count, ) + tuple(buf.shape[2:]),
                                          dtype=buf.dtype, device=dev))

        obs, act = rows(b['obs'], R), rows(b['act'], R)
        head = rows(b['head'], R) if b['head'] is not None else None
        rew, st = rows(b['rew'], R), rows(b['st'], R)
        last = plane(b['lastobs'], torch.empty(N, b['lastobs'].shape[2],
                                               dtype=f32, device=dev), True)
        for k in keys:
            plane(b['dev_infos'][k], out['info/' + k])
            plane(b['dev_infos'][k], out['end/' + k], True)
        for lo in range(0, len(planes), _lib.PACK_MAX_PLANES):
            part = planes[lo:lo + _lib.PACK_MAX_PLANES]
            call('ga_member_pack_gather', (_lib.PackPlane * len(part))(*part),
                 len(part), dptr(src), R, dptr(ep_env), dptr(ep_end), N, tcap,
                 s)
        if gaussian:
            out['raw_std'].copy_(params[:, 0])
        raw = blob.cpu().numpy()
        np_of = {i32: np.int32, i64: np.int64, u8: np.uint8, f32: np.float32}
        got = {name: raw[lo:lo + size].view(np_of[dtype])
               for name, (lo, dtype, size) in at.items()}
        member_off, member_samples = got['member_off'], got['member_samples']
        lengths = got['ep_len'].astype(np.int64)
        used = int(member_off[M])  # the rows behind it belong to no member
        obs, act, rew, st = obs[:used], act[:used], rew[:used], st[:used]
        head = None if head is None else head[:used]
        episode_infos = env.episode_infos_of(
            ep_env, lambda key: got['end/' + key].astype(specs[key]))
        members = []
        for m in range(M):
            lo = int(member_off[m])
            hi = lo + int(member_samples[m])
            e0, e1 = int(episode_start[m]), int(episode_start[m + 1])
            env_infos = {k: got['info/' + k][lo:hi].astype(specs[k])
                         for k in keys}
            if keys:
                env.finish_env_infos(env_infos)
            members.append(DeviceEpisodeBatch(
                env.spec, lengths=lengths[e0:e1], obs_dev=obs[lo:hi],
                last_obs_dev=last[e0:e1], actions_dev=act[lo:hi],
                rewards_dev=rew[lo:hi], step_types_dev=st[lo:hi],
                ep_off_dev=ep_off[e0 + m:e1 + m + 1],
                head_dev=None if head is None else head[lo:hi],
                head_name='mean' if gaussian else 'prob',
                log_std=(pol.log_std_of(float(got['raw_std'][m]))[0]
                         if gaussian else None),
                discrete=is_discrete(env.spec.action_space),
                env_infos=env_infos,
                episode_infos={k: v[e0:e1] for k, v in episode_infos.items()}))
        return DevicePopulationBatch(
            members, obs_dev=obs, actions_dev=act, head_dev=head,
            rewards_dev=rew, step_types_dev=st, last_obs_dev=last,
            ep_off_dev=ep_off, env_info_planes={k: out['info/' + k][:used] for k in keys},
            member_off=member_off.copy(), member_samples=member_samples.copy(),
            episode_start=episode_start)

    def obtain_statistics(self, itr, num_samples, member_params, discount,
                          env_update=None):
        """One :class:`~garage_amd._dtypes.EpisodeStatistics` per member, of
        exactly the episodes :meth:`obtain_samples` returns -- same stepping,
        same columns ``c_m``, same order -- reduced on the device from the raw
        rollout buffers (``ga_member_progress``,
        ``ga_member_episode_statistics``): nothing is packed or gathered, a
        progress check copies three integers per member to the host and the
        ending one array of all members' episodes.  ``discount``: of the
        discounted returns, in fp64 as ``log_performance_host`` applies it."""
        del itr
        w, M = self._worker, self._n_members
        num_samples = max(int(num_samples), 1)
        discount = float(discount)
        s = stream_ptr()
        progress, work = self._progress_check(num_samples)
        prog = work['prog']
        b, _, (col, host) = self._rollout(num_samples, member_params,
                                          env_update, progress)
        counts = host[:, 1].astype(np.int64)  # every member reached its c_m
        N = int(counts.sum())
        # one buffer, one copy: f64[N] f64[N] i32[N] u8[N] u8[N]
        out = torch.empty(22 * N, dtype=torch.uint8, device=w.device)
        und = out[:8 * N].view(torch.float64)
        disc = out[8 * N:16 * N].view(torch.float64)
        length = out[16 * N:20 * N].view(torch.int32)
        term, succ = out[20 * N:21 * N], out[21 * N:]
        plane = b['dev_infos'].get('success')
        call('ga_member_episode_statistics', dptr(b['rew']), dptr(b['st']),
             dptr(b['tail']), dptr(plane), w._n_envs, b['Tcap'], col, M,
             num_samples, discount, dptr(prog), dptr(work['col_base']), N,
             dptr(length), dptr(und), dptr(disc), dptr(term), dptr(succ), s)
        raw = out.cpu().numpy()
        und = raw[:8 * N].view(np.float64)
        disc = raw[8 * N:16 * N].view(np.float64)
        length = raw[16 * N:20 * N].view(np.int32).astype(np.int64)
        term = raw[20 * N:21 * N].astype(np.float64)
        succ = None if plane is None else raw[21 * N:].astype(np.float64)
        stats, lo = [], 0
        for m in range(M):
            hi = lo + int(counts[m])
            stats.append(EpisodeStatistics(
                length[lo:hi], und[lo:hi], disc[lo:hi], term[lo:hi],
                None if succ is None else succ[lo:hi], discount))
            lo = hi
        self.total_env_steps += int(length.sum())
        return stats

    def shutdown_worker(self):
        self._worker.shutdown()

    def __getstate__(self):
        state = self.__dict__.copy()
        w = state.pop('_worker')
        # (as GpuVecSampler: the Philox step counter and the episodes in flight)
        state['_worker_state'] = dict(
            global_step=w._global_step,
            ep_t=None if w._ep_t is None else w._ep_t.cpu().numpy())
        return state

    def __setstate__(self, state):
        saved = state.pop('_worker_state')
        self.__dict__.update(state)
        self._build_worker()
        self._worker._global_step = saved['global_step']
        if saved['ep_t'] is not None:
            self._worker._ep_t = torch.from_numpy(saved['ep_t']).to(
                self._worker.device)
            self._worker._needs_env_reset = False


__all__ = ['WorkerFactory', 'GpuVecWorker', 'GpuFragmentWorker',
           'GpuVecSampler', 'GpuPopulationSampler']
