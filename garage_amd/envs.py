"""Batched environments behind the GPU sampler.

garage steps one ``Environment`` object per env in a Python loop
(``sampler/vec_worker.py:185-197``; contract ``_environment.py:237-276``).  Here
an environment *batch* is one object that advances all ``n_envs`` members with
a single call and keeps its state in HBM:

    reset_all()            -> ``obs`` (n, ldo) holds every first observation
    step_all(actions)      -> ``reward`` (n,), ``step_type`` (n,) uint8 and
                              ``next_obs`` (n, ldo) (the true next observation,
                              terminal ones included)
    reset_where(done)      -> members with ``done != 0`` start a new episode;
                              their first observation overwrites ``next_obs``

``SyntheticVecEnv`` is the benchmark workload of BASELINE.json (HIP kernels,
Philox-keyed).  ``PointVecEnv`` and ``GridWorldVecEnv`` are the reference's own
``PointEnv`` and ``GridWorldEnv`` as device batches (HIP kernels, numpy's fp32
arithmetic), stepped inside the sampler's one-launch rollout like the synthetic
env; ``MultiTaskPointVecEnv`` is ``MultiEnvWrapper`` over ``PointEnv`` tasks, the
task switch at every reset included.  ``CartPoleVecEnv`` is gym's CartPole-v1 in a
fixed fp32 arithmetic (``CartPoleEnv`` is its per-env numpy twin), and
``PendulumVecEnv`` gym's Pendulum-v0 the same way (twin: ``PendulumEnv``), and
``DoublePendulumVecEnv`` the inverted double pendulum on a cart, the task of
InvertedDoublePendulum-v2 (twin: ``DoublePendulumEnv``).  ``AcrobotVecEnv`` is
gym's Acrobot-v1 (twin: ``AcrobotEnv``) and ``MountainCarVecEnv`` its
MountainCar-v0 and MountainCarContinuous-v0 (twin: ``MountainCarEnv``), which
completes gym's classic control on the device.
``HostVecEnv`` adapts a list of ordinary per-env objects (any
``garage.Environment``-like with ``reset``/``step``) so existing CPU simulators
still feed the device-resident update path.
"""
import collections
import ctypes as C

import numpy as np
import torch

from garage_amd import _lib
from garage_amd._dtypes import Box, Discrete, EnvSpec, StepType, is_discrete
from garage_amd._lib import call, dptr, stream_ptr
from garage_amd.engine import require_gpu, round4


class VecEnv:
    """Base class / protocol of a device-batched environment."""

    n_envs = 0
    spec = None

    @property
    def obs_dim(self):
        return self.spec.observation_space.flat_dim

    @property
    def act_width(self):
        """Columns of the action matrix handed to :meth:`step_all`."""
        if is_discrete(self.spec.action_space):
            return 1
        return self.spec.action_space.flat_dim

    def _alloc(self, device):
        n, ldo = self.n_envs, round4(self.obs_dim)
        self.device = device
        self.obs = torch.zeros(n, ldo, dtype=torch.float32, device=device)
        self.next_obs = torch.zeros(n, ldo, dtype=torch.float32, device=device)
        self.reward = torch.zeros(n, dtype=torch.float32, device=device)
        self.step_type = torch.zeros(n, dtype=torch.uint8, device=device)

    def advance(self):
        """Make ``next_obs`` the current observation (buffer swap)."""
        self.obs, self.next_obs = self.next_obs, self.obs

    def hold(self):
        """Carry the current observations over as the next ones (before a
        partial ``reset_where``: rows that are not reset keep their state)."""
        self.next_obs.copy_(self.obs)

    def reset_all(self):
        raise NotImplementedError

    def step_all(self, actions):
        raise NotImplementedError

    def reset_where(self, done):
        raise NotImplementedError

    def close(self):
        pass

    # -- device env_infos / episode_infos ------------------------------------
    # A device batch declares the per-step ``env_info`` keys it writes on the GPU
    # (key -> numpy dtype; bool is the one kind the kernels write, as uint8) and
    # reports per-episode ``episode_info`` values as (n, ...) device tensors.  The
    # worker records the former per rollout column and gathers both into the
    # packed batch with the same indices as the observations.
    env_info_specs = {}

    def step_env_infos(self):
        """``{key: (n,) device tensor}`` of the last :meth:`step_all`."""
        return {}

    def device_episode_infos(self):
        """``{key: (n, ...) device tensor}``: what ``reset()`` reported for each
        member's episode."""
        return {}

    def finish_env_infos(self, env_infos):
        """Adds, in place, the ``env_info`` keys that are made on the host from
        the gathered ``(S,)`` arrays of the recorded ones (a batch that reports
        such a key says so here; nothing by default)."""

    def episode_infos_of(self, ep_env, info_at_end):
        """``{key: (N, ...) array}``: the ``episode_info`` of each packed
        episode, given its member index (``ep_env``, an ``(N,)`` device tensor);
        ``info_at_end(key)`` gathers the recorded env_info ``key`` of each
        episode's last step as an ``(N,)`` array.  By default the member's row
        of :meth:`device_episode_infos`."""
        return {k: v[ep_env.long()].cpu().numpy()
                for k, v in self.device_episode_infos().items()}

    def native_env_ref(self, info_bufs):
        """``(ga_env_ref, keepalive)`` for ``ga_rollout_env_steps`` with the
        per-step env_infos written into ``info_bufs`` (``{key: (n, Tcap)}``), or
        None when the batch has no device step."""
        return None


class _DeviceVecEnv(VecEnv):
    """A batch stepped by the HIP kernels: the batch protocol over ``ga_env_*``
    and the ``ga_env_ref`` of the subclass's C struct (``_set_struct``), and
    pickling -- plain attributes as they are, the listed state tensors through
    the host (trainer.py:263-293 pickles algo + env)."""

    _KIND = None
    _STATE = ()

    def _set_struct(self, c):
        self._c = c
        self._ref = _lib.env_ref(self._KIND, c)

    def reset_all(self):
        call('ga_env_reset', C.byref(self._ref), None, dptr(self.obs),
             self.obs.stride(0), stream_ptr())

    def step_all(self, actions):
        call('ga_env_step', C.byref(self._ref), dptr(actions),
             actions.stride(0), dptr(self.obs), dptr(self.next_obs),
             self.obs.stride(0), dptr(self.reward), dptr(self.step_type),
             stream_ptr())

    def reset_where(self, done):
        call('ga_env_reset', C.byref(self._ref), dptr(done),
             dptr(self.next_obs), self.next_obs.stride(0), stream_ptr())

    def native_env_ref(self, info_bufs):
        return self._ref, self._c

    def __getstate__(self):
        state = {
            k: v for k, v in self.__dict__.items()
            if not torch.is_tensor(v) and k not in ('_c', '_ref', 'device')
        }
        state['_saved'] = {k: getattr(self, k).cpu().numpy()
                           for k in self._STATE + ('obs', )}
        return state

    def __setstate__(self, state):
        saved = state.pop('_saved')
        self.__dict__.update(state)
        self._init_device(None)
        for k, v in saved.items():
            getattr(self, k).copy_(torch.from_numpy(v))


class SyntheticVecEnv(_DeviceVecEnv):
    """``n_envs`` synthetic environments stepped by one HIP kernel.

    Observation ``t`` of episode ``e`` of env ``i``: ``obs_dim`` unit-variance
    uniforms from Philox4x32-10 keyed ``(seed; env_id0 + i, e, t)``; reward: a
    Philox value plus ``0.1 * <clip(a), obs>`` (continuous) or ``0.1 * obs[a]``
    (discrete); episode length ``L ~ U{min_len..max_episode_length}``, ending
    TIMEOUT when ``L == max_episode_length`` else TERMINAL.  ``oracle/envs.py``
    holds the bit-identical per-env CPU twin used by the parity tests.
    """

    _KIND = _lib.ENV_SYNTH
    _STATE = ('_episode', '_t', '_len')

    def __init__(self, n_envs, obs_dim, act_dim, max_episode_length, *,
                 min_len=None, seed=0, discrete=False, env_id0=0, device=None,
                 action_bounds=None):
        self.n_envs = int(n_envs)
        self._obs_dim = int(obs_dim)
        self._act_dim = int(act_dim)
        self.discrete = bool(discrete)
        self.max_episode_length = int(max_episode_length)
        self.min_len = (self.max_episode_length
                        if min_len is None else int(min_len))
        self.seed = int(seed)
        self.env_id0 = int(env_id0)
        # action_bounds = (low, high): the declared Box of a continuous action
        # space (what ``normalize`` rescales to); the dynamics do not change
        lo, hi = (-np.inf, np.inf) if action_bounds is None else action_bounds
        act_space = (Discrete(act_dim) if discrete else Box(
            lo, hi, (act_dim, )) if np.isscalar(lo) else Box(lo, hi))
        self.spec = EnvSpec(Box(-np.inf, np.inf, (obs_dim, )), act_space,
                            max_episode_length=self.max_episode_length)
        self._init_device(device)

    def _init_device(self, device):
        device = device or require_gpu()
        self._alloc(device)
        n = self.n_envs
        self._episode = torch.full((n, ), -1, dtype=torch.int32, device=device)
        self._t = torch.zeros(n, dtype=torch.int32, device=device)
        self._len = torch.zeros(n, dtype=torch.int32, device=device)
        e = _lib.SynthEnv()
        e.n, e.env_id0 = n, self.env_id0
        e.obs_dim, e.act_dim = self._obs_dim, self._act_dim
        e.discrete = int(self.discrete)
        e.min_len, e.max_len = self.min_len, self.max_episode_length
        e.seed = self.seed
        e.episode = self._episode.data_ptr()
        e.t = self._t.data_ptr()
        e.len = self._len.data_ptr()
        self._set_struct(e)


def _check_finite_length(max_episode_length):
    if max_episode_length is None or not np.isfinite(max_episode_length):
        raise ValueError('a device env batch needs a finite max_episode_length')
    max_episode_length = int(max_episode_length)
    if not 1 <= max_episode_length <= 65535:
        raise ValueError('max_episode_length must be in 1..65535')
    return max_episode_length


class PointVecEnv(_DeviceVecEnv):
    """``n_envs`` copies of ``garage.envs.PointEnv`` (``envs/point_env.py``)
    stepped by one HIP kernel, one thread per env, in numpy's fp32 arithmetic:
    observations, rewards, step types and ``env_info['success']`` equal the
    reference's bit for bit.

    Each member has its own goal (``goals``, an ``(n, 2)`` float32 device
    tensor); ``set_task`` sets every member's, ``set_tasks`` one per member.
    The per-step ``env_info['success']`` is recorded on the device and each
    episode reports ``episode_infos['goal']``.

    Deviations from the reference:

    - the per-step ``env_info['task']`` dict is not reported (the goal is in
      ``episode_infos``);
    - ``episode_infos['goal']`` is the goal in force when the batch is packed,
      which differs only if ``set_task`` is called mid-rollout (the sampler
      never does; :class:`MultiTaskPointVecEnv`, whose goals change at every
      reset, reports each episode's own);
    - goals are held in float32, as the reference's constructor holds them
      (its ``set_task`` keeps a float64 goal as float64);
    - the goal check of the constructor raises ``ValueError`` instead of an
      assertion, and ``max_episode_length`` must be finite.
    """

    env_info_specs = {'success': np.bool_}
    _KIND = _lib.ENV_POINT
    _STATE = ('_point', 'goals', '_t')

    def __init__(self, n_envs, goal=(1., 1.), arena_size=5., done_bonus=0.,
                 never_done=False, max_episode_length=None, device=None):
        self.n_envs = int(n_envs)
        self._arena_size = float(arena_size)
        self._done_bonus = float(done_bonus)
        self._never_done = bool(never_done)
        self.max_episode_length = _check_finite_length(max_episode_length)
        self._goal0 = self._check_goal(goal)
        self.spec = EnvSpec(Box(-np.inf, np.inf, (3, )), Box(-0.1, 0.1, (2, )),
                            max_episode_length=self.max_episode_length)
        self._init_device(device)
        self.goals.copy_(torch.from_numpy(np.tile(self._goal0, (self.n_envs, 1))))

    def _check_goal(self, goal):
        goal = np.array(goal, dtype=np.float32).reshape(2)
        if not ((goal >= -self._arena_size) &
                (goal <= self._arena_size)).all():
            raise ValueError('goal {} lies outside the arena [-{}, {}]'.format(
                goal, self._arena_size, self._arena_size))
        return goal

    def _init_device(self, device):
        device = device or require_gpu()
        self._alloc(device)
        n = self.n_envs
        self._point = torch.zeros(n, 2, dtype=torch.float32, device=device)
        self.goals = torch.zeros(n, 2, dtype=torch.float32, device=device)
        self._t = torch.zeros(n, dtype=torch.int32, device=device)
        self._success = torch.zeros(n, dtype=torch.uint8, device=device)
        self._set_struct(self._struct(self._success))

    def _struct(self, success):
        e = _lib.PointEnv()
        e.n = self.n_envs
        e.arena_size, e.done_bonus = self._arena_size, self._done_bonus
        e.never_done = int(self._never_done)
        e.max_episode_length = self.max_episode_length
        e.point, e.goal = self._point.data_ptr(), self.goals.data_ptr()
        e.t = self._t.data_ptr()
        e.success = success.data_ptr()
        return e

    # -- tasks (point_env.py:172-212) -------------------------------------------
    @staticmethod
    def sample_tasks(num_tasks):
        """``PointEnv.sample_tasks``: the same draw from numpy's global RNG."""
        goals = np.random.uniform(-2, 2, size=(num_tasks, 2))
        return [{'goal': goal} for goal in goals]

    def set_task(self, task):
        """Every member's goal <- ``task['goal']``."""
        self.set_tasks([task] * self.n_envs)

    def set_tasks(self, tasks):
        """Member ``i``'s goal <- ``tasks[i]['goal']``."""
        if len(tasks) != self.n_envs:
            raise ValueError('set_tasks needs one task per env ({}), got '
                             '{}'.format(self.n_envs, len(tasks)))
        goals = np.stack([np.asarray(t['goal'], dtype=np.float32).reshape(2)
                          for t in tasks])
        self.goals.copy_(torch.from_numpy(goals))

    def step_env_infos(self):
        return {'success': self._success}

    def device_episode_infos(self):
        return {'goal': self.goals}

    def native_env_ref(self, info_bufs):
        e = self._struct(info_bufs['success'])
        return _lib.env_ref(self._KIND, e), e


def round_robin_strategy(num_tasks, last_task=None):
    """``garage.envs.multi_env_wrapper.round_robin_strategy``: task 0 first,
    then ``(last_task + 1) % num_tasks``.  :class:`MultiTaskPointVecEnv`
    recognises the function and runs the rule on the device."""
    if last_task is None:
        return 0
    return (last_task + 1) % num_tasks


def uniform_random_strategy(num_tasks, _):
    """``garage.envs.multi_env_wrapper.uniform_random_strategy``.  Called on
    the host it draws from Python's ``random`` like the reference;
    :class:`MultiTaskPointVecEnv` recognises the function and draws on the
    device from its own Philox stream instead (see there)."""
    import random
    return random.randint(0, num_tasks - 1)


_STRATEGIES = {round_robin_strategy: _lib.TASK_ROUND_ROBIN,
               uniform_random_strategy: _lib.TASK_UNIFORM_RANDOM}
MAX_TASKS = 256  # env_info['task_id'] is recorded as uint8 on the device


def task_draw(seed, env_id, counter, num_tasks):
    """The task :class:`MultiTaskPointVecEnv`'s uniform random strategy gives
    member ``env_id`` at its reset number ``counter`` (host only, no GPU)."""
    task = _lib.load().ga_multi_env_task_draw(int(seed), int(env_id),
                                              int(counter), int(num_tasks))
    if task < 0:
        raise ValueError('num_tasks must be in 1..{}'.format(MAX_TASKS))
    return task


class MultiTaskPointVecEnv(_DeviceVecEnv):
    """``n_envs`` copies of ``MultiEnvWrapper([PointEnv(goal=g, ...) for g in
    goals], sample_strategy, mode, env_names)`` (``envs/multi_env_wrapper.py``)
    stepped by one HIP kernel inside the one-launch rollout.

    Every member keeps its own active task, as the reference ``VecWorker``'s
    deep-copied wrappers do: each reset -- ``reset_all``, ``reset_where`` and
    the reset of a finished member inside the rollout kernels -- picks the
    member's next task, and the member's PointEnv gets that task's goal.  With
    ``mode='add-onehot'`` the observation is the PointEnv's ``(x, y, dist)``
    followed by the one-hot of the active task (``spec.observation_space`` is
    the ``(3 + K,)`` Box); ``mode='vanilla'`` leaves it as it is.  Every step
    reports ``env_info['task_id']`` (int64) and, with ``env_names``,
    ``env_info['task_name']`` next to ``success``; each episode reports
    ``episode_infos['goal']``, the goal of the task *that episode* ran.
    Round robin equals the reference bit for bit.

    ``start='same'`` is one wrapper deep-copied ``n_envs`` times (every member
    begins with task 0); ``start='spread'`` lets member ``i`` begin with task
    ``i % K`` (the reference given ``n_envs`` wrappers whose
    ``_active_task_index`` is preset), so that a batch covers all tasks from
    its first step.  It has no effect on ``uniform_random_strategy``.

    Limits and deviations from the reference:

    - ``uniform_random_strategy`` does not consume Python's global ``random``:
      reset number ``c`` of member ``i`` takes the first word ``u`` of
      Philox4x32-10 keyed ``(seed; i, c)`` on its own stream and runs task
      ``(u * K) >> 32`` (:func:`task_draw` gives the same number on the host);
    - the tasks share ``arena_size``, ``done_bonus``, ``never_done`` and
      ``max_episode_length``; only the goal differs;
    - ``task_id`` is held as uint8 on the device: at most 256 tasks.  The
      one-launch rollout with resident weights needs ``3 + K <= 32``; rows
      up to 512 wide (every ``K`` a uint8 can name) stay in the one-launch
      rollout with the weights streamed, like any other observation;
    - a sample strategy other than the two above raises
      ``NotImplementedError`` (an arbitrary Python callable cannot run in the
      kernel); ``mode='del-onehot'`` raises ``ValueError``: a PointEnv
      observation has no one-hot to delete;
    - no per-step ``env_info['task']`` dict, as for :class:`PointVecEnv`;
      ``active_task_index`` is an ``(n_envs,)`` array (-1 before the first
      reset, where the reference has ``None``).
    """

    _KIND = _lib.ENV_MULTI_POINT
    _STATE = ('_point', '_goal', '_t', '_last_task', '_resets')

    def __init__(self, n_envs, goals, sample_strategy=uniform_random_strategy,
                 mode='add-onehot', env_names=None, start='same', seed=0,
                 arena_size=5., done_bonus=0., never_done=False,
                 max_episode_length=None, device=None):
        self.n_envs = int(n_envs)
        self._arena_size = float(arena_size)
        self._done_bonus = float(done_bonus)
        self._never_done = bool(never_done)
        self.max_episode_length = _check_finite_length(max_episode_length)
        goals = np.asarray(goals, dtype=np.float32)
        if goals.ndim != 2 or goals.shape[1] != 2 or not len(goals):
            raise ValueError('goals must be a non-empty (K, 2) array, one '
                             'goal per task')
        if len(goals) > MAX_TASKS:
            raise ValueError('at most {} tasks (task_id is a uint8 on the '
                             'device), got {}'.format(MAX_TASKS, len(goals)))
        self._goals_np = np.stack(
            [PointVecEnv._check_goal(self, g) for g in goals])
        known = [v for f, v in _STRATEGIES.items() if f is sample_strategy]
        if not known:
            raise NotImplementedError(
                'sample_strategy {!r} cannot run on the device: use '
                'garage_amd.envs.round_robin_strategy or '
                'uniform_random_strategy'.format(sample_strategy))
        self._strategy = known[0]
        if mode == 'del-onehot':
            raise ValueError("mode 'del-onehot' has nothing to delete from a "
                             'PointEnv observation')
        if mode not in ('vanilla', 'add-onehot'):
            raise ValueError("mode must be 'vanilla' or 'add-onehot', got "
                             '{!r}'.format(mode))
        self._mode = mode
        if env_names is not None:
            if not isinstance(env_names, list):
                raise ValueError('env_names must be a list')
            if len(set(env_names)) != len(goals):
                raise ValueError('env_names are not unique or there is not an '
                                 'env_name corresponding to each task')
        self._env_names = env_names
        if start not in ('same', 'spread'):
            raise ValueError("start must be 'same' or 'spread', got "
                             '{!r}'.format(start))
        self._start = start
        self.seed = int(seed)
        K = self.num_tasks
        low = np.concatenate([np.full(3, -np.inf), np.zeros(K)])
        high = np.concatenate([np.full(3, np.inf), np.ones(K)])
        obs_space = (Box(low, high) if mode == 'add-onehot' else
                     Box(-np.inf, np.inf, (3, )))
        self.spec = EnvSpec(obs_space, Box(-0.1, 0.1, (2, )),
                            max_episode_length=self.max_episode_length)
        self.env_info_specs = {'success': np.bool_, 'task_id': np.int64}
        self._init_device(device)
        if start == 'spread':  # the task before member i's first one
            self._last_task.copy_(torch.arange(self.n_envs) % K - 1)

    num_tasks = property(lambda self: len(self._goals_np))

    @property
    def task_space(self):
        return Box(np.zeros(self.num_tasks), np.ones(self.num_tasks))

    @property
    def active_task_index(self):
        return self._last_task.cpu().numpy().astype(np.int64)

    def _init_device(self, device):
        device = device or require_gpu()
        self._alloc(device)
        n = self.n_envs
        self._point = torch.zeros(n, 2, dtype=torch.float32, device=device)
        self._goal = torch.zeros(n, 2, dtype=torch.float32, device=device)
        self._t = torch.zeros(n, dtype=torch.int32, device=device)
        self._task_goals = torch.from_numpy(self._goals_np).to(device)
        self._last_task = torch.full((n, ), -1, dtype=torch.int32,
                                     device=device)
        self._resets = torch.zeros(n, dtype=torch.int32, device=device)
        self._success = torch.zeros(n, dtype=torch.uint8, device=device)
        self._task_id = torch.zeros(n, dtype=torch.uint8, device=device)
        self._set_struct(self._struct(self._success, self._task_id))

    def _struct(self, success, task_id):
        e = _lib.MultiPointEnv()
        e.n = self.n_envs
        e.arena_size, e.done_bonus = self._arena_size, self._done_bonus
        e.never_done = int(self._never_done)
        e.max_episode_length = self.max_episode_length
        e.point, e.goal = self._point.data_ptr(), self._goal.data_ptr()
        e.t = self._t.data_ptr()
        e.success, e.task_id = success.data_ptr(), task_id.data_ptr()
        e.num_tasks, e.strategy = self.num_tasks, self._strategy
        e.mode = (_lib.TASK_ADD_ONEHOT if self._mode == 'add-onehot' else
                  _lib.TASK_VANILLA)
        e.seed = self.seed
        e.task_goals = self._task_goals.data_ptr()
        e.last_task = self._last_task.data_ptr()
        e.resets = self._resets.data_ptr()
        return e

    def step_env_infos(self):
        return {'success': self._success, 'task_id': self._task_id}

    def finish_env_infos(self, env_infos):
        if self._env_names is not None:
            env_infos['task_name'] = np.asarray(
                self._env_names)[env_infos['task_id']]

    def episode_infos_of(self, ep_env, info_at_end):
        return {'goal': self._goals_np[info_at_end('task_id')]}

    def native_env_ref(self, info_bufs):
        e = self._struct(info_bufs['success'], info_bufs['task_id'])
        return _lib.env_ref(self._KIND, e), e


# garage.envs.grid_world_env.MAPS by name ('F' / '.' free, 'S' start, 'W' / 'x'
# wall, 'H' / 'o' hole, 'G' goal)
GRID_MAPS = {
    'chain': ('G' + 'F' * 13 + 'S' + 'F' * 13 + 'G', ),
    '4x4_safe': ('SFFF', 'FWFW', 'FFFW', 'WFFG'),
    '4x4': ('SFFF', 'FHFH', 'FFFH', 'HFFG'),
    '8x8': ('SFFFFFFF', 'FFFFFFFF', 'FFFHFFFF', 'FFFFFHFF', 'FFFHFFFF',
            'FHHFFFHF', 'FHFFHFHF', 'FFFHFFFG'),
}
_GRID_CODES = {'F': 0, '.': 0, 'S': 0, 'W': 1, 'x': 1, 'H': 2, 'o': 2, 'G': 3}


def _grid_rows(desc):
    """A map name or a list of row strings -> the list of rows."""
    if isinstance(desc, str):
        if desc not in GRID_MAPS:
            raise ValueError('unknown grid map {!r} (known: {})'.format(
                desc, sorted(GRID_MAPS)))
        return list(GRID_MAPS[desc])
    rows = [str(r) for r in desc]
    if not rows or any(len(r) != len(rows[0]) for r in rows) or not rows[0]:
        raise ValueError('a grid map is a non-empty list of rows of one length')
    return rows


class GridWorldVecEnv(_DeviceVecEnv):
    """``n_envs`` copies of ``garage.envs.GridWorldEnv``
    (``envs/grid_world_env.py``) stepped by one HIP kernel, one thread per env.

    ``desc`` is a map name of the reference's ``MAPS``, a list of row strings,
    or a list of one such map per env (all of one shape).  The observation row
    is the one-hot of the cell, as a discrete observation is seen by the
    policies.  Deviations from the reference: the device batch does not draw
    the one ``np.random.choice(..., p=[1.])`` per step the reference draws (the
    global numpy RNG is not consumed), and ``max_episode_length`` must be
    finite.
    """

    _KIND = _lib.ENV_GRID
    _STATE = ('_state', '_t')

    def __init__(self, n_envs, desc='4x4', max_episode_length=None,
                 device=None):
        self.n_envs = int(n_envs)
        self.max_episode_length = _check_finite_length(max_episode_length)
        per_env = (isinstance(desc, (list, tuple)) and len(desc) > 0 and all(
            isinstance(d, (list, tuple)) or (isinstance(d, str) and d in
                                              GRID_MAPS) for d in desc))
        if per_env:
            if len(desc) != self.n_envs:
                raise ValueError('one map per env: {} maps for {} envs'.format(
                    len(desc), self.n_envs))
            maps = [_grid_rows(d) for d in desc]
        else:
            maps = [_grid_rows(desc)] * self.n_envs
        shape = (len(maps[0]), len(maps[0][0]))
        codes, start = [], []
        for rows in maps:
            if (len(rows), len(rows[0])) != shape:
                raise ValueError('every env map must have the shape {}'.format(
                    shape))
            flat = ''.join(rows)
            bad = set(flat) - set(_GRID_CODES)
            if bad:
                raise ValueError('unknown grid cells {}'.format(sorted(bad)))
            if flat.count('S') != 1:
                raise ValueError('a grid map needs exactly one S cell')
            codes.append([_GRID_CODES[c] for c in flat])
            start.append(flat.index('S'))
        self.rows, self.cols = shape
        self._map_np = np.asarray(codes, dtype=np.uint8)
        self._start_np = np.asarray(start, dtype=np.int32)
        self.spec = EnvSpec(Discrete(self.rows * self.cols), Discrete(4),
                            max_episode_length=self.max_episode_length)
        self._init_device(device)

    def _init_device(self, device):
        device = device or require_gpu()
        self._alloc(device)
        n = self.n_envs
        self._map = torch.from_numpy(self._map_np).to(device)
        self._start = torch.from_numpy(self._start_np).to(device)
        self._state = torch.zeros(n, dtype=torch.int32, device=device)
        self._t = torch.zeros(n, dtype=torch.int32, device=device)
        e = _lib.GridEnv()
        e.n, e.rows, e.cols = n, self.rows, self.cols
        e.max_episode_length = self.max_episode_length
        e.map, e.start = self._map.data_ptr(), self._start.data_ptr()
        e.state, e.t = self._state.data_ptr(), self._t.data_ptr()
        self._set_struct(e)


class _StateVecEnv(_DeviceVecEnv):
    """A seeded state-vector batch: an ``(n, S)`` float32 state, a step and a
    reset counter per member, Philox reset draws keyed ``(seed; env_id0 + i,
    the member's reset counter)`` and a finite ``max_episode_length`` whose
    last step is TIMEOUT (``rollout_dev.h``: ``StateEnv<K>``).  A kind states
    ``_KIND``, its ctypes struct ``_STRUCT``, the state width ``_S``, its spec
    (``_make_spec``) and, where they are not trivial, what ``set_state``
    accepts (``_check_states``) and the observations of states
    (``_observe``); its constructor names its own default length."""

    _STATE = ('_state', '_t', '_resets')
    env_info_specs = {}
    _STRUCT = None
    _S = 0

    def _init_batch(self, n_envs, max_episode_length, seed, env_id0, device):
        self.n_envs = int(n_envs)
        self.max_episode_length = _check_finite_length(max_episode_length)
        self.seed = int(seed)
        self.env_id0 = int(env_id0)
        self.spec = self._make_spec(self.max_episode_length)
        self._init_device(device)

    def _new_struct(self):
        return self._STRUCT()

    def _init_device(self, device):
        device = device or require_gpu()
        self._alloc(device)
        n = self.n_envs
        self._state = torch.zeros(n, self._S, dtype=torch.float32,
                                  device=device)
        self._t = torch.zeros(n, dtype=torch.int32, device=device)
        self._resets = torch.zeros(n, dtype=torch.int32, device=device)
        e = self._new_struct()
        e.n, e.env_id0 = n, self.env_id0
        e.max_episode_length = self.max_episode_length
        e.seed = self.seed
        e.state = self._state.data_ptr()
        e.t = self._t.data_ptr()
        e.resets = self._resets.data_ptr()
        self._set_struct(e)

    def _check_states(self, states):
        """Raises ``ValueError`` for ``(n, S)`` states the kind cannot hold."""

    def _observe(self, states):
        """The observations of ``(n, S)`` states (by default the states)."""
        return states

    def set_state(self, states):
        """Every member's state <- row of ``states`` (``(n, S)`` float32, what
        the kind's ``_check_states`` accepts); the current observations
        follow."""
        states = np.asarray(states, dtype=np.float32)
        if states.shape != (self.n_envs, self._S):
            raise ValueError('set_state needs an ({}, {}) array, got {}'.format(
                self.n_envs, self._S, states.shape))
        self._check_states(states)
        obs = self._observe(states)
        self._state.copy_(torch.from_numpy(states))
        self.obs[:, :obs.shape[1]].copy_(torch.from_numpy(obs))

    def get_state(self):
        """The ``(n, S)`` float32 states."""
        return self._state.cpu().numpy()


def _state_reset_draw(entry, width, seed, env_id, counter):
    """``ga_*_reset_draw``: the ``(width,)`` float32 state of one reset."""
    out = (C.c_float * width)()
    call(entry, int(seed), int(env_id), int(counter), out)
    return np.array(out, dtype=np.float32)


# what a host twin's ``step`` returns (garage's ``EnvStep`` fields)
StateEnvStep = collections.namedtuple(
    'StateEnvStep', ['action', 'reward', 'observation', 'env_info',
                     'step_type'])
CartPoleStep = PendulumStep = DoublePendulumStep = StateEnvStep
AcrobotStep = MountainCarStep = StateEnvStep
_F = np.float32


class _StateEnv:
    """One member of a :class:`_StateVecEnv` on the host: the bookkeeping every
    twin shares.  A kind states its spec (``_make_spec``), its reset draw
    (``_reset_draw``), ``advance`` and, where they are not trivial, ``observe``
    (the observation of a state), ``_action`` (what ``advance`` takes of a
    policy's action) and ``_advance``."""

    _S = 0

    def _init_twin(self, seed, env_id, max_episode_length):
        self.max_episode_length = _check_finite_length(max_episode_length)
        self.seed, self.env_id = int(seed), int(env_id)
        self.spec = self._make_spec(self.max_episode_length)
        self.resets = 0
        self.state = np.zeros(self._S, dtype=np.float32)
        self._t = 0

    @classmethod
    def observe(cls, state):
        """The observations of ``state`` (``(..., S)``): the states."""
        return np.array(state, dtype=np.float32)

    @staticmethod
    def _action(action):
        """The torque / force of a continuous kind."""
        return np.asarray(action, dtype=np.float32).reshape(-1)[0]

    def _advance(self, a):
        """``(state, observation, reward, done)`` after one step with ``a``."""
        new, obs, reward, done = self.advance(self.state, a)
        return new, obs, _F(reward), done

    def reset(self):
        self.state = self._reset_draw(self.seed, self.env_id, self.resets)
        self.resets += 1
        self._t = 0
        return self.observe(self.state), {}

    def step(self, action):
        self.state, obs, reward, done = self._advance(self._action(action))
        self._t += 1
        st = StepType.get_step_type(self._t, self.max_episode_length,
                                    bool(done))
        return StateEnvStep(action, reward, obs, {}, st)

    def close(self):
        pass


def _cartpole_spec(max_episode_length):
    return EnvSpec(Box(-np.inf, np.inf, (4, )), Discrete(2),
                   max_episode_length=max_episode_length)


class CartPoleVecEnv(_StateVecEnv):
    """``n_envs`` cart-poles (gym's ``CartPole-v1``: the same constants, Euler
    step, termination limits and reward 1 per step) stepped by one HIP kernel,
    one thread per env, inside the sampler's one-launch rollout.

    Observation ``(x, x_dot, theta, theta_dot)``, ``Discrete(2)`` actions
    (1 pushes right).  ``include/garage_amd.h`` states the arithmetic operation
    by operation; :class:`CartPoleEnv` is the per-env numpy twin that gives the
    same bits.  ``set_state`` / ``get_state`` move the ``(n, 4)`` float32 states
    (scripted starts; the step counters are left alone).

    Deviations from gym:

    - fp32 throughout, ``sin`` / ``cos`` as fixed polynomials (valid because an
      episode ends once ``|theta|`` passes 0.2094): one step differs from the
      float64 equations by a few 1e-7;
    - resets draw from Philox4x32-10 keyed ``(seed; env_id0 + i, the member's
      reset counter)`` instead of gym's ``np_random``
      (:func:`cartpole_reset_draw` gives the same state on the host);
    - ``max_episode_length`` must be finite (default 500, CartPole-v1's limit):
      the step that reaches it is TIMEOUT.
    """

    _KIND = _lib.ENV_CARTPOLE
    _STRUCT = _lib.CartPoleEnv
    _S = 4
    _make_spec = staticmethod(_cartpole_spec)

    def __init__(self, n_envs, max_episode_length=500, seed=0, env_id0=0,
                 device=None):
        self._init_batch(n_envs, max_episode_length, seed, env_id0, device)


def cartpole_reset_draw(seed, env_id, counter):
    """The ``(4,)`` float32 state reset number ``counter`` gives member
    ``env_id`` (= ``env_id0 + i``) of a :class:`CartPoleVecEnv` with this seed
    (host only, no GPU)."""
    return _state_reset_draw('ga_cartpole_reset_draw', 4, seed, env_id, counter)


class CartPoleEnv(_StateEnv):
    """One member of :class:`CartPoleVecEnv` on the host, in numpy fp32: the
    same operations in the same order (``include/garage_amd.h``) and the same
    Philox reset draws, so observations, rewards and step types equal the
    device batch's bit for bit.  garage's ``Environment`` shape --
    ``reset() -> (obs, {})``, ``step(a)`` with ``reward / observation /
    step_type`` -- so a list of them goes behind :class:`HostVecEnv`."""

    S3, S5, S7 = _F(-1.0 / 6.0), _F(1.0 / 120.0), _F(-1.0 / 5040.0)
    C2, C4, C6, C8 = (_F(-0.5), _F(1.0 / 24.0), _F(-1.0 / 720.0),
                      _F(1.0 / 40320.0))
    X_LIMIT = _F(2.4)
    THETA_LIMIT = _F(12.0 * 2.0 * 3.141592653589793 / 360.0)

    _S = 4
    _make_spec = staticmethod(_cartpole_spec)
    _reset_draw = staticmethod(cartpole_reset_draw)

    def __init__(self, seed=0, env_id=0, max_episode_length=500):
        self._init_twin(seed, env_id, max_episode_length)

    @classmethod
    def advance(cls, state, push_right):
        """One Euler step of ``state`` (``(..., 4)`` float32): the new states
        and ``done``.  Every line is one fp32 operation."""
        state = np.asarray(state, dtype=np.float32)
        x, xd, th, thd = (state[..., j] for j in range(4))
        one, total = _F(1.0), _F(1.1)
        force = np.where(push_right, _F(10.0), _F(-10.0)).astype(np.float32)
        t2 = th * th
        ps = t2 * cls.S7
        ps = cls.S5 + ps
        ps = t2 * ps
        ps = cls.S3 + ps
        ps = t2 * ps
        ps = one + ps
        sn = th * ps
        pc = t2 * cls.C8
        pc = cls.C6 + pc
        pc = t2 * pc
        pc = cls.C4 + pc
        pc = t2 * pc
        pc = cls.C2 + pc
        pc = t2 * pc
        cs = one + pc
        thd2 = thd * thd
        pl = _F(0.05) * thd2
        pls = pl * sn
        fsum = force + pls
        temp = fsum / total
        gs = _F(9.8) * sn
        ct = cs * temp
        num = gs - ct
        cs2 = cs * cs
        mc = _F(0.1) * cs2
        mct = mc / total
        br = _F(4.0 / 3.0) - mct
        den = _F(0.5) * br
        th_acc = num / den
        pa = _F(0.05) * th_acc
        pac = pa * cs
        pact = pac / total
        x_acc = temp - pact
        tau = _F(0.02)
        dx = tau * xd
        dxd = tau * x_acc
        dth = tau * thd
        dthd = tau * th_acc
        new = np.stack([x + dx, xd + dxd, th + dth, thd + dthd],
                       axis=-1).astype(np.float32)
        done = ((np.abs(new[..., 0]) > cls.X_LIMIT) |
                (np.abs(new[..., 2]) > cls.THETA_LIMIT))
        return new, done

    @staticmethod
    def _action(action):
        return int(action) == 1

    def _advance(self, push_right):
        new, done = self.advance(self.state, push_right)
        return new, new.copy(), 1.0, done


def _pendulum_spec(max_episode_length):
    high = np.array([1.0, 1.0, 8.0], dtype=np.float32)
    return EnvSpec(Box(-high, high), Box(-2.0, 2.0, (1, )),
                   max_episode_length=max_episode_length)


class PendulumVecEnv(_StateVecEnv):
    """``n_envs`` pendulums (gym 0.17's ``Pendulum-v0``: the same constants,
    update order, clips of torque and speed, cost and reset ranges) stepped by
    one HIP kernel, one thread per env, inside the sampler's one-launch rollout.

    Observation ``(cos th, sin th, thdot)`` in ``Box(-[1, 1, 8], [1, 1, 8])``,
    one torque in ``Box(-2, 2, (1,))``: the env clips the torque itself, so any
    float may be passed and the batch keeps the policy's own actions.  Reward
    ``-(th^2 + 0.1 thdot^2 + 0.001 u^2)`` of the state before the step.  An
    episode never terminates: every ending is TIMEOUT.
    ``include/garage_amd.h`` states the arithmetic operation by operation;
    :class:`PendulumEnv` is the per-env numpy twin that gives the same bits.
    ``set_state`` / ``get_state`` move the ``(n, 2)`` float32 states
    ``(th, thdot)`` (scripted starts; the step counters are left alone).

    Deviations from gym:

    - fp32 throughout (gym steps in float64 and casts the observation): one
      step differs from the float64 equations by less than 1e-6 in the
      observation and 3e-6 in the reward;
    - ``sin`` / ``cos`` are fixed polynomials on the angle folded to
      ``[-pi/2, pi/2]``, within 2e-7 of the functions;
    - the angle is kept wrapped to ``[-PI, PI]`` (gym lets it grow and wraps it
      in the cost): the observation is periodic and ``angle_normalize`` of a
      wrapped angle is the angle itself, so the dynamics are gym's;
    - resets draw from Philox4x32-10 keyed ``(seed; env_id0 + i, the member's
      reset counter)`` instead of gym's ``np_random``
      (:func:`pendulum_reset_draw` gives the same state on the host);
    - ``max_episode_length`` must be finite (default 200, Pendulum-v0's
      TimeLimit): the step that reaches it is TIMEOUT.
    """

    _KIND = _lib.ENV_PENDULUM
    _STRUCT = _lib.PendulumEnv
    _S = 2
    _make_spec = staticmethod(_pendulum_spec)

    def __init__(self, n_envs, max_episode_length=200, seed=0, env_id0=0,
                 device=None):
        self._init_batch(n_envs, max_episode_length, seed, env_id0, device)

    def _check_states(self, states):
        """``(th, thdot)`` rows with ``|th| <= PI``."""
        if not (np.abs(states[:, 0]) <= PendulumEnv.PI).all():
            raise ValueError('set_state needs angles in [-PI, PI]')

    def _observe(self, states):
        return PendulumEnv.observe(states)


def pendulum_reset_draw(seed, env_id, counter):
    """The ``(2,)`` float32 state ``(th, thdot)`` reset number ``counter`` gives
    member ``env_id`` (= ``env_id0 + i``) of a :class:`PendulumVecEnv` with this
    seed (host only, no GPU)."""
    return _state_reset_draw('ga_pendulum_reset_draw', 2, seed, env_id, counter)


def _fact(k):
    out = 1.0
    for j in range(2, k + 1):
        out *= j
    return out


class PendulumEnv(_StateEnv):
    """One member of :class:`PendulumVecEnv` on the host, in numpy fp32: the
    same operations in the same order (``include/garage_amd.h``) and the same
    Philox reset draws, so observations, rewards and step types equal the
    device batch's bit for bit.  garage's ``Environment`` shape --
    ``reset() -> (obs, {})``, ``step(a)`` with ``reward / observation /
    step_type`` -- so a list of them goes behind :class:`HostVecEnv`."""

    PI = _F(3.141592653589793)
    TWO_PI = _F(6.283185307179586)
    HALF_PI = _F(1.5707963267948966)
    # S[j] = S(2j + 3), C[j] = C(2j + 2): the Taylor coefficients rounded once
    S = tuple(_F((-1.0)**(j + 1) / _fact(2 * j + 3)) for j in range(6))
    C = tuple(_F((-1.0)**(j + 1) / _fact(2 * j + 2)) for j in range(7))

    _S = 2
    _make_spec = staticmethod(_pendulum_spec)
    _reset_draw = staticmethod(pendulum_reset_draw)

    def __init__(self, seed=0, env_id=0, max_episode_length=200):
        self._init_twin(seed, env_id, max_episode_length)

    @classmethod
    def sincos(cls, th):
        """``(sin, cos)`` of ``th`` (float32, ``|th| <= PI``), every line one
        fp32 operation."""
        th = np.asarray(th, dtype=np.float32)
        one = _F(1.0)
        hi = th > cls.HALF_PI
        lo = th < -cls.HALF_PI
        r_hi = cls.PI - th
        r_lo = (-cls.PI) - th
        r = np.where(hi, r_hi, np.where(lo, r_lo, th)).astype(np.float32)
        sg = np.where(hi | lo, _F(-1.0), one).astype(np.float32)
        t2 = r * r
        ps = t2 * cls.S[5]
        for j in (4, 3, 2, 1, 0):
            ps = cls.S[j] + ps
            ps = t2 * ps
        ps = one + ps
        sp = r * ps
        sn = np.where(sp < -one, -one, np.where(sp > one, one, sp))
        sn = sn.astype(np.float32)
        pc = t2 * cls.C[6]
        for j in (5, 4, 3, 2, 1, 0):
            pc = cls.C[j] + pc
            pc = t2 * pc
        pc = one + pc
        cs = sg * pc
        return sn, cs

    @classmethod
    def advance(cls, state, action):
        """One step of ``state`` (``(..., 2)`` float32 ``(th, thdot)``) with
        the torques ``action`` (``(...)``; clipped here): the new states, the
        observations ``(..., 3)`` and the rewards.  Every line is one fp32
        operation."""
        state = np.asarray(state, dtype=np.float32)
        a = np.asarray(action, dtype=np.float32)
        th, thd = state[..., 0], state[..., 1]
        two, eight = _F(2.0), _F(8.0)
        u = np.where(a < -two, -two, np.where(a > two, two, a))
        u = u.astype(np.float32)
        sn, _ = cls.sincos(th)
        c1 = th * th
        c2 = thd * thd
        c3 = _F(0.1) * c2
        c4 = c1 + c3
        c5 = u * u
        c6 = _F(0.001) * c5
        cost = c4 + c6
        g1 = _F(15.0) * sn
        g2 = _F(3.0) * u
        acc = g1 + g2
        dv = acc * _F(0.05)
        v = thd + dv
        dth = v * _F(0.05)
        nth = th + dth
        nthd = np.where(v < -eight, -eight, np.where(v > eight, eight, v))
        nthd = nthd.astype(np.float32)
        down = nth - cls.TWO_PI
        up = nth + cls.TWO_PI
        nth = np.where(nth >= cls.PI, down, np.where(nth < -cls.PI, up, nth))
        nth = nth.astype(np.float32)
        sn2, cs2 = cls.sincos(nth)
        new = np.stack([nth, nthd], axis=-1).astype(np.float32)
        obs = np.stack([cs2, sn2, nthd], axis=-1).astype(np.float32)
        return new, obs, (-cost).astype(np.float32)

    @classmethod
    def observe(cls, state):
        """The ``(..., 3)`` observations of ``state`` (``(..., 2)``, angles in
        ``[-PI, PI]``)."""
        state = np.asarray(state, dtype=np.float32)
        sn, cs = cls.sincos(state[..., 0])
        return np.stack([cs, sn, state[..., 1]], axis=-1).astype(np.float32)

    def _advance(self, a):
        new, obs, reward = self.advance(self.state, a)
        return new, obs, _F(reward), False  # an episode never terminates


def _double_pendulum_spec(max_episode_length):
    return EnvSpec(Box(-np.inf, np.inf, (11, )), Box(-1.0, 1.0, (1, )),
                   max_episode_length=max_episode_length)


class DoublePendulumVecEnv(_StateVecEnv):
    """``n_envs`` inverted double pendulums on a cart (the task of gym's
    ``InvertedDoublePendulum-v2``: the same bodies, action scale, frame skip,
    reward, termination and observation layout) stepped by one HIP kernel, one
    thread per env, inside the sampler's one-launch rollout.

    State ``(x, th1, th2, xd, th1d, th2d)`` with ``th1``, ``th2`` the rods'
    absolute angles from the upright.  Observation ``(x, sin th1,
    sin(th2 - th1), cos th1, cos(th2 - th1), xd, th1d, th2d - th1d`` clipped to
    ``+-10``, ``0, 0, 0)``, one push in ``Box(-1, 1, (1,))``: the env clips it
    itself, so any float may be passed and the batch keeps the policy's own
    actions.  Reward ``10 - (0.01 x_tip^2 + (y_tip - 2)^2) - (0.001 w1^2 +
    0.005 w2^2)`` of the new state; an episode terminates once ``y_tip <= 1``.
    ``include/garage_amd.h`` states the arithmetic operation by operation;
    :class:`DoublePendulumEnv` is the per-env numpy twin that gives the same
    bits.  ``set_state`` / ``get_state`` move the ``(n, 6)`` float32 states
    (scripted starts; the step counters are left alone).

    Deviations from MuJoCo's model (which cannot be matched bit for bit):

    - the capsule masses rounded (10.5, 4.2, 4.2), no joint damping (0.05 in
      the XML), no rail stops;
    - five semi-implicit Euler substeps of 0.01 instead of RK4, in fp32, with
      ``sin`` / ``cos`` as :class:`PendulumEnv`'s fixed polynomials;
    - the last three observation entries (MuJoCo's constraint forces) are 0;
    - resets draw all six states from ``U(-0.1, 0.1)`` (MuJoCo: Gaussian
      velocities) by Philox4x32-10 keyed ``(seed; env_id0 + i, the member's
      reset counter)`` (:func:`double_pendulum_reset_draw` gives the same
      state on the host);
    - ``max_episode_length`` must be finite (default 1000, the task's
      TimeLimit): the step that reaches it is TIMEOUT.
    """

    _KIND = _lib.ENV_DOUBLE_PENDULUM
    _STRUCT = _lib.DoublePendulumEnv
    _S = 6
    _make_spec = staticmethod(_double_pendulum_spec)

    def __init__(self, n_envs, max_episode_length=1000, seed=0, env_id0=0,
                 device=None):
        self._init_batch(n_envs, max_episode_length, seed, env_id0, device)

    def _check_states(self, states):
        """Rows with ``|th1|, |th2| <= PI``."""
        if not (np.abs(states[:, 1:3]) <= PendulumEnv.PI).all():
            raise ValueError('set_state needs angles in [-PI, PI]')

    def _observe(self, states):
        return DoublePendulumEnv.observe(states)


def double_pendulum_reset_draw(seed, env_id, counter):
    """The ``(6,)`` float32 state reset number ``counter`` gives member
    ``env_id`` (= ``env_id0 + i``) of a :class:`DoublePendulumVecEnv` with this
    seed (host only, no GPU)."""
    return _state_reset_draw('ga_double_pendulum_reset_draw', 6, seed, env_id,
                             counter)


def _clip32(v, b):
    return np.where(v < -b, -b, np.where(v > b, b, v)).astype(np.float32)


class DoublePendulumEnv(_StateEnv):
    """One member of :class:`DoublePendulumVecEnv` on the host, in numpy fp32:
    the same operations in the same order (``include/garage_amd.h``) and the
    same Philox reset draws, so observations, rewards and step types equal the
    device batch's bit for bit.  garage's ``Environment`` shape --
    ``reset() -> (obs, {})``, ``step(a)`` with ``reward / observation /
    step_type`` -- so a list of them goes behind :class:`HostVecEnv`."""

    M0, M1, M2, L, G = 10.5, 4.2, 4.2, 0.6, 9.81
    D1 = _F(M0 + M1 + M2)
    D2 = _F((M1 / 2.0 + M2) * L)
    D3 = _F(M2 * L / 2.0)
    D4 = _F((M1 / 3.0 + M2) * L * L)
    D5 = _F(M2 * L * L / 2.0)
    D6 = _F(M2 * L * L / 3.0)
    F1 = _F((M1 / 2.0 + M2) * L * G)
    F2 = _F(M2 * L * G / 2.0)
    H, VMAX, SUBSTEPS = _F(0.01), _F(100.0), 5

    _S = 6
    _make_spec = staticmethod(_double_pendulum_spec)
    _reset_draw = staticmethod(double_pendulum_reset_draw)

    def __init__(self, seed=0, env_id=0, max_episode_length=1000):
        self._init_twin(seed, env_id, max_episode_length)

    @staticmethod
    def _wrap(th):
        pi, two_pi = PendulumEnv.PI, PendulumEnv.TWO_PI
        down = th - two_pi
        up = th + two_pi
        return np.where(th >= pi, down,
                        np.where(th < -pi, up, th)).astype(np.float32)

    @classmethod
    def _trig(cls, th1, th2):
        """``s1, c1, s2, sd, cd, y_tip`` of the two angles."""
        s1, c1 = PendulumEnv.sincos(th1)
        s2, c2 = PendulumEnv.sincos(th2)
        cc = c1 * c2
        ss = s1 * s2
        sc = s1 * c2
        cs = c1 * s2
        y1 = _F(0.6) * c1
        y2 = _F(0.6) * c2
        return s1, c1, s2, sc - cs, cc + ss, y1 + y2

    @classmethod
    def _observe(cls, state, s1, c1, sd, cd):
        ten = _F(10.0)
        x, xd, th1d, th2d = (state[..., j] for j in (0, 3, 4, 5))
        w2 = th2d - th1d
        zero = np.zeros_like(x)
        return np.stack([x, s1, -sd, c1, cd, _clip32(xd, ten),
                         _clip32(th1d, ten), _clip32(w2, ten), zero, zero,
                         zero], axis=-1).astype(np.float32)

    @classmethod
    def observe(cls, state):
        """The ``(..., 11)`` observations of ``state`` (``(..., 6)``)."""
        state = np.asarray(state, dtype=np.float32)
        s1, c1, _, sd, cd, _ = cls._trig(state[..., 1], state[..., 2])
        return cls._observe(state, s1, c1, sd, cd)

    @classmethod
    def advance(cls, state, action):
        """One env step (five substeps) of ``state`` (``(..., 6)`` float32)
        with the pushes ``action`` (``(...)``; clipped here): the new states,
        the observations ``(..., 11)``, the rewards and ``done``.  Every line
        is one fp32 operation."""
        state = np.asarray(state, dtype=np.float32)
        a = np.asarray(action, dtype=np.float32)
        x, th1, th2, xd, th1d, th2d = (state[..., j] for j in range(6))
        D1, D2, D3, D4, D5, D6 = (cls.D1, cls.D2, cls.D3, cls.D4, cls.D5,
                                  cls.D6)
        H = cls.H
        u = _clip32(a, _F(1.0))
        F = _F(500.0) * u
        for _ in range(cls.SUBSTEPS):
            s1, c1 = PendulumEnv.sincos(th1)
            s2, c2 = PendulumEnv.sincos(th2)
            cc = c1 * c2
            ss = s1 * s2
            cd = cc + ss
            sc = s1 * c2
            cs = c1 * s2
            sd = sc - cs
            q1 = th1d * th1d
            q2 = th2d * th2d
            a12 = D2 * c1
            a13 = D3 * c2
            a23 = D5 * cd
            b1 = D2 * s1
            b2 = b1 * q1
            b3 = D3 * s2
            b4 = b3 * q2
            b5 = F + b2
            r1 = b5 + b4
            e1 = D5 * sd
            g1 = cls.F1 * s1
            e2 = e1 * q2
            r2 = g1 - e2
            g2 = cls.F2 * s2
            e3 = e1 * q1
            r3 = g2 + e3
            l21 = a12 / D1
            l31 = a13 / D1
            m1 = l21 * a12
            p22 = D4 - m1
            m2 = l21 * a13
            t23 = a23 - m2
            m3 = l31 * a13
            t33 = D6 - m3
            l32 = t23 / p22
            m4 = l32 * t23
            p33 = t33 - m4
            m5 = l21 * r1
            y2 = r2 - m5
            m6 = l31 * r1
            y3a = r3 - m6
            m7 = l32 * y2
            y3 = y3a - m7
            z1 = r1 / D1
            z2 = y2 / p22
            acc3 = y3 / p33
            m8 = l32 * acc3
            acc2 = z2 - m8
            m9 = l21 * acc2
            z1a = z1 - m9
            m10 = l31 * acc3
            acc1 = z1a - m10
            dv1 = H * acc1
            dv2 = H * acc2
            dv3 = H * acc3
            v1 = xd + dv1
            v2 = th1d + dv2
            v3 = th2d + dv3
            xd = _clip32(v1, cls.VMAX)
            th1d = _clip32(v2, cls.VMAX)
            th2d = _clip32(v3, cls.VMAX)
            dx = H * xd
            dt1 = H * th1d
            dt2 = H * th2d
            x = x + dx
            n1 = th1 + dt1
            n2 = th2 + dt2
            th1 = cls._wrap(n1)
            th2 = cls._wrap(n2)
        new = np.stack([x, th1, th2, xd, th1d, th2d],
                       axis=-1).astype(np.float32)
        s1, c1, s2, sd, cd, yt = cls._trig(th1, th2)
        xa = _F(0.6) * s1
        xb = _F(0.6) * s2
        xc = x + xa
        xt = xc + xb
        xt2 = xt * xt
        dist_x = _F(0.01) * xt2
        dy = yt - _F(2.0)
        dy2 = dy * dy
        dist = dist_x + dy2
        w2 = th2d - th1d
        w1s = th1d * th1d
        w2s = w2 * w2
        vp1 = _F(0.001) * w1s
        vp2 = _F(0.005) * w2s
        vel = vp1 + vp2
        alive = _F(10.0) - dist
        reward = (alive - vel).astype(np.float32)
        obs = cls._observe(new, s1, c1, sd, cd)
        return new, obs, reward, yt <= _F(1.0)


def _acrobot_spec(max_episode_length):
    high = np.array([1.0, 1.0, 1.0, 1.0, AcrobotEnv.MAX_VEL_1,
                     AcrobotEnv.MAX_VEL_2], dtype=np.float32)
    return EnvSpec(Box(-high, high), Discrete(3),
                   max_episode_length=max_episode_length)


class AcrobotVecEnv(_StateVecEnv):
    """``n_envs`` acrobots (gym 0.17's ``Acrobot-v1``: the "book" dynamics, no
    torque noise, one classical RK4 step of 0.2 s, the same speed bounds,
    reward and goal) stepped by one HIP kernel, one thread per env, inside the
    sampler's one-launch rollout.

    State ``(th1, th2, thd1, thd2)`` with both angles kept in ``[-PI, PI]``.
    Observation ``(cos th1, sin th1, cos th2, sin th2, thd1, thd2)`` in gym's
    ``Box``, ``Discrete(3)`` actions: class 0 is torque -1, class 2 torque +1,
    anything else (1, and any index out of range) no torque.  Reward -1 per
    step and 0 on the step that swings the tip above the line,
    ``-cos th1 - cos(th1 + th2) > 1``, which is TERMINAL.
    ``include/garage_amd.h`` states the arithmetic operation by operation;
    :class:`AcrobotEnv` is the per-env numpy twin that gives the same bits.
    ``set_state`` / ``get_state`` move the ``(n, 4)`` float32 states (scripted
    starts; the step counters are left alone).

    Deviations from gym:

    - fp32 throughout, ``sin`` / ``cos`` as :class:`PendulumEnv`'s fixed
      polynomials behind a two-constant reduction of the RK4 stage angles
      (which leave ``[-PI, PI]`` by far), ``sin(th1 + th2)`` by the addition
      theorem;
    - the angles are wrapped by that reduction instead of ``mod``;
    - resets draw from Philox4x32-10 keyed ``(seed; env_id0 + i, the member's
      reset counter)`` instead of gym's ``np_random``
      (:func:`acrobot_reset_draw` gives the same state on the host);
    - ``max_episode_length`` must be finite (default 500, Acrobot-v1's
      TimeLimit): the step that reaches it is TIMEOUT.
    """

    _KIND = _lib.ENV_ACROBOT
    _STRUCT = _lib.AcrobotEnv
    _S = 4

    _make_spec = staticmethod(_acrobot_spec)

    def __init__(self, n_envs, max_episode_length=500, seed=0, env_id0=0,
                 device=None):
        self._init_batch(n_envs, max_episode_length, seed, env_id0, device)

    def _check_states(self, states):
        """Rows with the angles in ``[-PI, PI]`` and the speeds inside their
        clips."""
        if not (np.abs(states[:, :2]) <= AcrobotEnv.PI).all():
            raise ValueError('set_state needs angles in [-PI, PI]')
        if not ((np.abs(states[:, 2]) <= AcrobotEnv.MAX_VEL_1).all() and
                (np.abs(states[:, 3]) <= AcrobotEnv.MAX_VEL_2).all()):
            raise ValueError('set_state needs speeds within 4 pi and 9 pi')

    def _observe(self, states):
        return AcrobotEnv.observe(states)


def acrobot_reset_draw(seed, env_id, counter):
    """The ``(4,)`` float32 state reset number ``counter`` gives member
    ``env_id`` (= ``env_id0 + i``) of an :class:`AcrobotVecEnv` with this seed
    (host only, no GPU)."""
    return _state_reset_draw('ga_acrobot_reset_draw', 4, seed, env_id, counter)


class AcrobotEnv(_StateEnv):
    """One member of :class:`AcrobotVecEnv` on the host, in numpy fp32: the
    same operations in the same order (``include/garage_amd.h``) and the same
    Philox reset draws, so observations, rewards and step types equal the
    device batch's bit for bit.  garage's ``Environment`` shape --
    ``reset() -> (obs, {})``, ``step(a)`` with ``reward / observation /
    step_type`` -- so a list of them goes behind :class:`HostVecEnv`."""

    PI, TWO_PI = PendulumEnv.PI, PendulumEnv.TWO_PI
    INV_TWO_PI = _F(1.0 / 6.283185307179586)
    # TWO_PI in two parts: R_HI has 9 significant bits, so k * R_HI is exact
    R_HI = _F(6.28125)
    R_LO = _F(6.283185307179586 - 6.28125)
    MAX_VEL_1 = _F(4.0 * 3.141592653589793)
    MAX_VEL_2 = _F(9.0 * 3.141592653589793)
    H, H2, H6 = _F(0.2), _F(0.1), _F(0.2 / 6.0)

    _S = 4
    _make_spec = staticmethod(_acrobot_spec)
    _reset_draw = staticmethod(acrobot_reset_draw)

    def __init__(self, seed=0, env_id=0, max_episode_length=500):
        self._init_twin(seed, env_id, max_episode_length)

    @classmethod
    def reduce(cls, th):
        """``th`` (float32, any stage angle) brought into ``[-PI, PI]``."""
        th = np.asarray(th, dtype=np.float32)
        q = th * cls.INV_TWO_PI
        k = np.rint(q)
        m1 = k * cls.R_HI
        r1 = th - m1
        m2 = k * cls.R_LO
        r = r1 - m2
        down = r - cls.TWO_PI
        up = r + cls.TWO_PI
        return np.where(r >= cls.PI, down,
                        np.where(r < -cls.PI, up, r)).astype(np.float32)

    @classmethod
    def torque(cls, action):
        """The torque of the class indices ``action``: 0 -> -1, 2 -> +1,
        anything else 0."""
        a = np.asarray(action)
        return np.where(a == 0, _F(-1.0),
                        np.where(a == 2, _F(1.0), _F(0.0))).astype(np.float32)

    @classmethod
    def dynamics(cls, th1, th2, w1, w2, a):
        """``(acc1, acc2)`` of the book dynamics at the (unreduced) angles and
        speeds under torque ``a``; every line one fp32 operation."""
        s1, c1 = PendulumEnv.sincos(cls.reduce(th1))
        s2, c2 = PendulumEnv.sincos(cls.reduce(th2))
        d1 = _F(3.5) + c2
        hc = _F(0.5) * c2
        d2 = _F(1.25) + hc
        sc = s1 * c2
        cs = c1 * s2
        s12 = sc + cs
        phi2 = _F(4.9) * s12
        q2 = w2 * w2
        p1 = _F(-0.5) * q2
        p2 = p1 * s2
        p3 = w2 * w1
        p4 = p3 * s2
        p5 = p2 - p4
        p6 = _F(14.7) * s1
        p7 = p6 + phi2
        phi1 = p5 + p7
        r = d2 / d1
        e1 = r * phi1
        e2 = a + e1
        q1 = w1 * w1
        e3 = _F(0.5) * q1
        e4 = e3 * s2
        e5 = e2 - e4
        e6 = e5 - phi2
        e7 = d2 * r
        den = _F(1.25) - e7
        acc2 = e6 / den
        g1 = d2 * acc2
        g2 = g1 + phi1
        g3 = g2 / d1
        acc1 = -g3
        return acc1, acc2

    @classmethod
    def observe(cls, state):
        """The ``(..., 6)`` observations of ``state`` (``(..., 4)``, angles in
        ``[-PI, PI]``)."""
        state = np.asarray(state, dtype=np.float32)
        s1, c1 = PendulumEnv.sincos(state[..., 0])
        s2, c2 = PendulumEnv.sincos(state[..., 1])
        return np.stack([c1, s1, c2, s2, state[..., 2], state[..., 3]],
                        axis=-1).astype(np.float32)

    @classmethod
    def advance(cls, state, action):
        """One env step (one RK4 step of 0.2) of ``state`` (``(..., 4)``
        float32) with the class indices ``action`` (``(...)``): the new states,
        the observations ``(..., 6)``, the rewards and ``done``.  Every line
        is one fp32 operation."""
        state = np.asarray(state, dtype=np.float32)
        a = cls.torque(action)
        th1, th2, w1, w2 = (state[..., j] for j in range(4))
        H, H2, H6, two = cls.H, cls.H2, cls.H6, _F(2.0)
        # k1 = (w1, w2, a1, a2)
        a1, a2 = cls.dynamics(th1, th2, w1, w2, a)
        s_t1, s_t2, s_w1, s_w2 = w1, w2, a1, a2
        k = (w1, w2, a1, a2)
        for h, wt in ((H2, two), (H2, two), (H, None)):
            dt1 = h * k[0]
            dt2 = h * k[1]
            dw1 = h * k[2]
            dw2 = h * k[3]
            y1 = th1 + dt1
            y2 = th2 + dt2
            v1 = w1 + dw1
            v2 = w2 + dw2
            a1, a2 = cls.dynamics(y1, y2, v1, v2, a)
            k = (v1, v2, a1, a2)
            if wt is None:
                s_t1 = s_t1 + k[0]
                s_t2 = s_t2 + k[1]
                s_w1 = s_w1 + k[2]
                s_w2 = s_w2 + k[3]
            else:
                s_t1 = s_t1 + wt * k[0]
                s_t2 = s_t2 + wt * k[1]
                s_w1 = s_w1 + wt * k[2]
                s_w2 = s_w2 + wt * k[3]
        n1 = th1 + H6 * s_t1
        n2 = th2 + H6 * s_t2
        u1 = w1 + H6 * s_w1
        u2 = w2 + H6 * s_w2
        nth1 = cls.reduce(n1)
        nth2 = cls.reduce(n2)
        nw1 = _clip32(u1, cls.MAX_VEL_1)
        nw2 = _clip32(u2, cls.MAX_VEL_2)
        s1, c1 = PendulumEnv.sincos(nth1)
        s2, c2 = PendulumEnv.sincos(nth2)
        cc = c1 * c2
        ss = s1 * s2
        c12 = cc - ss
        hgt = (-c1) - c12
        done = hgt > _F(1.0)
        reward = np.where(done, _F(0.0), _F(-1.0)).astype(np.float32)
        new = np.stack([nth1, nth2, nw1, nw2], axis=-1).astype(np.float32)
        obs = np.stack([c1, s1, c2, s2, nw1, nw2], axis=-1).astype(np.float32)
        return new, obs, reward, done

    @staticmethod
    def _action(action):
        return int(np.asarray(action).reshape(-1)[0])


def _mountain_car_spec(continuous, max_episode_length):
    low = np.array([-1.2, -0.07], dtype=np.float32)
    high = np.array([0.6, 0.07], dtype=np.float32)
    act = Box(-1.0, 1.0, (1, )) if continuous else Discrete(3)
    return EnvSpec(Box(low, high), act, max_episode_length=max_episode_length)


def _mountain_car_length(continuous, max_episode_length):
    if max_episode_length is None:
        return 999 if continuous else 200
    return _check_finite_length(max_episode_length)


class MountainCarVecEnv(_StateVecEnv):
    """``n_envs`` mountain cars (gym 0.17's ``MountainCar-v0``, or with
    ``continuous=True`` its ``MountainCarContinuous-v0``: the same constants,
    update order, clips, wall, goals and rewards) stepped by one HIP kernel,
    one thread per env, inside the sampler's one-launch rollout.

    State and observation ``(x, v)`` in ``Box([-1.2, -0.07], [0.6, 0.07])``.
    Discrete variant: ``Discrete(3)``, class 0 pushes left, class 2 right,
    anything else coasts; reward -1 every step; TERMINAL once ``x >= 0.5`` with
    ``v >= 0``.  Continuous variant: one force in ``Box(-1, 1, (1,))`` which
    the env clips itself (the batch keeps the policy's own actions); reward
    ``100`` on reaching ``x >= 0.45`` minus ``0.1 a^2`` of the UNCLIPPED
    action, as in gym.  ``include/garage_amd.h`` states the arithmetic
    operation by operation; :class:`MountainCarEnv` is the per-env numpy twin
    that gives the same bits.  ``set_state`` / ``get_state`` move the
    ``(n, 2)`` float32 states (scripted starts; the step counters are left
    alone).

    Deviations from gym:

    - fp32 throughout, ``cos(3 x)`` as :class:`PendulumEnv`'s fixed polynomial;
    - resets draw ``x`` from Philox4x32-10 keyed ``(seed; env_id0 + i, the
      member's reset counter)`` instead of gym's ``np_random``
      (:func:`mountain_car_reset_draw` gives the same state on the host);
    - ``max_episode_length`` must be finite: ``None`` selects the variant's
      TimeLimit (200, continuous 999); the step that reaches it is TIMEOUT.
    """

    _KIND = _lib.ENV_MOUNTAIN_CAR
    _S = 2

    def __init__(self, n_envs, continuous=False, max_episode_length=None,
                 seed=0, env_id0=0, device=None):
        self.continuous = bool(continuous)
        self._init_batch(
            n_envs, _mountain_car_length(self.continuous, max_episode_length),
            seed, env_id0, device)

    def _make_spec(self, max_episode_length):
        return _mountain_car_spec(self.continuous, max_episode_length)

    def _new_struct(self):
        return _lib.MountainCarEnv(continuous=int(self.continuous))

    def _check_states(self, states):
        """``(x, v)`` rows inside the observation ``Box``."""
        box = self.spec.observation_space
        if not ((states >= box.low).all() and (states <= box.high).all()):
            raise ValueError('set_state needs x in [-1.2, 0.6] and v in '
                             '[-0.07, 0.07]')


def mountain_car_reset_draw(seed, env_id, counter):
    """The ``(2,)`` float32 state ``(x, 0)`` reset number ``counter`` gives
    member ``env_id`` (= ``env_id0 + i``) of a :class:`MountainCarVecEnv` with
    this seed, either variant (host only, no GPU)."""
    return _state_reset_draw('ga_mountain_car_reset_draw', 2, seed, env_id,
                             counter)


class MountainCarEnv(_StateEnv):
    """One member of :class:`MountainCarVecEnv` on the host, in numpy fp32:
    the same operations in the same order (``include/garage_amd.h``) and the
    same Philox reset draws, so observations, rewards and step types equal the
    device batch's bit for bit.  garage's ``Environment`` shape --
    ``reset() -> (obs, {})``, ``step(a)`` with ``reward / observation /
    step_type`` -- so a list of them goes behind :class:`HostVecEnv`."""

    MIN_X, MAX_X, MAX_V = _F(-1.2), _F(0.6), _F(0.07)
    GOAL, GOAL_CONTINUOUS = _F(0.5), _F(0.45)
    _S = 2
    _reset_draw = staticmethod(mountain_car_reset_draw)

    def __init__(self, seed=0, env_id=0, continuous=False,
                 max_episode_length=None):
        self.continuous = bool(continuous)
        self._init_twin(
            seed, env_id,
            _mountain_car_length(self.continuous, max_episode_length))

    def _make_spec(self, max_episode_length):
        return _mountain_car_spec(self.continuous, max_episode_length)

    @classmethod
    def advance(cls, state, action, continuous=False):
        """One step of ``state`` (``(..., 2)`` float32 ``(x, v)``) with the
        class indices (or, ``continuous``, the forces) ``action`` (``(...)``):
        the new states, the observations (the new states), the rewards and
        ``done``.  Every line is one fp32 operation."""
        state = np.asarray(state, dtype=np.float32)
        x, v = state[..., 0], state[..., 1]
        x3 = _F(3.0) * x
        up = x3 + PendulumEnv.TWO_PI
        down = x3 - PendulumEnv.TWO_PI
        ang = np.where(x3 >= PendulumEnv.PI, down,
                       np.where(x3 < -PendulumEnv.PI, up, x3))
        _, cs = PendulumEnv.sincos(ang.astype(np.float32))
        if continuous:
            a = np.asarray(action, dtype=np.float32)
            u = _clip32(a, _F(1.0))
            f1 = u * _F(0.0015)
            f2 = _F(0.0025) * cs
            dv = f1 - f2
        else:
            k = np.asarray(action)
            push = np.where(k == 0, _F(-1.0),
                            np.where(k == 2, _F(1.0),
                                     _F(0.0))).astype(np.float32)
            f1 = push * _F(0.001)
            f2 = cs * _F(-0.0025)
            dv = f1 + f2
        v1 = v + dv
        nv = _clip32(v1, cls.MAX_V)
        x1 = x + nv
        nx = np.where(x1 < cls.MIN_X, cls.MIN_X,
                      np.where(x1 > cls.MAX_X, cls.MAX_X,
                               x1)).astype(np.float32)
        wall = (nx == cls.MIN_X) & (nv < _F(0.0))
        nv = np.where(wall, _F(0.0), nv).astype(np.float32)
        goal = cls.GOAL_CONTINUOUS if continuous else cls.GOAL
        done = (nx >= goal) & (nv >= _F(0.0))
        if continuous:
            a2 = a * a
            cost = _F(0.1) * a2
            bonus = np.where(done, _F(100.0), _F(0.0)).astype(np.float32)
            reward = (bonus - cost).astype(np.float32)
        else:
            reward = np.full(np.shape(nx), -1.0, dtype=np.float32)
        new = np.stack([nx, nv], axis=-1).astype(np.float32)
        return new, new.copy(), reward, done

    def _action(self, action):
        if self.continuous:
            return _StateEnv._action(action)
        return int(np.asarray(action).reshape(-1)[0])

    def _advance(self, a):
        new, obs, reward, done = self.advance(self.state, a, self.continuous)
        return new, obs, _F(reward), done


class NormalizedVecEnv(VecEnv):
    """``garage.envs.normalize`` for a device batch (``envs/normalized_env.py``).

    Wraps any :class:`VecEnv`; keeps one float64 moving mean / variance per
    member env (the reference deep-copies a ``NormalizedEnv`` per env, so the
    statistics are per env there too) and normalises every observation the
    policy sees -- first observations, next observations and terminal ones --
    with the statistics updated *by that observation* (``:144-147``).  Rewards
    are scaled by ``scale_reward`` and optionally normalised the same way.
    Actions of a ``Box`` action space whose bounds pass the reference's test
    (``:92-94``: no ``-inf`` in ``low`` **or in ``high``** -- its check of the
    upper bound compares with ``-inf`` too, which is kept) are rescaled from
    ``[-expected_action_scale, expected_action_scale]`` to ``[low, high]`` and
    clipped before the wrapped env steps on them (``:90-100``); the batch keeps
    the policy's own actions, as ``EnvStep.action`` does (``:109``).  Same
    keywords, order and defaults as ``garage.envs.normalize``.
    """

    def __init__(self, env, scale_reward=1., normalize_obs=False,
                 normalize_reward=False, expected_action_scale=1.,
                 flatten_obs=True, obs_alpha=0.001, reward_alpha=0.001):
        self._env = env
        self.n_envs = env.n_envs
        self.spec = env.spec
        self._scale_reward = float(scale_reward)
        self._normalize_reward = bool(normalize_reward)
        self._normalize_obs = bool(normalize_obs)
        self._expected_action_scale = float(expected_action_scale)
        # observations of a device batch are flat rows either way
        self._flatten_obs = bool(flatten_obs)
        self._obs_alpha = float(obs_alpha)
        self._reward_alpha = float(reward_alpha)
        dev = env.device
        self.device = dev
        self._act_low = self._act_high = self._scaled = None
        space = env.spec.action_space
        if isinstance(space, Box):
            lb = np.asarray(space.low, dtype=np.float32).reshape(-1)
            ub = np.asarray(space.high, dtype=np.float32).reshape(-1)
            if np.all(lb != -np.inf) and np.all(ub != -np.inf):
                self._act_low = torch.from_numpy(lb.copy()).to(dev)
                self._act_high = torch.from_numpy(ub.copy()).to(dev)
                self._scaled = torch.zeros(self.n_envs, round4(lb.size),
                                           dtype=torch.float32, device=dev)
        n, O = self.n_envs, env.obs_dim
        self._obs_mean = torch.zeros(n, O, dtype=torch.float64, device=dev)
        self._obs_var = torch.ones(n, O, dtype=torch.float64, device=dev)
        self._reward_mean = torch.zeros(n, dtype=torch.float64, device=dev)
        self._reward_var = torch.ones(n, dtype=torch.float64, device=dev)
        # the wrapped env keeps its own (raw) observations -- its dynamics must
        # not see the normalised ones, exactly as the inner env of the
        # reference's wrapper does not; the policy reads these
        if self._normalize_obs:
            self._obs = torch.zeros_like(env.obs)
            self._next_obs = torch.zeros_like(env.next_obs)

    # buffers under the protocol names: normalised copies when observations are
    # normalised, else the wrapped env's own
    obs = property(lambda self: self._obs if self._normalize_obs
                   else self._env.obs)
    next_obs = property(lambda self: self._next_obs if self._normalize_obs
                        else self._env.next_obs)
    reward = property(lambda self: self._env.reward)
    step_type = property(lambda self: self._env.step_type)
    env_id0 = property(lambda self: getattr(self._env, 'env_id0', 0))

    @property
    def last_env_infos(self):
        """Pass-through of a wrapped CPU env batch's per-step ``env_info``."""
        return getattr(self._env, 'last_env_infos', None)

    def pop_finished_episode_infos(self):
        pop = getattr(self._env, 'pop_finished_episode_infos', None)
        return pop() if pop is not None else []

    env_info_specs = property(lambda self: self._env.env_info_specs)

    def step_env_infos(self):
        return self._env.step_env_infos()

    def device_episode_infos(self):
        return self._env.device_episode_infos()

    def finish_env_infos(self, env_infos):
        self._env.finish_env_infos(env_infos)

    def episode_infos_of(self, ep_env, info_at_end):
        return self._env.episode_infos_of(ep_env, info_at_end)

    def advance(self):
        self._env.advance()
        if self._normalize_obs:
            self._obs, self._next_obs = self._next_obs, self._obs

    def hold(self):
        self._env.hold()
        if self._normalize_obs:
            self._next_obs.copy_(self._obs)

    def _norm(self, src, dst, mask=None):
        if self._normalize_obs:
            call('ga_obs_normalize_from_f64', self.n_envs, self.obs_dim,
                 dptr(src), dptr(dst), src.stride(0), dptr(self._obs_mean),
                 dptr(self._obs_var), self._obs_alpha, dptr(mask),
                 stream_ptr())

    def reset_all(self):
        self._env.reset_all()
        self._norm(self._env.obs, self.obs)

    def step_all(self, actions):
        if self._act_low is not None:
            A = self._act_low.numel()
            call('ga_action_rescale_f32', self.n_envs, A, dptr(actions),
                 actions.stride(0), dptr(self._act_low), dptr(self._act_high),
                 self._expected_action_scale, dptr(self._scaled),
                 self._scaled.stride(0), stream_ptr())
            actions = self._scaled
        self._env.step_all(actions)
        self._norm(self._env.next_obs, self.next_obs)
        if self._normalize_reward or self._scale_reward != 1.0:
            call('ga_reward_normalize_f64', self.n_envs,
                 dptr(self._env.reward), dptr(self._reward_mean),
                 dptr(self._reward_var), self._reward_alpha,
                 self._scale_reward, int(self._normalize_reward),
                 stream_ptr())

    def reset_where(self, done):
        self._env.reset_where(done)
        self._norm(self._env.next_obs, self.next_obs, done)

    def norm_args(self):
        """``ga_norm_args`` for the fused env-step kernel (raw buffers are
        filled in by the caller)."""
        from garage_amd import _lib
        a = _lib.NormArgs()
        a.normalize_obs = int(self._normalize_obs)
        a.normalize_reward = int(self._normalize_reward)
        a.obs_mean, a.obs_var = (self._obs_mean.data_ptr(),
                                 self._obs_var.data_ptr())
        a.obs_alpha = self._obs_alpha
        a.reward_mean, a.reward_var = (self._reward_mean.data_ptr(),
                                       self._reward_var.data_ptr())
        a.reward_alpha, a.reward_scale = (self._reward_alpha,
                                          self._scale_reward)
        if self._act_low is not None:
            a.act_low, a.act_high = (self._act_low.data_ptr(),
                                     self._act_high.data_ptr())
            a.expected_action_scale = self._expected_action_scale
            a.scaled_action = self._scaled.data_ptr()
        return a

    def close(self):
        self._env.close()


class HostVecEnv(VecEnv):
    """Adapter: a list of per-env CPU objects behind the batched protocol.

    Each member follows garage's ``Environment`` contract
    (``_environment.py:237-276``): ``reset() -> (obs, episode_info)`` and
    ``step(action) -> EnvStep`` with ``.reward``, ``.observation``,
    ``.step_type``.  Stepping stays a host loop (that is what those simulators
    are).  Per step the actions come down through a pinned buffer (the one
    stream synchronisation of the step: the simulators need them), the
    simulators write observations / rewards / step types straight into numpy
    views of pinned staging buffers, and those go up with asynchronous copies
    on the worker's stream -- the next step's synchronisation is what makes the
    staging buffers reusable.  Everything downstream stays on the device.
    """

    def __init__(self, envs, spec=None, device=None):
        self.envs = list(envs)
        self.n_envs = len(self.envs)
        self.spec = spec if spec is not None else self.envs[0].spec
        self._alloc(device or require_gpu())
        n, ldo = self.n_envs, self.obs.shape[1]
        self._h_obs = torch.zeros(n, ldo, dtype=torch.float32).pin_memory()
        self._h_rew = torch.zeros(n, dtype=torch.float32).pin_memory()
        self._h_st = torch.zeros(n, dtype=torch.uint8).pin_memory()
        self._h_done = torch.zeros(n, dtype=torch.uint8).pin_memory()
        self._h_act = None  # pinned, sized at the first step
        # numpy views of the pinned buffers: the simulators' outputs land in
        # page-locked memory without a per-element tensor operation
        self._np_obs = self._h_obs.numpy()
        self._np_rew = self._h_rew.numpy()
        self._np_st = self._h_st.numpy()
        self.discrete = is_discrete(self.spec.action_space)
        self._obs_discrete = is_discrete(self.spec.observation_space)
        # the last step's ``EnvStep.env_info`` per env (None when every env
        # reported an empty dict); the worker files them per rollout column and
        # packs them into ``EpisodeBatch.env_infos`` (vec_worker.py:192-193)
        self.last_env_infos = None
        # ``reset()[1]`` of the episode each env is in (default_worker.py:94-96),
        # and -- since the last call of pop_finished_episode_infos -- those of the
        # episodes that ended, as (env index, episode_info)
        self._episode_info = [{} for _ in range(n)]
        self._finished = []

    def _put_obs(self, i, obs):
        # discrete observation spaces are seen one-hot by the networks, as
        # ``observation_space.flatten`` makes them for garage's policies
        # (torch/policies/stochastic_policy.py:70-74)
        row = self._np_obs[i]
        if self._obs_discrete:
            row[:] = 0.0
            row[int(obs)] = 1.0
        else:
            flat = np.asarray(obs, dtype=np.float32).reshape(-1)
            row[:flat.shape[0]] = flat

    def _reset_member(self, i):
        obs, info = self.envs[i].reset()
        self._put_obs(i, obs)
        self._episode_info[i] = dict(info or {})

    def reset_all(self):
        torch.cuda.current_stream().synchronize()  # staging buffers are free
        for i in range(self.n_envs):
            self._reset_member(i)
        self._finished = []
        self.obs.copy_(self._h_obs, non_blocking=True)

    def step_all(self, actions):
        if self._h_act is None or self._h_act.shape != actions.shape:
            self._h_act = torch.zeros(actions.shape,
                                      dtype=torch.float32).pin_memory()
        self._h_act.copy_(actions, non_blocking=True)
        # the one synchronisation of the step (it also retires the previous
        # step's uploads from the staging buffers written below)
        torch.cuda.current_stream().synchronize()
        acts = self._h_act.numpy()
        infos, any_info = [], False
        width = self.act_width
        for i, env in enumerate(self.envs):
            a = int(acts[i, 0]) if self.discrete else acts[i, :width]
            es = env.step(a)
            self._put_obs(i, es.observation)
            self._np_rew[i] = es.reward
            self._np_st[i] = int(es.step_type)
            info = getattr(es, 'env_info', None) or {}
            any_info = any_info or bool(info)
            infos.append(info)
        self.last_env_infos = infos if any_info else None
        self.next_obs.copy_(self._h_obs, non_blocking=True)
        self.reward.copy_(self._h_rew, non_blocking=True)
        self.step_type.copy_(self._h_st, non_blocking=True)

    def reset_where(self, done):
        self._h_done.copy_(done, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        idx = np.nonzero(self._h_done.numpy())[0]
        if idx.size == 0:
            return
        # the staging buffer still holds the rows just uploaded to next_obs
        # unless somebody else wrote that tensor (hold() after advance()):
        # fetch them so that rows which are not reset keep their state
        self._h_obs.copy_(self.next_obs)
        for i in idx:
            self._finished.append((int(i), self._episode_info[int(i)]))
            self._reset_member(int(i))
        self.next_obs.copy_(self._h_obs, non_blocking=True)

    def pop_finished_episode_infos(self):
        """``(env index, episode_info)`` of the episodes that ended since the
        last call, in the order they were reset."""
        out, self._finished = self._finished, []
        return out

    def close(self):
        for env in self.envs:
            env.close()


__all__ = ['VecEnv', 'SyntheticVecEnv', 'PointVecEnv', 'GridWorldVecEnv',
           'MultiTaskPointVecEnv', 'round_robin_strategy',
           'uniform_random_strategy', 'task_draw', 'GRID_MAPS',
           'CartPoleVecEnv', 'CartPoleEnv', 'cartpole_reset_draw',
           'PendulumVecEnv', 'PendulumEnv', 'pendulum_reset_draw',
           'DoublePendulumVecEnv', 'DoublePendulumEnv',
           'double_pendulum_reset_draw',
           'AcrobotVecEnv', 'AcrobotEnv', 'acrobot_reset_draw',
           'MountainCarVecEnv', 'MountainCarEnv', 'mountain_car_reset_draw',
           'NormalizedVecEnv', 'HostVecEnv', 'StepType']
