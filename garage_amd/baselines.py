"""``LinearFeatureBaseline``: garage's closed-form baseline, device resident.

Mirrors ``garage.np.baselines.LinearFeatureBaseline``
(``np/baselines/linear_feature_baseline.py``): a ridge regression of the returns
on ``[clip(obs), clip(obs)**2, al, al**2, al**3, 1]`` with ``al = t / 100``.  The
one pass over the batch -- the feature rows, their Gram matrix and right-hand side
in fp64 -- is a HIP kernel (``ga_linear_features_gram_f64``); the ``F x F`` solve
is the reference's own ``np.linalg.lstsq`` on the host, unchanged; the
predictions are a second kernel (``ga_linear_features_predict_f32``).

Two surfaces: the reference's (``fit(paths)`` / ``predict(path)`` on dicts of
numpy arrays, ``get_param_values`` / ``set_param_values``) and the one the algos
use (``fit_batch`` / ``predict_batch`` on a :class:`DeviceEpisodeBatch`, and the
two halves ``begin_fit`` / ``finish_fit`` of a fit, between which a caller may
enqueue other work: the host solve then runs while those kernels execute).

The observations are fp32 as every batch here holds them; the reference's result
for float64 copies of the same fp32 observations is what the tests pin.
"""
import numpy as np
import torch

from garage_amd import _lib
from garage_amd._lib import call, dptr, stream_ptr
from garage_amd.engine import pad_rows, require_gpu

MAX_OBS_DIM = 128  # ga_linear_features_supported


class LinearFeatureBaseline:
    """A linear value function (baseline) on hand-made features.

    Args:
        env_spec: Environment specification (its flat observation width).
        reg_coeff (float): Regularization coefficient.
        name (str): Name of baseline.
    """

    kind = 'linear'  # what VPG / PPO / TRPO ask a value function

    def __init__(self, env_spec, reg_coeff=1e-5, name='LinearFeatureBaseline'):
        self._obs_dim = int(env_spec.observation_space.flat_dim)
        if not 1 <= self._obs_dim <= MAX_OBS_DIM:
            raise ValueError(
                'LinearFeatureBaseline: obs_dim {} is outside 1 .. {} (the '
                'Gram kernel holds at most 2 * 128 + 4 = 260 features)'.format(
                    self._obs_dim, MAX_OBS_DIM))
        self._coeffs = None
        self._reg_coeff = reg_coeff
        self.name = name
        self.lower_bound = -10
        self.upper_bound = 10
        self._reset_device_state()

    def _reset_device_state(self):
        self._coeffs_dev = None  # fp64 device copy of _coeffs, made on demand
        self._pending = None     # (pinned host buffer, event) of a begun fit
        self._scratch = {}       # device: (gram + rhs, workspace, pinned)

    @property
    def n_features(self):
        return 2 * self._obs_dim + 4

    # -- the reference's surface ---------------------------------------------
    def get_param_values(self):
        """float64 coefficients ``[2 * obs_dim + 4]``, or ``None`` before a fit."""
        return self._coeffs

    def set_param_values(self, flattened_params):
        if flattened_params is None:
            self._coeffs = None
        else:
            coeffs = np.array(flattened_params, dtype=np.float64).reshape(-1)
            if coeffs.shape != (self.n_features, ):
                raise ValueError(
                    'LinearFeatureBaseline: {} coefficients for {} '
                    'features'.format(coeffs.size, self.n_features))
            self._coeffs = coeffs
        self._coeffs_dev = None

    def fit(self, paths):
        """Fit on ``paths``: dicts with ``observations`` ``[T, obs_dim]`` and
        ``returns`` ``[T]`` (``linear_feature_baseline.py:61-79``)."""
        obs, ep_off = self._upload_paths(paths)
        returns = torch.from_numpy(np.concatenate(
            [np.asarray(p['returns'], dtype=np.float32).reshape(-1)
             for p in paths])).to(obs.device)
        self._begin(obs, ep_off, len(paths), returns)
        self.finish_fit()

    def predict(self, paths):
        """Values of ONE path (the reference's argument name), float64 ``[T]``;
        zeros before the first fit (``linear_feature_baseline.py:81-93``)."""
        n = len(paths['observations'])
        if self._coeffs is None:
            return np.zeros(n)
        obs, ep_off = self._upload_paths([paths])
        return self._predict(obs, ep_off, 1).view(-1).cpu().numpy().astype(
            np.float64)

    def _upload_paths(self, paths):
        dev = require_gpu()
        lengths = [len(p['observations']) for p in paths]
        if not lengths or min(lengths) < 1:
            raise ValueError('LinearFeatureBaseline: every path needs a step')
        obs = np.concatenate([
            np.asarray(p['observations'], dtype=np.float32).reshape(n, -1)
            for p, n in zip(paths, lengths)])
        if obs.shape[1] != self._obs_dim:
            raise ValueError('LinearFeatureBaseline: observations of width {} '
                             'for obs_dim {}'.format(obs.shape[1],
                                                     self._obs_dim))
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        return pad_rows(obs), torch.from_numpy(off).to(dev)

    # -- the device surface -----------------------------------------------------
    def fit_batch(self, batch, returns):
        """Fit on a :class:`DeviceEpisodeBatch` and its ``[S]`` fp32 device
        returns."""
        self.begin_fit(batch, returns)
        self.finish_fit()

    def begin_fit(self, batch, returns):
        """Enqueue the Gram pass and the copy of its result to pinned host
        memory on the current stream; :meth:`finish_fit` does the rest."""
        self._begin(batch.obs_dev, batch.ep_off_dev, len(batch.lengths),
                    returns)

    def _begin(self, obs, ep_off, n_eps, returns):
        if self._pending is not None:
            raise RuntimeError('LinearFeatureBaseline: begin_fit twice '
                               'without finish_fit')
        S, F = int(obs.shape[0]), self.n_features
        returns = returns.reshape(-1)
        if (returns.dtype != torch.float32 or returns.numel() != S
                or not returns.is_contiguous()):
            raise ValueError('LinearFeatureBaseline: returns must be {} '
                             'contiguous fp32 values'.format(S))
        self._check_batch(obs, ep_off, n_eps)
        out, pinned = self._buffers(obs.device, S)
        call('ga_linear_features_gram_f64', dptr(obs), obs.stride(0),
             self._obs_dim, dptr(ep_off), n_eps, S, dptr(returns),
             dptr(out), out[F * F:].data_ptr(), dptr(self._workspace),
             stream_ptr())
        # ONE asynchronous copy (G and b are neighbours), then the event the
        # host waits for
        pinned.copy_(out, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._pending = (pinned, event, obs.device)

    def finish_fit(self):
        """Wait for the Gram pass, solve on the host as the reference does
        (``linear_feature_baseline.py:70-79``) and upload the coefficients."""
        if self._pending is None:
            raise RuntimeError('LinearFeatureBaseline: finish_fit without '
                               'begin_fit')
        pinned, event, dev = self._pending
        self._pending = None
        event.synchronize()
        F = self.n_features
        host = pinned.numpy()
        gram, rhs = host[:F * F].reshape(F, F), host[F * F:]
        self._solve(gram, rhs)
        self._upload_coeffs(dev)

    def _solve(self, gram, rhs):
        """The reference's solve (``linear_feature_baseline.py:70-79``) of the
        ``F x F`` system into ``_coeffs``; the device copy is not touched."""
        F = self.n_features
        reg_coeff = self._reg_coeff
        for _ in range(5):
            self._coeffs = np.linalg.lstsq(gram + reg_coeff * np.identity(F),
                                           rhs, rcond=-1)[0]
            if not np.any(np.isnan(self._coeffs)):
                break
            reg_coeff *= 10

    def _upload_coeffs(self, device):
        """``_coeffs`` to ``device`` as ``_coeffs_dev``."""
        self._coeffs_dev = torch.from_numpy(
            np.ascontiguousarray(self._coeffs, np.float64)).to(device)

    def cancel_fit(self):
        """Forget a begun fit (its caller failed before :meth:`finish_fit`); the
        coefficients stay what they were."""
        self._pending = None

    def predict_batch(self, batch):
        """``[S, 1]`` fp32 device values of every sample of ``batch``; zeros
        before the first fit."""
        return self._predict(batch.obs_dev, batch.ep_off_dev,
                             len(batch.lengths))

    def _predict(self, obs, ep_off, n_eps):
        S = int(obs.shape[0])
        if self._coeffs is None:
            return torch.zeros(S, 1, dtype=torch.float32, device=obs.device)
        self._check_batch(obs, ep_off, n_eps)
        if self._coeffs_dev is None or self._coeffs_dev.device != obs.device:
            self._upload_coeffs(obs.device)
        values = torch.empty(S, 1, dtype=torch.float32, device=obs.device)
        call('ga_linear_features_predict_f32', dptr(obs), obs.stride(0),
             self._obs_dim, dptr(ep_off), n_eps, S, dptr(self._coeffs_dev),
             dptr(values), 1, stream_ptr())
        return values

    def _check_batch(self, obs, ep_off, n_eps):
        if (obs.dtype != torch.float32 or obs.dim() != 2 or obs.stride(1) != 1
                or obs.shape[1] < self._obs_dim):
            raise ValueError('LinearFeatureBaseline: observations must be '
                             '[S, >= {}] fp32 rows'.format(self._obs_dim))
        if (ep_off.dtype != torch.int64 or ep_off.numel() != n_eps + 1
                or not ep_off.is_contiguous()):
            raise ValueError('LinearFeatureBaseline: ep_off must hold {} '
                             'int64 offsets'.format(n_eps + 1))

    def _buffers(self, device, S):
        """Device ``[F * F + F]`` fp64 for G and b, the Gram pass's workspace for
        ``S`` rows and the pinned host mirror of the former."""
        F = self.n_features
        key = (device.type, device.index)
        if key not in self._scratch:
            out = torch.empty(F * F + F, dtype=torch.float64, device=device)
            pinned = torch.empty(F * F + F, dtype=torch.float64).pin_memory()
            self._scratch[key] = [out, pinned, None]
        entry = self._scratch[key]
        need = int(_lib.load().ga_linear_gram_workspace_doubles(
            self._obs_dim, S))
        if need < 0:
            raise ValueError('LinearFeatureBaseline: {} samples'.format(S))
        if entry[2] is None or entry[2].numel() < need:
            entry[2] = torch.empty(need, dtype=torch.float64, device=device)
        self._workspace = entry[2]
        return entry[0], entry[1]

    # -- pickling: the coefficients travel, device scratch is rebuilt -----------
    def __getstate__(self):
        state = self.__dict__.copy()
        for k in ('_coeffs_dev', '_pending', '_scratch', '_workspace'):
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._reset_device_state()


class _PopulationMember(LinearFeatureBaseline):
    """Member ``index`` of a :class:`LinearFeatureBaselinePopulation`: a
    ``LinearFeatureBaseline`` whose device coefficients are row ``index`` of the
    population's ``(M, F)`` tensor."""

    def __init__(self, population, index, env_spec, reg_coeff, name):
        self._population, self._index = population, index
        super().__init__(env_spec, reg_coeff=reg_coeff, name=name)

    def set_param_values(self, flattened_params):
        super().set_param_values(flattened_params)
        self._population._row_stale(self._index)

    def _upload_coeffs(self, device):
        self._coeffs_dev = self._population._upload_row(self._index, device)


class LinearFeatureBaselinePopulation:
    """``n_members`` :class:`LinearFeatureBaseline` objects fitted and evaluated
    in shared launches (``ga_linear_features_gram_members_f64``,
    ``ga_linear_features_predict_members_f32``): one Gram launch, one reduce
    launch, one copy and one wait for all of them, and one predict launch.
    Every member gets, bit for bit, what it gets fitted alone on its batch.
    There is no reference counterpart: garage fits one baseline per process.

    ``population[m]`` (also ``.members[m]``) is a ``LinearFeatureBaseline`` in
    every respect -- hand it to member ``m``'s ``PPO`` / ``VPG`` as
    ``value_function`` --, whose device coefficients are row ``m`` of one
    ``(M, F)`` fp64 tensor: fitted or set on its own or with the others, the
    member and the row agree.

    Args:
        env_spec: Environment specification (its flat observation width).
        n_members (int): Members, 1 .. 1024.
        reg_coeff (float or sequence): Regularization coefficient, one for all
            members or one per member.
        name (str): Name of the population; member ``m`` is ``name`` +
            ``'/member<m>'``.
    """

    MAX_MEMBERS = 1024  # ga_linear_features_*_members_*

    def __init__(self, env_spec, n_members, reg_coeff=1e-5,
                 name='LinearFeatureBaselinePopulation'):
        n_members = int(n_members)
        if not 1 <= n_members <= self.MAX_MEMBERS:
            raise ValueError(
                'LinearFeatureBaselinePopulation: n_members {} is outside 1 .. '
                '{}'.format(n_members, self.MAX_MEMBERS))
        if np.ndim(reg_coeff) == 0:
            reg_coeffs = [reg_coeff] * n_members
        else:
            reg_coeffs = list(reg_coeff)
            if len(reg_coeffs) != n_members:
                raise ValueError(
                    'LinearFeatureBaselinePopulation: {} reg_coeff values for '
                    '{} members'.format(len(reg_coeffs), n_members))
        self.name = name
        self.members = [
            _PopulationMember(self, m, env_spec, reg_coeffs[m],
                              '{}/member{}'.format(name, m))
            for m in range(n_members)]
        self._obs_dim = self.members[0]._obs_dim
        self._reset_device_state()

    def _reset_device_state(self):
        self._rows = None     # (M, F) fp64 device tensor of the coefficients
        self._fresh = [False] * len(self.members)  # row m holds member m's
        self._pending = None  # (pinned, event, device) of a begun fit
        self._scratch = {}    # device: [out, pinned out, workspace, pinned rows]

    def __len__(self):
        return len(self.members)

    def __getitem__(self, m):
        return self.members[m]

    def __iter__(self):
        return iter(self.members)

    @property
    def n_features(self):
        return 2 * self._obs_dim + 4

    # -- the rows ---------------------------------------------------------------
    def _row_tensor(self, device):
        if self._rows is None or self._rows.device != device:
            self._rows = torch.zeros(len(self.members), self.n_features,
                                     dtype=torch.float64, device=device)
            self._fresh = [False] * len(self.members)
            for member in self.members:
                member._coeffs_dev = None
        return self._rows

    def _row_stale(self, m):
        self._fresh[m] = False

    def _upload_row(self, m, device):
        """Member ``m``'s coefficients into its row; returns the row."""
        row = self._row_tensor(device)[m]
        row.copy_(torch.from_numpy(
            np.ascontiguousarray(self.members[m]._coeffs, np.float64)))
        self._fresh[m] = True
        return row

    @property
    def coeffs_dev(self):
        """The ``(M, F)`` fp64 device tensor (``None`` before anything was
        uploaded); the row of a member without coefficients is meaningless."""
        return self._rows

    def get_param_values(self):
        """The members' coefficients, a list of ``[F]`` float64 arrays (``None``
        for a member before its first fit)."""
        return [member.get_param_values() for member in self.members]

    def set_param_values(self, values):
        """One ``[F]`` array (or ``None``) per member."""
        values = list(values)
        if len(values) != len(self.members):
            raise ValueError(
                'LinearFeatureBaselinePopulation: coefficients of {} members '
                'for {}'.format(len(values), len(self.members)))
        for member, v in zip(self.members, values):
            member.set_param_values(v)

    # -- the joint fit ------------------------------------------------------------
    def _check_count(self, what, items):
        if len(items) != len(self.members):
            raise ValueError(
                'LinearFeatureBaselinePopulation: {} {} for {} members'.format(
                    len(items), what, len(self.members)))

    def fit_batches(self, batches, returns):
        """Fit member ``m`` on ``batches[m]`` and ``returns[m]``."""
        self.begin_fit(batches, returns)
        self.finish_fit()

    def begin_fit(self, batches, returns):
        """Enqueue every member's Gram pass (one Gram launch, one reduce
        launch) and ONE copy of all ``M * (F * F + F)`` doubles to pinned host
        memory on the current stream, then record one event."""
        import ctypes as C
        if self._pending is not None:
            raise RuntimeError('LinearFeatureBaselinePopulation: begin_fit '
                               'twice without finish_fit')
        batches, returns = list(batches), list(returns)
        self._check_count('batches', batches)
        self._check_count('returns', returns)
        M, F = len(self.members), self.n_features
        device = batches[0].obs_dev.device
        flat = []
        for m, (batch, ret) in enumerate(zip(batches, returns)):
            member, S = self.members[m], int(batch.obs_dev.shape[0])
            if member._pending is not None:
                raise RuntimeError(
                    'LinearFeatureBaselinePopulation: member {} has a fit of '
                    'its own begun'.format(m))
            ret = ret.reshape(-1)
            if (ret.dtype != torch.float32 or ret.numel() != S
                    or not ret.is_contiguous() or ret.device != device):
                raise ValueError(
                    'LinearFeatureBaselinePopulation: member {}: returns must '
                    'be {} contiguous fp32 values on {}'.format(m, S, device))
            member._check_batch(batch.obs_dev, batch.ep_off_dev,
                                len(batch.lengths))
            if batch.obs_dev.device != device:
                raise ValueError('LinearFeatureBaselinePopulation: member {}: '
                                 'a batch on another device'.format(m))
            flat.append(ret)
        out, pinned, workspace = self._fit_buffers(
            device, [int(b.obs_dev.shape[0]) for b in batches])
        arr = (_lib.LinearGramMember * M)()
        for m, (batch, ret) in enumerate(zip(batches, flat)):
            u, base = arr[m], out[m * (F * F + F):]
            u.obs, u.ldo = batch.obs_dev.data_ptr(), batch.obs_dev.stride(0)
            u.ep_off, u.n_eps = batch.ep_off_dev.data_ptr(), len(batch.lengths)
            u.S, u.returns = int(batch.obs_dev.shape[0]), ret.data_ptr()
            u.gram, u.rhs = base.data_ptr(), base[F * F:].data_ptr()
        call('ga_linear_features_gram_members_f64', arr, M, self._obs_dim,
             dptr(workspace), workspace.numel(), stream_ptr())
        pinned.copy_(out, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._pending = (pinned, event, device)

    def finish_fit(self):
        """Wait once, solve every member's system on the host exactly as
        :meth:`LinearFeatureBaseline.finish_fit` does (the member's own
        ``reg_coeff``, the reference's retries) and upload all coefficients in
        one copy."""
        if self._pending is None:
            raise RuntimeError('LinearFeatureBaselinePopulation: finish_fit '
                               'without begin_fit')
        pinned, event, device = self._pending
        self._pending = None
        event.synchronize()
        M, F = len(self.members), self.n_features
        host = pinned.numpy().reshape(M, F * F + F)
        rows_host = self._scratch[(device.type, device.index)][3]
        stage = rows_host.numpy()
        for m, member in enumerate(self.members):
            member._solve(host[m, :F * F].reshape(F, F), host[m, F * F:])
            stage[m] = member._coeffs
        rows = self._row_tensor(device)
        rows.copy_(rows_host, non_blocking=True)
        # (the pinned rows are rewritten by the next finish_fit only, which
        # waits for an event recorded behind this copy)
        for m, member in enumerate(self.members):
            member._coeffs_dev = rows[m]
            self._fresh[m] = True

    def cancel_fit(self):
        """Forget a begun fit; the coefficients stay what they were."""
        self._pending = None

    def predict_batches(self, batches):
        """One ``[S_m, 1]`` fp32 device tensor per member, one launch; zeros
        for a member that has no coefficients yet."""
        batches = list(batches)
        self._check_count('batches', batches)
        M = len(self.members)
        device = batches[0].obs_dev.device
        rows = self._row_tensor(device)
        sizes = [int(b.obs_dev.shape[0]) for b in batches]
        # every member's values in one allocation, each from a 256-byte boundary
        starts = np.concatenate([[0], np.cumsum([(S + 63) // 64 * 64
                                                 for S in sizes])])
        store = torch.empty(int(starts[-1]), 1, dtype=torch.float32,
                            device=device)
        arr = (_lib.LinearPredictMember * M)()
        values = []
        for m, (member, batch) in enumerate(zip(self.members, batches)):
            member._check_batch(batch.obs_dev, batch.ep_off_dev,
                                len(batch.lengths))
            if batch.obs_dev.device != device:
                raise ValueError('LinearFeatureBaselinePopulation: member {}: '
                                 'a batch on another device'.format(m))
            if member._coeffs is not None and not self._fresh[m]:
                member._upload_coeffs(device)
            v = store[int(starts[m]):int(starts[m]) + sizes[m]]
            u = arr[m]
            u.obs, u.ldo = batch.obs_dev.data_ptr(), batch.obs_dev.stride(0)
            u.ep_off, u.n_eps = batch.ep_off_dev.data_ptr(), len(batch.lengths)
            u.S = sizes[m]
            u.coeffs = None if member._coeffs is None else rows[m].data_ptr()
            u.values, u.ldv = v.data_ptr(), 1
            values.append(v)
        call('ga_linear_features_predict_members_f32', arr, M, self._obs_dim,
             stream_ptr())
        return values

    def _fit_buffers(self, device, sizes):
        """Device ``[M * (F * F + F)]`` fp64 for every member's G and b, its
        pinned mirror, the joint Gram pass's workspace for members of ``sizes``
        rows (and, for :meth:`finish_fit`, pinned ``(M, F)`` coefficients)."""
        import ctypes as C
        M, F = len(self.members), self.n_features
        key = (device.type, device.index)
        if key not in self._scratch:
            n = M * (F * F + F)
            self._scratch[key] = [
                torch.empty(n, dtype=torch.float64, device=device),
                torch.empty(n, dtype=torch.float64).pin_memory(), None,
                torch.empty(M, F, dtype=torch.float64).pin_memory()]
        entry = self._scratch[key]
        need = int(_lib.load().ga_linear_gram_members_workspace_doubles(
            self._obs_dim, M, (C.c_int64 * M)(*sizes)))
        if need < 0:
            raise ValueError('LinearFeatureBaselinePopulation: members of {} '
                             'samples'.format(sizes))
        if entry[2] is None or entry[2].numel() < need:
            entry[2] = torch.empty(need, dtype=torch.float64, device=device)
        return entry[0], entry[1], entry[2]

    # -- pickling: the members (coefficients, reg_coeff) travel, device state is
    # rebuilt
    def __getstate__(self):
        state = self.__dict__.copy()
        for k in ('_rows', '_fresh', '_pending', '_scratch'):
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._reset_device_state()


__all__ = ['LinearFeatureBaseline', 'LinearFeatureBaselinePopulation']
