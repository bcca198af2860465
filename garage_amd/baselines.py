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
        reg_coeff = self._reg_coeff
        for _ in range(5):
            self._coeffs = np.linalg.lstsq(gram + reg_coeff * np.identity(F),
                                           rhs, rcond=-1)[0]
            if not np.any(np.isnan(self._coeffs)):
                break
            reg_coeff *= 10
        self._coeffs_dev = torch.from_numpy(self._coeffs).to(dev)

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
            self._coeffs_dev = torch.from_numpy(
                np.ascontiguousarray(self._coeffs, np.float64)).to(obs.device)
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
