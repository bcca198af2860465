"""``ga_policy_head_sample`` -- the per-layer path's action head -- called directly
through ``garage_amd._lib``: what it writes to ``action`` / ``act_buf`` /
``head_buf`` / ``obs_buf`` and what it leaves alone.

Shapes: 300 envs (two workgroups, the second partial), observations of 5 columns in
rows of 8, a rollout buffer of 4 columns written at column 2; every output buffer
starts filled with a sentinel.  The Gaussian cases use means that are multiples of
1/16 in [-2, 2], noise that is a multiple of 1/8 in [-4, 4] and a standard deviation
of exactly 1 (``expf(0)``), so ``mean + std * noise`` is exact in fp32 with or
without a fused multiply-add and the comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, OBS, LDO, TCAP, COL = 300, 5, 8, 4, 2
SENTINEL = -777.25


def _head_sample(kind, A, head, lda, ldh, noise=None, log_std=0.0, has_min=0,
                 min_log_std=0.0, double_softmax=0, seed=0, step=0, env_id0=0,
                 with_head_buf=True):
    """One call; returns the observations given and the four output buffers."""
    from garage_amd import _lib
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)
    obs = rng.uniform(-1, 1, (N, LDO)).astype(np.float32)
    t_obs = torch.from_numpy(obs).to(dev)
    t_head = torch.from_numpy(np.ascontiguousarray(head, np.float32)).to(dev)
    t_log_std = torch.tensor([log_std], dtype=torch.float32, device=dev)
    t_noise = None if noise is None else torch.from_numpy(
        np.ascontiguousarray(noise, np.float32)).to(dev)
    out = {
        'action': torch.full((N, lda), SENTINEL, device=dev),
        'obs_buf': torch.full((N, TCAP, LDO), SENTINEL, device=dev),
        'act_buf': torch.full((N, TCAP, lda), SENTINEL, device=dev),
        'head_buf': torch.full((N, TCAP, ldh), SENTINEL, device=dev),
    }
    a = _lib.HeadArgs()
    a.n, a.env_id0, a.A, a.kind = N, env_id0, A, kind
    a.head, a.ldh = t_head.data_ptr(), t_head.stride(0)
    assert t_head.stride(0) == ldh
    a.log_std = t_log_std.data_ptr()
    a.has_min, a.has_max, a.min_log_std, a.max_log_std = has_min, 0, min_log_std, 0.0
    if t_noise is not None:
        a.noise, a.ldn = t_noise.data_ptr(), t_noise.stride(0)
    a.seed, a.step, a.double_softmax = seed, step, double_softmax
    a.obs, a.ldo, a.obs_dim = t_obs.data_ptr(), LDO, OBS
    a.col, a.Tcap = COL, TCAP
    a.action, a.lda = out['action'].data_ptr(), lda
    a.obs_buf, a.act_buf = out['obs_buf'].data_ptr(), out['act_buf'].data_ptr()
    a.head_buf = out['head_buf'].data_ptr() if with_head_buf else None
    _lib.call('ga_policy_head_sample', C.byref(a), _lib.stream_ptr())
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['obs'] = obs
    return res


def _only_written(res, width, head_width):
    """The observation rows went to column COL; outside the first ``width`` columns
    of ``action`` / ``act_buf[:, COL]``, the first ``head_width`` of
    ``head_buf[:, COL]`` and the first OBS of ``obs_buf[:, COL]`` every buffer still
    holds the sentinel."""
    assert np.array_equal(res['obs_buf'][:, COL, :OBS], res['obs'][:, :OBS])
    assert (res['action'][:, width:] == SENTINEL).all()
    for name, w in (('obs_buf', OBS), ('act_buf', width), ('head_buf', head_width)):
        buf = res[name]
        other = [c for c in range(TCAP) if c != COL]
        assert (buf[:, other] == SENTINEL).all(), name
        assert (buf[:, COL, w:] == SENTINEL).all(), name


def _gaussian_inputs():
    rng = np.random.default_rng(3)
    A, ld = 6, 8
    mu = np.full((N, ld), 123.0, np.float32)  # (padding columns are never read)
    mu[:, :A] = rng.integers(-32, 33, (N, A)) / 16.0
    z = np.full((N, ld), 321.0, np.float32)
    z[:, :A] = rng.integers(-32, 33, (N, A)) / 8.0
    return A, ld, mu, z


@pytest.mark.parametrize('log_std,has_min', [(0.0, 0), (-3.0, 1)])
def test_gaussian_teacher_forced_is_exact(log_std, has_min):
    """std = expf(0) = 1, directly or through the min_log_std = 0 clamp of
    log_std = -3: action = mean + noise bit for bit, and the same call without
    head_buf writes the same action / act_buf / obs_buf."""
    A, ld, mu, z = _gaussian_inputs()
    want = mu[:, :A] + z[:, :A]
    kw = dict(noise=z, log_std=log_std, has_min=has_min, min_log_std=0.0)
    res = _head_sample(0, A, mu, ld, ld, **kw)
    assert np.array_equal(res['action'][:, :A], want)
    assert np.array_equal(res['act_buf'][:, COL, :A], want)
    assert np.array_equal(res['head_buf'][:, COL, :A], mu[:, :A])
    _only_written(res, A, A)
    bare = _head_sample(0, A, mu, ld, ld, with_head_buf=False, **kw)
    for name in ('action', 'act_buf', 'obs_buf'):
        assert np.array_equal(bare[name], res[name]), name
    assert (bare['head_buf'] == SENTINEL).all()


def test_gaussian_device_noise_is_the_oracle_stream():
    """noise = NULL: action - mean is the action stream of env_id0 + i at `step`
    (oracle.envs.action_noise), to the 1e-5 tests/test_configs_gpu.py compares the
    actions of a rollout with (the device's own logf / sincosf)."""
    from oracle import envs as oenvs
    A, ld, mu, _ = _gaussian_inputs()
    seed, step, env_id0 = 0x1234567887654321, 41, 7
    res = _head_sample(0, A, mu, ld, ld, seed=seed, step=step, env_id0=env_id0)
    z = oenvs.action_noise(seed, env_id0 + np.arange(N), step, A)
    got = res['action'][:, :A] - mu[:, :A]
    print('max |z - oracle|', np.abs(got - z).max())
    assert np.allclose(got, z, atol=1e-5, rtol=0)
    assert np.array_equal(res['act_buf'][:, COL, :A], res['action'][:, :A])
    assert np.array_equal(res['head_buf'][:, COL, :A], mu[:, :A])
    _only_written(res, A, A)


@pytest.mark.parametrize('double_softmax', [0, 1])
def test_categorical_teacher_forced_picks_every_class(double_softmax):
    """u = the midpoint of class (row % 5)'s interval of the fp64 (double-)softmax
    CDF: every interval is wider than 2e-3, so the midpoint is 1e-3 from both ends
    and the fp32 inverse CDF must pick that class, for all 300 rows; head_buf holds
    the probabilities."""
    A, lda, ldh, ldn = 5, 4, 8, 4
    rng = np.random.default_rng(17)
    sc = np.full((N, ldh), 55.0, np.float32)
    sc[:, :A] = rng.uniform(-1, 1, (N, A))

    def softmax(x):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    probs = softmax(sc[:, :A].astype(np.float64))
    if double_softmax:
        probs = softmax(probs)
    assert probs.min() > 2e-3  # the condition the exact comparison rests on
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(probs, axis=1)], axis=1)
    cls = np.arange(N) % A
    u = np.full((N, ldn), 0.999, np.float32)
    u[:, 0] = 0.5 * (cdf[np.arange(N), cls] + cdf[np.arange(N), cls + 1])
    res = _head_sample(1, A, sc, lda, ldh, noise=u, double_softmax=double_softmax)
    assert np.array_equal(res['action'][:, 0], cls.astype(np.float32))
    assert np.array_equal(res['act_buf'][:, COL, 0], cls.astype(np.float32))
    print('max |probs - fp64|', np.abs(res['head_buf'][:, COL, :A] - probs).max())
    assert np.allclose(res['head_buf'][:, COL, :A], probs, atol=1e-6, rtol=0)
    _only_written(res, 1, A)
