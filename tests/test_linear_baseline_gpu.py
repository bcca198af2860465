"""The linear feature baseline on the device against the fp64 numpy twin of
``_linear_baseline_cases.py`` (which ``test_linear_baseline_cpu.py`` holds to the
real reference class): the Gram pass and the predict pass through the C ABI, the
whole fit and both surfaces through ``garage_amd.baselines.LinearFeatureBaseline``.

Bounds.  Gram: two fp64 sums of the same S products in different orders differ
by at most S * 2^-52 * sum |products|, entry by entry.  Predict: one fp32
rounding of an fp64 sum, with a factor two: 2^-23 * max(|v|, 1).  Whole fit: the
twin's own predictions move by ``SPREAD`` when its rows are permuted; the device
is allowed 100 times that (a margin over the reference's order sensitivity, not
a measurement of the device), at least 1e-9 * max |v|.
"""
import pickle

import numpy as np
import pytest
import torch

import _linear_baseline_cases as lc

pytestmark = pytest.mark.gpu

EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
GUARD = 64


class Case:
    """A case's inputs on the device and the twin's answers, built once."""

    def __init__(self, name):
        from garage_amd._dtypes import Box, DeviceEpisodeBatch, EnvSpec
        dev = torch.device('cuda:0')
        _, self.obs_dim, lengths, ld_extra = lc.case(name)
        self.name = name
        self.obs, self.returns, self.lengths = lc.make_inputs(name)
        self.S, self.F = len(self.returns), 2 * self.obs_dim + 4
        self.phi = lc.features(self.obs, lengths)
        self.coeffs = lc.fit(self.phi, self.returns)
        self.pred = self.phi.dot(self.coeffs)
        self.off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        ldo = lc.round4(self.obs_dim) + ld_extra
        # NaN in a wider stride's padding: whoever reads it cannot pass
        padded = np.full((self.S, ldo), np.nan if ld_extra else 0.0, np.float32)
        padded[:, :self.obs_dim] = self.obs
        self.obs_dev = torch.from_numpy(padded).to(dev)
        self.off_dev = torch.from_numpy(self.off).to(dev)
        self.returns_dev = torch.from_numpy(self.returns).to(dev)
        self.spec = EnvSpec(Box(-np.inf, np.inf, (self.obs_dim, )),
                            Box(-np.inf, np.inf, (1, )),
                            max_episode_length=max(lengths))
        n = len(lengths)
        self.batch = DeviceEpisodeBatch(
            self.spec, lengths=lengths, obs_dev=self.obs_dev,
            last_obs_dev=torch.zeros(n, ldo, device=dev),
            actions_dev=torch.zeros(self.S, 4, device=dev),
            rewards_dev=torch.zeros(self.S, device=dev),
            step_types_dev=torch.zeros(self.S, dtype=torch.uint8, device=dev),
            ep_off_dev=self.off_dev)
        self.fit_bound = max(100 * lc.SPREAD[name],
                             1e-9 * np.abs(self.pred).max())


_CASES = {}


@pytest.fixture
def case(request):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


all_cases = pytest.mark.parametrize('case', lc.CASE_NAMES, indirect=True)


def _gram(c):
    """(G, b, workspace with its guard words) of one call through the C ABI."""
    from garage_amd import _lib
    dev = c.obs_dev.device
    need = _lib.load().ga_linear_gram_workspace_doubles(c.obs_dim, c.S)
    assert need > 0
    ws = torch.full((need + GUARD, ), float('nan'), dtype=torch.float64,
                    device=dev)
    ws[need:] = -777.0
    gram = torch.full((c.F, c.F), float('nan'), dtype=torch.float64, device=dev)
    rhs = torch.full((c.F, ), float('nan'), dtype=torch.float64, device=dev)
    _lib.call('ga_linear_features_gram_f64', _lib.dptr(c.obs_dev),
              c.obs_dev.stride(0), c.obs_dim, _lib.dptr(c.off_dev),
              len(c.lengths), c.S, _lib.dptr(c.returns_dev), _lib.dptr(gram),
              _lib.dptr(rhs), _lib.dptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    return gram, rhs, ws, need


@all_cases
def test_gram_matches_the_twin(case):
    c = case
    gram, rhs, ws, need = _gram(c)
    # the workspace: all of what the library reports, nothing beyond
    assert bool((ws[need:] == -777.0).all())
    assert not bool(torch.isnan(ws[:need]).any())
    G, b = gram.cpu().numpy(), rhs.cpu().numpy()
    r = c.returns.astype(np.float64)
    want_G, want_b = c.phi.T.dot(c.phi), c.phi.T.dot(r)
    bound_G = c.S * EPS64 * np.abs(c.phi).T.dot(np.abs(c.phi))
    bound_b = c.S * EPS64 * np.abs(c.phi).T.dot(np.abs(r))
    err_G, err_b = np.abs(G - want_G), np.abs(b - want_b)
    print(c.name, 'G worst error / bound',
          np.max(err_G / np.maximum(bound_G, 1e-300)),
          'b', np.max(err_b / np.maximum(bound_b, 1e-300)))
    assert not np.isnan(G).any() and not np.isnan(b).any()
    assert (err_G <= bound_G).all()
    assert (err_b <= bound_b).all()
    assert np.array_equal(G, G.T)  # exactly symmetric
    # a second call: the same bits
    gram2, rhs2, _, _ = _gram(c)
    assert torch.equal(gram, gram2) and torch.equal(rhs, rhs2)


@all_cases
def test_predict_matches_the_twin(case):
    from garage_amd import _lib
    c = case
    dev = c.obs_dev.device
    coeffs = torch.from_numpy(c.coeffs).to(dev)
    ldv = 3  # a strided output: the neighbours stay untouched
    values = torch.full((c.S, ldv), -5.0, dtype=torch.float32, device=dev)
    _lib.call('ga_linear_features_predict_f32', _lib.dptr(c.obs_dev),
              c.obs_dev.stride(0), c.obs_dim, _lib.dptr(c.off_dev),
              len(c.lengths), c.S, _lib.dptr(coeffs), _lib.dptr(values), ldv,
              _lib.stream_ptr())
    got = values.cpu().numpy().astype(np.float64)
    assert (got[:, 1:] == -5.0).all()
    v = got[:, 0]
    bound = EPS32 * np.maximum(np.abs(c.pred), 1.0)
    print(c.name, 'worst error / bound', np.max(np.abs(v - c.pred) / bound))
    assert (np.abs(v - c.pred) <= bound).all()
    # the first and the last row of every episode, and the batch's last row
    for e in range(len(c.lengths)):
        for row in (c.off[e], c.off[e + 1] - 1):
            assert abs(v[row] - c.pred[row]) <= bound[row], (e, row)
    assert abs(v[-1] - c.pred[-1]) <= bound[-1]


@all_cases
def test_whole_fit_matches_the_twin(case):
    from garage_amd.baselines import LinearFeatureBaseline
    c = case
    b = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF)
    before = b.predict_batch(c.batch)
    assert before.shape == (c.S, 1) and before.dtype == torch.float32
    assert not bool(before.any())
    b.fit_batch(c.batch, c.returns_dev)
    coeffs = b.get_param_values()
    assert coeffs.dtype == np.float64 and coeffs.shape == (c.F, )
    moved = np.abs(c.phi.dot(coeffs) - c.pred).max()
    print(c.name, 'fp64 predictions moved by', moved, 'bound', c.fit_bound)
    assert moved <= c.fit_bound
    v = b.predict_batch(c.batch)
    assert v.shape == (c.S, 1) and v.dtype == torch.float32
    v = v.view(-1).cpu().numpy().astype(np.float64)
    bound = c.fit_bound + EPS32 * np.maximum(np.abs(c.pred), 1.0)
    assert (np.abs(v - c.pred) <= bound).all()


@pytest.mark.parametrize('case', ['stride4', 'equal_then_ragged'],
                         indirect=True)
def test_reference_surface_is_the_batch_surface(case):
    from garage_amd.baselines import LinearFeatureBaseline
    c = case
    on_batch = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF)
    on_batch.fit_batch(c.batch, c.returns_dev)
    want = on_batch.predict_batch(c.batch).view(-1).cpu().numpy()
    paths = lc.paths_of(c.obs, c.returns, c.lengths)
    b = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF)
    zeros = b.predict(paths[0])
    assert zeros.shape == (c.lengths[0], ) and not zeros.any()
    b.fit(paths)
    assert np.array_equal(b.get_param_values(), on_batch.get_param_values())
    for e, path in enumerate(paths):
        got = b.predict(path)
        assert got.dtype == np.float64 and got.shape == (c.lengths[e], )
        assert np.array_equal(got, want[c.off[e]:c.off[e + 1]].astype(
            np.float64)), e
    # set_param_values: the twin's coefficients give the twin's predictions
    b.set_param_values(c.coeffs)
    assert np.array_equal(b.get_param_values(), c.coeffs)
    v = b.predict_batch(c.batch).view(-1).cpu().numpy().astype(np.float64)
    assert (np.abs(v - c.pred) <= EPS32 * np.maximum(np.abs(c.pred),
                                                      1.0)).all()
    # pickle: the coefficients travel, the device state is rebuilt
    again = pickle.loads(pickle.dumps(on_batch))
    assert np.array_equal(again.get_param_values(),
                          on_batch.get_param_values())
    assert np.array_equal(
        again.predict_batch(c.batch).view(-1).cpu().numpy(), want)
    b.set_param_values(None)
    assert not bool(b.predict_batch(c.batch).any())


@pytest.mark.parametrize('case', ['tile_edge'], indirect=True)
def test_begin_and_finish_are_the_two_halves(case):
    from garage_amd.baselines import LinearFeatureBaseline
    c = case
    whole = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF)
    whole.fit_batch(c.batch, c.returns_dev)
    b = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF)
    with pytest.raises(RuntimeError):
        b.finish_fit()
    b.begin_fit(c.batch, c.returns_dev)
    assert b.get_param_values() is None  # nothing solved yet
    other = torch.ones(1024, device=c.obs_dev.device).sum()  # work in between
    with pytest.raises(RuntimeError):
        b.begin_fit(c.batch, c.returns_dev)
    b.finish_fit()
    assert float(other) == 1024.0
    assert np.array_equal(b.get_param_values(), whole.get_param_values())


def test_obs_dim_129_raises():
    from garage_amd._dtypes import Box, EnvSpec
    from garage_amd.baselines import LinearFeatureBaseline
    spec = EnvSpec(Box(-np.inf, np.inf, (129, )), Box(-np.inf, np.inf, (1, )),
                   max_episode_length=5)
    with pytest.raises(ValueError) as e:
        LinearFeatureBaseline(spec)
    assert '129' in str(e.value)
