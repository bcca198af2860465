"""The linear baselines' device solver: ``ga_linear_solve_members_f64`` against the
backward-error bound of a Cholesky solve (Higham, Accuracy and Stability, theorem
10.4: normwise ``|b - A x| / (|A| |x| + |b|) <= F (3 F + 1) 2^-53`` whatever the
order of the sums), its retries exactly, and the whole fit through the classes with
``solver='device'`` at the bar ``test_linear_baseline_gpu.py`` holds the host to."""
import pickle

import numpy as np
import pytest
import torch

import _linear_baseline_cases as lc
from test_linear_baseline_gpu import EPS32, Case

pytestmark = pytest.mark.gpu

GUARD = 64


def _system(obs_dim, n_rows, seed):
    """``(G, b)`` of ``n_rows`` feature rows, G exactly symmetric."""
    rng = np.random.RandomState(seed)
    phi = lc.features(rng.uniform(-3, 3, (n_rows, obs_dim)), [n_rows])
    G = phi.T.dot(phi)
    return (G + G.T) / 2, phi.T.dot(30.0 * rng.standard_normal(n_rows))


def _solve(obs_dim, systems, regs):
    """``(coeffs [M, F], status [M])`` of one launch; G, b and the guard words
    around the coefficients and behind the workspace must come back untouched."""
    from garage_amd import _lib
    dev = torch.device('cuda:0')
    M, F = len(systems), 2 * obs_dim + 4
    grams = [torch.from_numpy(G).to(dev) for G, _ in systems]
    rhs = [torch.from_numpy(b).to(dev) for _, b in systems]
    out = torch.full((M, F + 2 * GUARD), -777.0, dtype=torch.float64, device=dev)
    status = torch.full((M, ), 99, dtype=torch.int32, device=dev)
    need = _lib.load().ga_linear_solve_workspace_doubles(obs_dim, M)
    ws = torch.full((need + GUARD, ), -777.0, dtype=torch.float64, device=dev)
    arr = (_lib.LinearSolveMember * M)()
    for m, u in enumerate(arr):
        u.gram, u.rhs, u.reg_coeff = grams[m].data_ptr(), rhs[m].data_ptr(), regs[m]
        u.coeffs, u.status = out[m, GUARD:].data_ptr(), status[m:].data_ptr()
    _lib.call('ga_linear_solve_members_f64', arr, M, obs_dim, _lib.dptr(ws), need,
              _lib.stream_ptr())
    got = out.cpu().numpy()
    assert (got[:, :GUARD] == -777.0).all() and (got[:, GUARD + F:] == -777.0).all()
    assert bool((ws[need:] == -777.0).all())
    for (G, b), g, r in zip(systems, grams, rhs):
        assert np.array_equal(g.cpu().numpy(), G) and np.array_equal(r.cpu().numpy(), b)
    return got[:, GUARD:GUARD + F], status.cpu().numpy()


# F = 6, 16, 18, 32, 128, 260: below a tile, 1, 1 and a ragged one, 2, 8, 16 and a ragged
@pytest.mark.parametrize('n_members', [1, 3])
@pytest.mark.parametrize('obs_dim', [1, 6, 7, 14, 62, 128])
def test_solve_meets_the_cholesky_backward_error_bound(obs_dim, n_members):
    F = 2 * obs_dim + 4
    # (the second member: 9 rows, at F > 9 only the regulariser keeps it definite)
    rows, regs = [2 * F + 5, 9, F][:n_members], [1e-5, 1e-3, 1e-1][:n_members]
    systems = [_system(obs_dim, n, 10 * obs_dim + m) for m, n in enumerate(rows)]
    coeffs, status = _solve(obs_dim, systems, regs)
    assert (status == 0).all()
    bound = F * (3 * F + 1) * 2.0 ** -53
    for (G, b), reg, x in zip(systems, regs, coeffs):
        A = G + reg * np.identity(F)
        err = np.linalg.norm(b - A.dot(x)) / (
            np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))
        print('F', F, 'reg', reg, 'backward error', err, 'bound', bound)
        assert np.isfinite(x).all() and err <= bound


@pytest.mark.parametrize('obs_dim', [1, 7])
def test_retries_are_the_references(obs_dim):
    F = 2 * obs_dim + 4
    ones, eye = np.ones(F), np.identity(F)
    reg3 = 1e-5
    for _ in range(3):
        reg3 *= 10
    coeffs, status = _solve(obs_dim, [(-0.005 * eye, ones)], [1e-5])
    want = 1.0 / (-0.005 + reg3)  # 1e-5, 1e-4 and 1e-3 break down, 1e-2 does not
    assert status[0] == 3
    assert (np.abs(coeffs[0] - want) <= 4 * np.spacing(want)).all()
    healthy = _system(obs_dim, 2 * F, 3)
    alone, _ = _solve(obs_dim, [healthy], [1e-5])
    coeffs, status = _solve(obs_dim, [(-eye, ones), healthy, (-0.005 * eye, ones)],
                            [1e-5, 1e-5, 1e-5])
    assert list(status) == [-1, 0, 3]
    assert np.isnan(coeffs[0]).all()
    assert np.array_equal(coeffs[1], alone[0])  # bit for bit what it gets alone
    assert (np.abs(coeffs[2] - want) <= 4 * np.spacing(want)).all()


FIT_CASES = ['smallest', 'stride4', 'tile_edge', 'limit', 'slab_plus']
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _check_fit(c, b, row):
    """Fitted ``b`` of case ``c`` whose device coefficients are ``row``."""
    v = b.predict_batch(c.batch).view(-1).cpu().numpy().astype(np.float64)
    bound = c.fit_bound + EPS32 * np.maximum(np.abs(c.pred), 1.0)
    assert (np.abs(v - c.pred) <= bound).all()
    coeffs = b.get_param_values()
    assert coeffs.dtype == np.float64 and b.solve_status == 0
    assert np.array_equal(coeffs, row.cpu().numpy())
    assert np.abs(c.phi.dot(coeffs) - c.pred).max() <= c.fit_bound
    again = pickle.loads(pickle.dumps(b))
    assert np.array_equal(again.get_param_values(), coeffs)


def _fit_alone(name):
    from garage_amd.baselines import LinearFeatureBaseline
    c = _case(name)
    b = LinearFeatureBaseline(c.spec, reg_coeff=lc.REG_COEFF, solver='device')
    assert not bool(b.predict_batch(c.batch).any())
    b.fit_batch(c.batch, c.returns_dev)
    assert b._coeffs is None and b._has_coeffs()  # nothing fetched, nothing waited for
    return c, b


@pytest.mark.parametrize('name', FIT_CASES)
def test_whole_fit_on_the_device_matches_the_twin(name):
    c, b = _fit_alone(name)
    _check_fit(c, b, b._coeffs_dev)


@pytest.mark.parametrize('names', [['slab_plus', 'slab_minus', 'slab_exact']])
def test_population_fit_on_the_device_is_the_lone_fit(names):
    from garage_amd.baselines import LinearFeatureBaselinePopulation
    cases = [_case(n) for n in names]  # (one obs_dim, three different batches)
    pop = LinearFeatureBaselinePopulation(cases[0].spec, 3, reg_coeff=lc.REG_COEFF,
                                          solver='device')
    pop.fit_batches([c.batch for c in cases], [c.returns_dev for c in cases])
    assert all(b._coeffs is None and b._has_coeffs() for b in pop)
    values = pop.predict_batches([c.batch for c in cases])
    for m, (c, name) in enumerate(zip(cases, names)):
        _, alone = _fit_alone(name)
        assert torch.equal(pop.coeffs_dev[m], alone._coeffs_dev)
        assert torch.equal(values[m], alone.predict_batch(c.batch))
        _check_fit(c, pop[m], pop.coeffs_dev[m])
