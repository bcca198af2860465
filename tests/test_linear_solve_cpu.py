"""The linear baselines' device solver without a device: the C record and entries in
the header, ``_lib`` and the library; the workspace rule; every refusal before
anything is read; the ``solver`` keyword of the two classes."""
import ctypes as C
import math
import os
import pickle

import numpy as np
import pytest

from garage_amd import _lib
from garage_amd._dtypes import Box, EnvSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = EnvSpec(Box(-1, 1, (4, )), Box(-1, 1, (2, )), max_episode_length=8)
F = 2 * 4 + 4
BASE = 0x100000  # never read: every call that takes it is refused first


def test_record_and_entries_mirror_the_header():
    rec = _lib.LinearSolveMember
    assert [f[0] for f in rec._fields_] == ['gram', 'rhs', 'reg_coeff',
                                            'coeffs', 'status']
    assert C.sizeof(rec) == 40
    assert [getattr(rec, n).offset for n, _ in rec._fields_] == [0, 8, 16, 24, 32]
    header = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    lib = _lib.load()
    for decl in ('GA_API int64_t ga_linear_solve_workspace_doubles(',
                 'GA_API int ga_linear_solve_members_f64('):
        name = decl.split()[-1][:-1]
        assert decl in header
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert '} ga_linear_solve_member;' in header


def test_workspace_doubles_on_both_sides_of_the_limits():
    ws = _lib.load().ga_linear_solve_workspace_doubles
    tiles = lambda obs_dim: (2 * obs_dim + 4 + 15) // 16
    tri = lambda T: 256 * T * (T + 1) // 2  # the factor's triangle of tiles
    assert ws(1, 1) == tri(1) == 256
    assert ws(6, 3) == 3 * tri(1) and ws(7, 1) == tri(2)
    assert ws(128, 1) == tri(tiles(128)) == 256 * 153
    assert ws(128, 1024) == 1024 * 256 * 153
    assert ws(129, 1) == -1 and ws(0, 1) == -1
    assert ws(128, 1025) == -1 and ws(4, 0) == -1


def _member(**kw):
    arr = (_lib.LinearSolveMember * 2)()
    for u in arr:
        u.gram, u.rhs, u.reg_coeff, u.coeffs, u.status = (BASE, BASE, 1e-5,
                                                          BASE, BASE)
    for k, v in kw.items():
        setattr(arr[1], k, v)
    return arr


@pytest.mark.parametrize('arr, n, obs_dim, ws, doubles, message', [
    (None, 2, 4, BASE, 1 << 20, 'null pointer'),
    (_member(), 2, 4, None, 1 << 20, 'null pointer'),
    (_member(status=None), 2, 4, BASE, 1 << 20, 'member 1: null pointer'),
    (_member(), 0, 4, BASE, 1 << 20, 'n_members'),
    (_member(), 1025, 4, BASE, 1 << 20, 'n_members'),
    (_member(), 2, 0, BASE, 1 << 20, 'obs_dim'),
    (_member(), 2, 129, BASE, 1 << 20, 'obs_dim'),
    (_member(), 2, 4, BASE + 4, 1 << 20, 'aligned'),
    (_member(rhs=BASE + 4), 2, 4, BASE, 1 << 20, 'member 1: gram, rhs'),
    (_member(reg_coeff=-1e-9), 2, 4, BASE, 1 << 20, 'member 1: reg_coeff'),
    (_member(reg_coeff=math.nan), 2, 4, BASE, 1 << 20, 'member 1: reg_coeff'),
    (_member(), 2, 4, BASE, 2 * 256 - 1, 'workspace too small'),
])
def test_entry_refuses_before_anything_is_read(arr, n, obs_dim, ws, doubles,
                                               message):
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_linear_solve_members_f64', arr, n, obs_dim, ws, doubles,
                  None)
    assert message in str(e.value)


def test_solver_keyword():
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    for make in (lambda **kw: LinearFeatureBaseline(SPEC, **kw),
                 lambda **kw: LinearFeatureBaselinePopulation(SPEC, 2, **kw)):
        with pytest.raises(ValueError) as e:
            make(solver='bogus')
        assert 'bogus' in str(e.value)
        assert make()._solver == 'host' and make(solver='device')
    pop = LinearFeatureBaselinePopulation(SPEC, 2, solver='device')
    assert [b._solver for b in pop] == ['device', 'device']


@pytest.mark.parametrize('solver', ['host', 'device'])
def test_objects_pickle_and_behave_as_before(solver):
    from garage_amd.baselines import (LinearFeatureBaseline,
                                      LinearFeatureBaselinePopulation)
    b = LinearFeatureBaseline(SPEC, reg_coeff=0.5, solver=solver)
    assert b.get_param_values() is None and b.solve_status is None
    assert not b.predict({'observations': np.zeros((3, 4))}).any()
    b.set_param_values(np.arange(F))
    again = pickle.loads(pickle.dumps(b))
    assert np.array_equal(again.get_param_values(), np.arange(F))
    assert again._solver == solver and again._reg_coeff == 0.5
    assert again._pending is None and again._coeffs_dev is None
    pop = LinearFeatureBaselinePopulation(SPEC, 2, solver=solver)
    pop[1].set_param_values(np.ones(F))
    again = pickle.loads(pickle.dumps(pop))
    assert np.array_equal(again.get_param_values()[1], np.ones(F))
    assert again[0].get_param_values() is None and again._solver == solver
