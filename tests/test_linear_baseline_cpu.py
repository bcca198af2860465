"""CPU checks of the linear feature baseline: the numpy twin of
``_linear_baseline_cases.py`` says what the REAL ``LinearFeatureBaseline`` says
(``tests/golden/linear_feature_baseline.npz``, written by
``tests/golden/make_golden_linear_baseline.py``), the cases are well enough
conditioned to pin anything, the C ABI of the new entry points, their refusals
without a GPU, and the host side under the address sanitizer."""
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

import _linear_baseline_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('ga_linear_features_supported', 'ga_linear_gram_workspace_doubles',
           'ga_linear_features_gram_f64', 'ga_linear_features_predict_f32')


@pytest.fixture(scope='module')
def ref(golden):
    return golden('linear_feature_baseline')


@pytest.fixture(scope='module')
def twins():
    """name -> (phi, returns, coefficients, predictions) of the twin, once."""
    out = {}
    for name in lc.CASE_NAMES:
        obs, returns, lengths = lc.make_inputs(name)
        phi = lc.features(obs, lengths)
        coeffs = lc.fit(phi, returns)
        out[name] = (phi, returns, coeffs, phi.dot(coeffs))
    return out


def test_case_table_covers_what_it_says():
    names = lc.CASE_NAMES
    assert len(set(names)) == len(names) and set(lc.SPREAD) == set(names)
    by = {c[0]: c for c in lc.CASES}
    assert by['smallest'][1:3] == (1, [1])
    assert by['single_steps'][1:3] == (1, [1, 1, 2])
    assert by['stride4'][1:3] == (3, [5, 1, 40, 17]) and by['stride4'][3] > 0
    assert by['equal_then_ragged'][1:3] == (17, 8 * [40] + [13, 1, 27])
    assert 2 * by['exact_tiles'][1] + 4 == 64
    assert by['tile_edge'][1:3] == (31, [64, 65, 63, 1, 200])
    assert by['many_chunks'][1:3] == (4, [1000, 3])
    assert by['long_episode'][2][0] > 2 * lc.SLAB  # one episode, three slabs
    assert by['limit'][1:3] == (128, 12 * [100] + [37])
    assert [sum(by[n][2]) for n in ('slab_minus', 'slab_exact', 'slab_plus')] \
        == [lc.SLAB - 1, lc.SLAB, lc.SLAB + 1]


@pytest.mark.parametrize('name', lc.CASE_NAMES)
def test_inputs_make_the_clip_act(name):
    obs, returns, lengths = lc.make_inputs(name)
    assert obs.dtype == np.float32 and returns.dtype == np.float32
    assert obs.shape == (sum(lengths), lc.case(name)[1])
    assert np.abs(obs).max() <= 15.0
    if obs.size >= 8:
        assert (np.abs(obs) == 10.0).sum() >= 4
    if obs.size >= 1000:
        assert (np.abs(obs) > 10.0).any()


@pytest.mark.parametrize('name', lc.CASE_NAMES)
def test_twin_reproduces_the_reference(name, ref, twins):
    phi, _, coeffs, pred = twins[name]
    rows = ref[name + '/feature_rows']
    assert np.array_equal(rows, lc.golden_feature_rows(*phi.shape))
    want = ref[name + '/features']
    assert want.dtype == np.float64 and want.shape == (len(rows), phi.shape[1])
    assert np.array_equal(phi[rows], want)  # exactly
    want = ref[name + '/predictions']
    scale = max(np.abs(want).max(), 1.0)
    assert np.abs(pred - want).max() <= 1e-9 * scale
    assert ref[name + '/coeffs'].shape == coeffs.shape
    before = ref[name + '/before']
    assert before.shape == (lc.case(name)[2][0], ) and not before.any()


@pytest.mark.parametrize('name', lc.CASE_NAMES)
def test_cases_are_conditioned_well_enough_to_pin(name, twins):
    """The twin's own predictions move by at most 1e-8 when the rows are permuted
    before the fit; the recorded spread (the GPU tests' margin is 100 times it) is
    of the size measured here."""
    phi, returns, _, _ = twins[name]
    spread = lc.permutation_spread(phi, returns)
    print(name, 'spread', spread, 'recorded', lc.SPREAD[name])
    assert spread <= 1e-8
    assert lc.SPREAD[name] <= 1e-8
    # BLAS builds differ in their summation order: the recorded figure with its
    # factor 100 must still cover what this machine measures
    assert spread <= max(100 * lc.SPREAD[name], 1e-9 * np.abs(phi).max())


def test_gae_twin_appends_a_zero():
    adv, ret = lc.gae([1.0, 2.0, 4.0], [0.5, 0.25, 2.0], [2, 1], 0.5, 0.5)
    assert np.allclose(ret, [2.0, 2.0, 4.0])
    # episode 1: delta1 = 2 + 0 - 0.25, delta0 = 1 + 0.5 * 0.25 - 0.5
    assert np.allclose(adv, [0.625 + 0.25 * 1.75, 1.75, 2.0])


# ---- the C ABI -------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree():
    from garage_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\bGA_API\s+\w+\s+' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the declared argument counts are the ctypes table's
    for name in ENTRIES:
        args = re.search(name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(args.split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert lib.ga_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert _lib.SIGNATURES['ga_linear_gram_workspace_doubles'][0] is \
        ctypes.c_int64


def test_supported_on_both_sides_of_the_limits():
    from garage_amd import _lib
    lib = _lib.load()
    assert [lib.ga_linear_features_supported(o) for o in (0, 1, 128, 129)] \
        == [0, 1, 1, 0]
    assert lib.ga_linear_gram_workspace_doubles(17, 2048) == 1584
    assert lib.ga_linear_gram_workspace_doubles(17, 2049) == 2 * 1584
    assert lib.ga_linear_gram_workspace_doubles(128, 1) == 153 * 256 + 272
    assert lib.ga_linear_gram_workspace_doubles(129, 1) == -1
    assert lib.ga_linear_gram_workspace_doubles(1, 0) == -1


def _host_call(entry, spoil):
    """The entry point on host buffers it would refuse before any launch."""
    from garage_amd import _lib
    obs = np.zeros((8, 4), np.float32)
    off = np.array([0, 3, 8], np.int64)
    f64 = np.zeros(64, np.float64)
    f32 = np.zeros(8, np.float32)
    a = dict(obs=obs.ctypes.data, ldo=4, obs_dim=3, ep_off=off.ctypes.data,
             n_eps=2, S=8, returns=f32.ctypes.data, gram=f64.ctypes.data,
             rhs=f64.ctypes.data, workspace=f64.ctypes.data,
             coeffs=f64.ctypes.data, values=f32.ctypes.data, ldv=1)
    a.update(spoil)
    if entry == 'gram':
        _lib.call('ga_linear_features_gram_f64', a['obs'], a['ldo'],
                  a['obs_dim'], a['ep_off'], a['n_eps'], a['S'], a['returns'],
                  a['gram'], a['rhs'], a['workspace'], None)
    else:
        _lib.call('ga_linear_features_predict_f32', a['obs'], a['ldo'],
                  a['obs_dim'], a['ep_off'], a['n_eps'], a['S'], a['coeffs'],
                  a['values'], a['ldv'], None)


SHARED_REFUSALS = [
    ('obs', None, 'null pointer'), ('ep_off', None, 'null pointer'),
    ('obs_dim', 0, 'obs_dim'), ('obs_dim', 129, 'obs_dim'),
    ('ldo', 2, 'ldo'), ('S', 0, 'S '), ('S', 1 << 31, 'S '),
    ('n_eps', 0, 'n_eps'), ('n_eps', 9, 'n_eps'),
]


@pytest.mark.parametrize('entry', ['gram', 'predict'])
@pytest.mark.parametrize('field,value,says', SHARED_REFUSALS)
def test_both_entries_refuse_without_a_gpu(entry, field, value, says):
    from garage_amd import _lib
    with pytest.raises(_lib.GarageAmdError) as e:
        _host_call(entry, {field: value})
    assert says in str(e.value)


@pytest.mark.parametrize('entry,field,value,says', [
    ('gram', 'returns', None, 'null pointer'),
    ('gram', 'gram', None, 'null pointer'),
    ('gram', 'rhs', None, 'null pointer'),
    ('gram', 'workspace', None, 'null pointer'),
    ('gram', 'gram', 'odd', 'aligned'), ('gram', 'rhs', 'odd', 'aligned'),
    ('gram', 'workspace', 'odd', 'aligned'),
    ('predict', 'coeffs', None, 'null pointer'),
    ('predict', 'values', None, 'null pointer'),
    ('predict', 'coeffs', 'odd', 'aligned'), ('predict', 'ldv', 0, 'ldv'),
])
def test_each_entry_refuses_its_own_without_a_gpu(entry, field, value, says):
    from garage_amd import _lib
    if value == 'odd':
        keep = np.zeros(64, np.float64)
        value = keep.ctypes.data + 4
    with pytest.raises(_lib.GarageAmdError) as e:
        _host_call(entry, {field: value})
    assert says in str(e.value)


def test_host_side_under_address_sanitizer():
    """``make asan-linear-baseline``: linear_baseline_host.cpp compiled with
    ``-fsanitize=address,undefined`` for the CPU against recording fakes of the
    launch seam (tests/host/linear_baseline_harness.cpp)."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-linear-baseline'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'linear baseline ok' in out.stdout


# ---- the class, as far as it goes without a GPU ----------------------------------
def _spec(obs_dim):
    from garage_amd._dtypes import Box, EnvSpec
    return EnvSpec(Box(-np.inf, np.inf, (obs_dim, )),
                   Box(-np.inf, np.inf, (2, )), max_episode_length=20)


def test_class_surface_without_a_gpu():
    from garage_amd.baselines import LinearFeatureBaseline
    b = LinearFeatureBaseline(_spec(3))
    assert b.kind == 'linear' and b.name == 'LinearFeatureBaseline'
    assert (b.lower_bound, b.upper_bound) == (-10, 10)
    assert b.get_param_values() is None
    # predict before any fit: zeros, and no device is touched
    v = b.predict({'observations': np.ones((5, 3))})
    assert v.shape == (5, ) and v.dtype == np.float64 and not v.any()
    coeffs = np.arange(10, dtype=np.float32)
    b.set_param_values(coeffs)
    got = b.get_param_values()
    assert got.dtype == np.float64 and np.array_equal(got, coeffs)
    again = pickle.loads(pickle.dumps(b))
    assert np.array_equal(again.get_param_values(), got)
    assert again._reg_coeff == 1e-5 and again.name == b.name
    with pytest.raises(ValueError):
        b.set_param_values(np.zeros(9))
    b.set_param_values(None)
    assert b.get_param_values() is None


def test_obs_dim_129_raises():
    from garage_amd.baselines import LinearFeatureBaseline
    LinearFeatureBaseline(_spec(128))
    with pytest.raises(ValueError) as e:
        LinearFeatureBaseline(_spec(129))
    assert '129' in str(e.value) and '128' in str(e.value)
