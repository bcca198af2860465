"""The population's entry points of the linear feature baseline through the C ABI
(``ga_linear_features_gram_members_f64``, ``ga_linear_features_predict_members_f32``).

The contract is the project's twin rule: for every member, ``gram``, ``rhs`` and
``values`` carry the BITS the lone entry points (``ga_linear_features_gram_f64``,
``ga_linear_features_predict_f32``) give on that member's batch alone.  Every output
lies in sentinel-filled surroundings, the workspace has guard words behind it, and a
wider row stride carries NaN in its padding columns.

The same sets are also held to the fp64 numpy twin of ``_linear_baseline_cases.py``
at the bounds ``test_linear_baseline_gpu.py`` states for the lone entries.  Gram: two
fp64 sums of the same S products in different orders differ by at most
S * 2^-52 * sum |products|, entry by entry.  Predict: one fp32 rounding of an fp64
sum, with a factor two: 2^-23 * max(|v|, 1).

The inputs follow ``_linear_baseline_cases.make_inputs``' recipe (observations
uniform in [-3, 3], 2 % of the entries times 5, a few exactly +-10; returns
N(0, 30) plus a ramp from 100 to 0 over the episode), seeded per set and member.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _linear_baseline_cases as lc

pytestmark = pytest.mark.gpu

EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
GUARD = 64
SENTINEL = -777.0

BIG = 2048 * 1024 + 1  # one row beyond the 1024 slabs a lone grid holds

# name -> (obs_dim, [(episode lengths, ld_extra) per member])
SETS = {
    # 1, 1 and 2 workgroups: the slab_* cases
    'slabs': (2, [([700, 647, 700], 0), ([700, 648, 700], 0),
                  ([700, 649, 700], 0)]),
    'one_row': (1, [([1], 0)]),
    'single_steps': (1, [([1], 0), ([1, 1, 2], 0)]),
    # one episode across three slabs beside a small member, one stride wider
    'long_episode': (4, [([1000, 3], 0), ([4500, 3], 8)]),
    'exact_tiles': (30, [([90, 61, 120], 0), ([7], 0), ([300, 1, 2048], 4)]),
    'tile_edge': (31, [([64, 65, 63, 1, 200], 0), ([2049], 0), ([1, 1], 0)]),
    'limit': (128, [(12 * [100] + [37], 0), ([9], 0)]),
    'one_member': (4, [([33, 2100], 0)]),
    # the only shape where a workgroup takes a second slab: the stride must be the
    # member's 1024 workgroups, with a neighbour on either side of it in the grid
    'second_slab': (1, [([5], 0), (2097 * [1000] + [153], 0), ([2, 3], 0)]),
}
assert sum(SETS['second_slab'][1][1][0]) == BIG


def recipe(obs_dim, lengths, seed):
    """``_linear_baseline_cases.make_inputs`` for any shape."""
    rng = np.random.RandomState(seed)
    S = int(sum(lengths))
    obs = rng.uniform(-3.0, 3.0, size=(S, obs_dim))
    obs[rng.uniform(size=obs.shape) < 0.02] *= 5.0
    flat = obs.reshape(-1)
    n_ten = min(4, flat.size // 2)
    where = rng.choice(flat.size, size=n_ten, replace=False)
    flat[where] = np.where(np.arange(n_ten) % 2 == 0, 10.0, -10.0)
    ramp = np.concatenate([100.0 * np.arange(n, 0, -1) / n for n in lengths])
    returns = 30.0 * rng.standard_normal(S) + ramp
    return obs.astype(np.float32), returns.astype(np.float32)


class Member:
    def __init__(self, obs_dim, lengths, ld_extra, seed, dev):
        self.lengths = list(lengths)
        self.obs, self.returns = recipe(obs_dim, lengths, seed)
        self.S = len(self.returns)
        self.n_eps = len(lengths)
        ldo = lc.round4(obs_dim) + ld_extra
        padded = np.full((self.S, ldo), np.nan if ld_extra else 0.0, np.float32)
        padded[:, :obs_dim] = self.obs
        self.obs_dev = torch.from_numpy(padded).to(dev)
        self.off_dev = torch.from_numpy(np.concatenate(
            [[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
        self.returns_dev = torch.from_numpy(self.returns).to(dev)


class Set:
    """A set's members on the device, the joint and the lone results, built once."""

    def __init__(self, name):
        from garage_amd import _lib
        self.name = name
        self.obs_dim, specs = SETS[name]
        self.F = F = 2 * self.obs_dim + 4
        dev = self.dev = torch.device('cuda:0')
        seed0 = 7000 + 100 * sorted(SETS).index(name)
        self.members = [Member(self.obs_dim, lengths, extra, seed0 + m, dev)
                        for m, (lengths, extra) in enumerate(specs)]
        M = self.M = len(self.members)
        lib = _lib.load()
        # coefficients: a fit would do; any fp64 vector does for the bits
        rng = np.random.RandomState(seed0 + 99)
        self.coeffs = [rng.standard_normal(F) for _ in self.members]
        self.coeffs_dev = torch.from_numpy(np.stack(self.coeffs)).to(dev)

        # ---- the joint Gram pass: every output between sentinels
        sizes = (C.c_int64 * M)(*[mem.S for mem in self.members])
        self.need = int(lib.ga_linear_gram_members_workspace_doubles(
            self.obs_dim, M, sizes))
        assert self.need == sum(int(lib.ga_linear_gram_workspace_doubles(
            self.obs_dim, mem.S)) for mem in self.members)
        self.ws = torch.full((self.need + GUARD, ), float('nan'),
                             dtype=torch.float64, device=dev)
        self.ws[self.need:] = SENTINEL
        self.stride = GUARD + F * F + GUARD + F
        self.out = torch.full((M * self.stride + GUARD, ), SENTINEL,
                              dtype=torch.float64, device=dev)
        arr = (_lib.LinearGramMember * M)()
        for m, mem in enumerate(self.members):
            self._batch_fields(arr[m], mem)
            arr[m].returns = mem.returns_dev.data_ptr()
            arr[m].gram = self.gram_of(self.out, m).data_ptr()
            arr[m].rhs = self.rhs_of(self.out, m).data_ptr()
        _lib.call('ga_linear_features_gram_members_f64', arr, M, self.obs_dim,
                  _lib.dptr(self.ws), self.need, _lib.stream_ptr())

        # ---- the joint predict pass: strided values between sentinels
        self.ldv = 3
        self.values = [torch.full((mem.S, self.ldv), -5.0, dtype=torch.float32,
                                  device=dev) for mem in self.members]
        parr = (_lib.LinearPredictMember * M)()
        for m, mem in enumerate(self.members):
            self._batch_fields(parr[m], mem)
            parr[m].coeffs = self.coeffs_dev[m].data_ptr()
            parr[m].values, parr[m].ldv = self.values[m].data_ptr(), self.ldv
        _lib.call('ga_linear_features_predict_members_f32', parr, M,
                  self.obs_dim, _lib.stream_ptr())
        torch.cuda.synchronize()

        # ---- the lone entry points, member after member
        self.lone = []
        for m, mem in enumerate(self.members):
            need = int(lib.ga_linear_gram_workspace_doubles(self.obs_dim, mem.S))
            ws = torch.empty(need, dtype=torch.float64, device=dev)
            gram = torch.empty(F, F, dtype=torch.float64, device=dev)
            rhs = torch.empty(F, dtype=torch.float64, device=dev)
            _lib.call('ga_linear_features_gram_f64', _lib.dptr(mem.obs_dev),
                      mem.obs_dev.stride(0), self.obs_dim,
                      _lib.dptr(mem.off_dev), mem.n_eps, mem.S,
                      _lib.dptr(mem.returns_dev), _lib.dptr(gram),
                      _lib.dptr(rhs), _lib.dptr(ws), _lib.stream_ptr())
            values = torch.empty(mem.S, dtype=torch.float32, device=dev)
            _lib.call('ga_linear_features_predict_f32', _lib.dptr(mem.obs_dev),
                      mem.obs_dev.stride(0), self.obs_dim,
                      _lib.dptr(mem.off_dev), mem.n_eps, mem.S,
                      _lib.dptr(self.coeffs_dev[m]), _lib.dptr(values), 1,
                      _lib.stream_ptr())
            self.lone.append((gram, rhs, values))
        torch.cuda.synchronize()

    @staticmethod
    def _batch_fields(u, mem):
        u.obs, u.ldo = mem.obs_dev.data_ptr(), mem.obs_dev.stride(0)
        u.ep_off, u.n_eps, u.S = mem.off_dev.data_ptr(), mem.n_eps, mem.S

    def gram_of(self, out, m):
        at = m * self.stride + GUARD
        return out[at:at + self.F * self.F]

    def rhs_of(self, out, m):
        at = m * self.stride + GUARD + self.F * self.F + GUARD
        return out[at:at + self.F]


_SETS = {}


@pytest.fixture(scope='module', autouse=True)
def leave_no_nan_behind():
    """The NaNs of this module -- the padding columns of the wider strides, a
    workspace before its pass -- go back to the allocator as zeros: a later test
    that compares memory nobody wrote with ``torch.equal`` would otherwise find
    them there and fail (NaN != NaN)."""
    yield
    for s in _SETS.values():
        s.ws.zero_()
        for mem in s.members:
            mem.obs_dev.zero_()
    _SETS.clear()
    torch.cuda.synchronize()


@pytest.fixture
def members(request):
    name = request.param
    if name not in _SETS:
        _SETS[name] = Set(name)
    return _SETS[name]


all_sets = pytest.mark.parametrize('members', sorted(SETS), indirect=True)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64
                               else torch.int32)


@all_sets
def test_every_member_has_the_lone_entry_points_bits(members):
    s = members
    F = s.F
    for m, (gram, rhs, values) in enumerate(s.lone):
        assert torch.equal(_bits(s.gram_of(s.out, m)),
                           _bits(gram.view(-1))), (s.name, m, 'gram')
        assert torch.equal(_bits(s.rhs_of(s.out, m)), _bits(rhs)), (s.name, m)
        assert torch.equal(_bits(s.values[m][:, 0]), _bits(values)), (s.name, m)
        assert not bool(torch.isnan(gram).any() | torch.isnan(rhs).any())
        assert not bool(torch.isnan(values).any())
    # sentinels: everything of `out` that is no member's gram or rhs
    keep = torch.ones_like(s.out, dtype=torch.bool)
    for m in range(s.M):
        at = m * s.stride + GUARD
        keep[at:at + F * F] = False
        keep[at + F * F + GUARD:at + F * F + GUARD + F] = False
    assert bool((s.out[keep] == SENTINEL).all())
    # the workspace: all of what the library reports, nothing beyond
    assert bool((s.ws[s.need:] == SENTINEL).all())
    assert not bool(torch.isnan(s.ws[:s.need]).any())
    for v in s.values:
        assert bool((v[:, 1:] == -5.0).all())


@all_sets
def test_every_member_matches_the_fp64_twin(members):
    s = members
    for m, mem in enumerate(s.members):
        phi = lc.features(mem.obs, mem.lengths)
        r = mem.returns.astype(np.float64)
        G = s.gram_of(s.out, m).view(s.F, s.F).cpu().numpy()
        b = s.rhs_of(s.out, m).cpu().numpy()
        aphi = np.abs(phi)
        bound_G = mem.S * EPS64 * aphi.T.dot(aphi)
        bound_b = mem.S * EPS64 * aphi.T.dot(np.abs(r))
        err_G, err_b = np.abs(G - phi.T.dot(phi)), np.abs(b - phi.T.dot(r))
        print(s.name, m, 'G worst error / bound',
              np.max(err_G / np.maximum(bound_G, 1e-300)), 'b',
              np.max(err_b / np.maximum(bound_b, 1e-300)))
        assert (err_G <= bound_G).all() and (err_b <= bound_b).all()
        assert np.array_equal(G, G.T)  # exactly symmetric
        pred = phi.dot(s.coeffs[m])
        v = s.values[m][:, 0].cpu().numpy().astype(np.float64)
        bound = EPS32 * np.maximum(np.abs(pred), 1.0)
        print(s.name, m, 'values worst error / bound',
              np.max(np.abs(v - pred) / bound))
        assert (np.abs(v - pred) <= bound).all()


@pytest.mark.parametrize('members', ['exact_tiles'], indirect=True)
def test_a_member_without_coefficients_gets_zeros(members):
    from garage_amd import _lib
    s = members
    values = [torch.full((mem.S, 2), -5.0, dtype=torch.float32, device=s.dev)
              for mem in s.members]
    parr = (_lib.LinearPredictMember * s.M)()
    for m, mem in enumerate(s.members):
        s._batch_fields(parr[m], mem)
        parr[m].coeffs = None if m == 1 else s.coeffs_dev[m].data_ptr()
        parr[m].values, parr[m].ldv = values[m].data_ptr(), 2
    _lib.call('ga_linear_features_predict_members_f32', parr, s.M, s.obs_dim,
              _lib.stream_ptr())
    for m in range(s.M):
        want = torch.zeros_like(s.lone[m][2]) if m == 1 else s.lone[m][2]
        assert torch.equal(_bits(values[m][:, 0]), _bits(want)), m
        assert bool((values[m][:, 1] == -5.0).all())


# ---- refusals: the error, and nothing written ---------------------------------------
def _spoilt_gram(s, spoil):
    from garage_amd import _lib
    lib = _lib.load()
    F, M = s.F, s.M
    out = torch.full((M * s.stride + GUARD, ), SENTINEL, dtype=torch.float64,
                     device=s.dev)
    ws = torch.full((s.need + GUARD, ), SENTINEL, dtype=torch.float64,
                    device=s.dev)
    arr = (_lib.LinearGramMember * M)()
    for m, mem in enumerate(s.members):
        s._batch_fields(arr[m], mem)
        arr[m].returns = mem.returns_dev.data_ptr()
        arr[m].gram = s.gram_of(out, m).data_ptr()
        arr[m].rhs = s.rhs_of(out, m).data_ptr()
    call = dict(members=arr, n=M, obs_dim=s.obs_dim, ws=ws.data_ptr(),
                ws_doubles=s.need)
    spoil(call, arr)
    rc = lib.ga_linear_features_gram_members_f64(
        call['members'], call['n'], call['obs_dim'], call['ws'],
        call['ws_doubles'], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0 and lib.ga_last_error()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    del F


def _set(field, value, m=1):
    def spoil(call, arr):
        setattr(arr[m], field, value)
    return spoil


def _arg(name, value):
    def spoil(call, arr):
        call[name] = value
    return spoil


def _shift(field, m=1):
    def spoil(call, arr):
        setattr(arr[m], field, getattr(arr[m], field) + 4)
    return spoil


GRAM_REFUSALS = {
    'null members': _arg('members', None),
    'no members': _arg('n', 0),
    '1025 members': _arg('n', 1025),
    'obs_dim 0': _arg('obs_dim', 0),
    'obs_dim 129': _arg('obs_dim', 129),
    'null workspace': _arg('ws', None),
    'workspace a double short': lambda call, arr: call.update(
        ws_doubles=call['ws_doubles'] - 1),
    'misaligned workspace': lambda call, arr: call.update(ws=call['ws'] + 4),
    'null obs': _set('obs', None),
    'null ep_off': _set('ep_off', None, m=2),
    'ldo < obs_dim': _set('ldo', 3),
    'S = 0': _set('S', 0, m=0),
    'S = 2^31': _set('S', 1 << 31),
    'n_eps = 0': _set('n_eps', 0),
    'n_eps > S': _set('n_eps', 1 << 20, m=2),
    'null returns': _set('returns', None, m=2),
    'null gram': _set('gram', None),
    'null rhs': _set('rhs', None, m=0),
    'misaligned gram': _shift('gram'),
    'misaligned rhs': _shift('rhs', m=2),
}


@pytest.mark.parametrize('what', sorted(GRAM_REFUSALS))
@pytest.mark.parametrize('members', ['exact_tiles'], indirect=True)
def test_gram_refusals_write_nothing(members, what):
    _spoilt_gram(members, GRAM_REFUSALS[what])


PREDICT_REFUSALS = {
    'null members': _arg('members', None),
    'no members': _arg('n', 0),
    '1025 members': _arg('n', 1025),
    'obs_dim 0': _arg('obs_dim', 0),
    'obs_dim 129': _arg('obs_dim', 129),
    'null obs': _set('obs', None),
    'null ep_off': _set('ep_off', None, m=2),
    'ldo < obs_dim': _set('ldo', 3),
    'S = 0': _set('S', 0, m=0),
    'S = 2^31': _set('S', 1 << 31),
    'n_eps = 0': _set('n_eps', 0),
    'n_eps > S': _set('n_eps', 1 << 20, m=2),
    'null values': _set('values', None),
    'misaligned coeffs': _shift('coeffs', m=2),
    'ldv = 0': _set('ldv', 0, m=0),
}


@pytest.mark.parametrize('what', sorted(PREDICT_REFUSALS))
@pytest.mark.parametrize('members', ['exact_tiles'], indirect=True)
def test_predict_refusals_write_nothing(members, what):
    from garage_amd import _lib
    s = members
    lib = _lib.load()
    values = [torch.full((mem.S, ), -5.0, dtype=torch.float32, device=s.dev)
              for mem in s.members]
    arr = (_lib.LinearPredictMember * s.M)()
    for m, mem in enumerate(s.members):
        s._batch_fields(arr[m], mem)
        arr[m].coeffs = s.coeffs_dev[m].data_ptr()
        arr[m].values, arr[m].ldv = values[m].data_ptr(), 1
    call = dict(members=arr, n=s.M, obs_dim=s.obs_dim)
    PREDICT_REFUSALS[what](call, arr)
    rc = lib.ga_linear_features_predict_members_f32(
        call['members'], call['n'], call['obs_dim'], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0 and lib.ga_last_error()
    for v in values:
        assert bool((v == -5.0).all())


def test_workspace_size_refuses_what_the_pass_refuses():
    from garage_amd import _lib
    lib = _lib.load()
    ok = (C.c_int64 * 2)(5, 2049)
    assert lib.ga_linear_gram_members_workspace_doubles(1, 2, ok) == 3 * 272
    assert lib.ga_linear_gram_members_workspace_doubles(0, 2, ok) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(129, 2, ok) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(1, 0, ok) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(1, 1025, ok) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(1, 2, None) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(
        1, 2, (C.c_int64 * 2)(5, 0)) == -1
    assert lib.ga_linear_gram_members_workspace_doubles(
        1, 2, (C.c_int64 * 2)(5, 1 << 31)) == -1
