"""Population rollouts without a GPU: the policies' flat-vector helpers and
``pack_members`` (on CPU tensors), the declaration of
``ga_policy_env_step_members_f32`` in header, library and ctypes table, and every
refusal of that entry point through ctypes with host pointers -- each check
precedes the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from garage_amd import _lib
from garage_amd._dtypes import Box, Discrete, EnvSpec
from garage_amd.engine import FlatMLP, round4
from garage_amd.policies import CategoricalMLPPolicy, GaussianMLPPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def _gaussian(learn_std, layer_norm=False, hidden=(5, 3)):
    spec = EnvSpec(Box(-np.inf, np.inf, (6, )), Box(-np.inf, np.inf, (3, )),
                   max_episode_length=8)
    torch.manual_seed(3)
    return GaussianMLPPolicy(spec, hidden_sizes=hidden, learn_std=learn_std,
                             init_std=0.7, layer_normalization=layer_norm,
                             hidden_nonlinearity=torch.relu if layer_norm
                             else torch.tanh, device=CPU)


def _categorical():
    spec = EnvSpec(Box(-np.inf, np.inf, (4, )), Discrete(2),
                   max_episode_length=8)
    torch.manual_seed(4)
    return CategoricalMLPPolicy(spec, hidden_sizes=(7, ), device=CPU)


POLICIES = {
    'gaussian_learn_std': lambda: _gaussian(True),
    'gaussian_fixed_std': lambda: _gaussian(False),
    'gaussian_layer_norm': lambda: _gaussian(True, layer_norm=True),
    'categorical': _categorical,
}


@pytest.mark.parametrize('name', sorted(POLICIES))
def test_flat_vector_is_parameters_order_and_round_trips(name):
    pol = POLICIES[name]()
    flat = pol.get_flat_param_values()
    want = np.concatenate([p.reshape(-1).numpy() for p in pol.parameters()])
    assert flat.dtype == np.float32 and flat.ndim == 1
    assert np.array_equal(flat, want)
    # odd widths: the compact vector leaves the padding of the device layout out
    assert flat.size < pol.net.n_flat - 3
    new = np.arange(flat.size, dtype=np.float32) * 0.5 - 3
    before = pol.net.params.clone()
    pol.set_flat_param_values(new)
    assert np.array_equal(pol.get_flat_param_values(), new)
    # only the trainable slots moved: padding stays zero, a fixed std stays put
    idx = pol._flat_index()
    rest = torch.ones(pol.net.n_flat, dtype=torch.bool)
    rest[idx] = False
    assert torch.equal(pol.net.params[rest], before[rest])
    with pytest.raises(ValueError, match='flat parameter vector'):
        pol.set_flat_param_values(new[:-1])


@pytest.mark.parametrize('name', sorted(POLICIES))
def test_pack_members_layout_padding_and_std(name):
    pol = POLICIES[name]()
    net, M = pol.net, 3
    P = pol.get_flat_param_values().size
    rng = np.random.RandomState(5)
    vectors = rng.randn(M, P)  # float64 in, float32 out
    packed = pol.pack_members(vectors)
    assert packed.shape == (M, net.n_flat) and packed.dtype == torch.float32
    assert net.n_flat % 4 == 0 and packed.stride(0) == net.n_flat
    template = net.params.clone()
    for m in range(M):
        # the row, loaded as the policy's parameters, reads back as the vector
        net.params.copy_(packed[m])
        assert np.array_equal(pol.get_flat_param_values(),
                              vectors[m].astype(np.float32))
        # every weight's padded columns and every bias's padded tail are zero
        for l in range(len(net.dims) - 1):
            rows, cols = net.dims[l + 1], net.dims[l]
            w = packed[m, net.w_off[l]:net.w_off[l] + rows * round4(cols)]
            assert not w.view(rows, round4(cols))[:, cols:].any()
            b = packed[m, net.b_off[l]:net.b_off[l] + round4(rows)]
            assert not b[rows:].any()
        for l, o in enumerate(net.ln_off):
            n, d = round4(net.dims[l]), net.dims[l]
            assert not packed[m, o + d:o + n].any()
            assert not packed[m, o + n + d:o + 2 * n].any()
        assert not packed[m, 1:4].any()
        if pol._learn_std:
            assert packed[m, 0] == np.float32(vectors[m, 0])
        else:  # the template's own log-std, for every member
            assert packed[m, 0] == template[0]
    net.params.copy_(template)
    if not pol._learn_std and pol.kind == 'gaussian':
        assert packed[0, 0] == np.float32(np.log(0.7))
    with pytest.raises(ValueError, match='pack_members needs'):
        pol.pack_members(vectors[:, :-1])


def test_header_library_and_ctypes_table_agree():
    name = 'ga_policy_env_step_members_f32'
    text = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    decl = re.search(r'GA_API int %s\((.*?)\);' % name, text, flags=re.S)
    assert decl, 'not declared in the header'
    args = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == [
        'd', 'params', 'head', 'env', 'rec', 'norm', 'n_steps', 'n_members',
        'member_stride', 'stream']
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(args)
    assert argtypes[6:9] == [C.c_int64] * 3
    assert all(a.startswith('int64_t') for a in args[6:9])
    lib = _lib.load()
    assert hasattr(lib, name)
    assert lib.ga_abi_version() == 5
    # the host loop of ga_rollout_env_steps does not know the symbol: its
    # sanitizer harness links rollout_loop.cpp against fakes of what it calls
    loop = open(os.path.join(ROOT, 'garage_amd', 'csrc',
                             'rollout_loop.cpp')).read()
    assert name not in loop


def _args(n=64, hidden=(8, 8), obs=4, out=2):
    """A call that passes every check of its own (host pointers throughout:
    none of the calls below may reach a launch)."""
    net = FlatMLP(obs, out, hidden, CPU)
    buf = (C.c_float * 16)()
    addr = C.addressof(buf)
    head = _lib.HeadArgs(n=n, A=out, kind=1, obs=addr, ldo=4, obs_dim=obs,
                         col=0, Tcap=8, action=addr, lda=4, obs_buf=addr,
                         act_buf=addr)
    rec = _lib.RecordArgs(
        n=n, col=0, Tcap=8, max_episode_length=5, reward=addr, step_type=addr,
        next_obs=addr, ldo=4, obs_dim=obs, ep_t=addr, rew_buf=addr,
        st_buf=addr, tail_buf=addr, lastobs_buf=addr, done=addr, step_eps=addr,
        step_samples=addr)
    env = _lib.CartPoleEnv(n=n, max_episode_length=5, state=addr, t=addr,
                           resets=addr)
    ref = _lib.env_ref(_lib.ENV_CARTPOLE, env)
    return dict(net=net, addr=addr, head=head, rec=rec, ref=ref, buf=buf)


def _call(a, n_members, stride=None, norm=None, params='addr', n_steps=4,
          desc=None):
    net = a['net']
    _lib.call('ga_policy_env_step_members_f32',
              C.byref(net._desc if desc is None else desc),
              a['addr'] if params == 'addr' else params, C.byref(a['head']),
              C.byref(a['ref']), C.byref(a['rec']),
              None if norm is None else C.byref(norm), n_steps, n_members,
              net.n_flat if stride is None else stride, None)


def test_every_refusal_precedes_the_launch():
    name = 'ga_policy_env_step_members_f32'
    a = _args()
    flat = a['net'].n_flat
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _call(a, 2, params=None)
    for bad in (0, -3):
        with pytest.raises(_lib.GarageAmdError,
                           match='n_members must be at least 1'):
            _call(a, bad)
    with pytest.raises(_lib.GarageAmdError,
                       match='64 envs do not split into 3 members'):
        _call(a, 3)
    # 64 / 8 = 8 envs per member: half a workgroup
    with pytest.raises(_lib.GarageAmdError,
                       match='8 envs per member are not a multiple of the 16'):
        _call(a, 8)
    b = _args(n=96)  # 96 / 4 = 24
    with pytest.raises(_lib.GarageAmdError, match='24 envs per member'):
        _call(b, 4)
    with pytest.raises(_lib.GarageAmdError, match='not a multiple of 4 floats'):
        _call(a, 2, stride=flat + 2)
    with pytest.raises(_lib.GarageAmdError,
                       match='smaller than the %d floats' % flat):
        _call(a, 2, stride=flat - 4)
    with pytest.raises(_lib.GarageAmdError, match='smaller than'):
        _call(a, 2, stride=0)
    a['head'].noise = a['addr']
    with pytest.raises(_lib.GarageAmdError, match='teacher-forced noise'):
        _call(a, 2)
    with pytest.raises(_lib.GarageAmdError, match='teacher-forced noise'):
        _call(a, 2, n_steps=1)  # (the single-policy entry takes it per step)
    a['head'].noise = None
    norm = _lib.NormArgs(act_low=a['addr'], act_high=a['addr'],
                         scaled_action=a['addr'])
    with pytest.raises(_lib.GarageAmdError, match='action rescale'):
        _call(a, 2, norm=norm)
    wide = FlatMLP(4, 2, (600, ), CPU)  # a layer input past 512
    with pytest.raises(_lib.GarageAmdError,
                       match='network not supported by the fused step'):
        _call(a, 2, desc=wide._desc, stride=wide.n_flat)
    big_head = FlatMLP(4, 40, (8, ), CPU)  # more than 32 outputs
    with pytest.raises(_lib.GarageAmdError, match='network not supported'):
        _call(a, 2, desc=big_head._desc, stride=big_head.n_flat)
    bad = _lib.EnvRef(kind=7, env=a['addr'])
    a['ref'] = bad
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _call(a, 2)
    assert name.encode() in _lib.load().ga_last_error()


def test_flat_size_the_stride_is_checked_against_counts_layer_norm():
    """The smallest stride is the descriptor's whole vector: with LayerNorm its
    gamma / beta blocks sit behind the last bias."""
    a = _args()
    ln = FlatMLP(4, 2, (8, 8), CPU, hidden_act='relu', layer_norm=True)
    assert ln.n_flat > a['net'].n_flat
    with pytest.raises(_lib.GarageAmdError,
                       match='smaller than the %d floats' % ln.n_flat):
        _call(a, 2, desc=ln._desc, stride=ln.n_flat - 4)
