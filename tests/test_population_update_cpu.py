"""CPU checks of the population update: what ``ga_update_epoch_members`` refuses
before any launch, which networks it takes, the host loop under AddressSanitizer
(``make asan-members``) and ``PopulationPPO``'s constructor errors."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from garage_amd import _lib
from garage_amd._dtypes import Box, EnvSpec
from garage_amd.engine import FlatMLP, round4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')
BASE = 0x100000  # addresses that are never read: every call below is refused first


def _args(n_members=3, kind=0, hidden=(64, 64), in_w=4, out_w=2, mb=64):
    """A pass the library would take, on made-up device addresses."""
    net = FlatMLP(in_w, out_w, hidden, CPU)
    a = _lib.UpdateMembersArgs()
    a.desc = C.pointer(net._desc)
    a.kind, a.algo, a.learn_std = kind, 0, 1
    a.beta1, a.beta2, a.eps, a.mb = 0.9, 0.999, 1e-8, mb
    a.n_members = n_members
    arr = (_lib.MemberUpdate * max(n_members, 1))()
    for u in arr:
        u.params, u.grads = BASE, BASE + 0x10000
        u.exp_avg, u.exp_avg_sq = BASE + 0x20000, BASE + 0x30000
        u.X, u.ldx, u.S, u.perm = BASE + 0x40000, round4(in_w), 130, BASE
        u.actions, u.lda = BASE + 0x50000, round4(out_w)
        u.old_ll = u.adv = u.returns = BASE + 0x60000
        u.lr, u.clip = 1e-3, 0.2
    a.members_host = arr
    a.partials = BASE + 0x70000
    a.partials_floats = _lib.load().ga_update_members_partials_floats(
        a.desc, max(n_members, 1), 130 if mb == 0 else min(130, mb))
    assert a.partials_floats > 0
    return a, (net, arr)


def _set(field, value):
    def spoil(a, arr):
        setattr(a, field, value)
    return spoil


def _member(m, field, value):
    def spoil(a, arr):
        setattr(arr[m], field, value)
    return spoil


def _desc(field, value, index=None):
    def spoil(a, arr):
        if index is None:
            setattr(a.desc.contents, field, value)
        else:
            getattr(a.desc.contents, field)[index] = value
    return spoil


REFUSALS = {
    'null desc': (_set('desc', None), 'null pointer'),
    'null members': (_set('members_host', None), 'null pointer'),
    'null partials': (_set('partials', None), 'null pointer'),
    'null params': (_member(1, 'params', None), 'null pointer'),
    'null grads': (_member(0, 'grads', None), 'null pointer'),
    'null exp_avg': (_member(2, 'exp_avg', None), 'null pointer'),
    'null exp_avg_sq': (_member(2, 'exp_avg_sq', None), 'null pointer'),
    'null X': (_member(1, 'X', None), 'null pointer'),
    'null perm': (_member(1, 'perm', None), 'null pointer'),
    'null actions': (_member(0, 'actions', None), 'null pointer'),
    'null adv': (_member(0, 'adv', None), 'null pointer'),
    'null old_ll': (_member(2, 'old_ll', None), 'null pointer'),
    'no members': (_set('n_members', 0), 'n_members'),
    'too many members': (_set('n_members', 1025), 'n_members'),
    'three hidden widths differ': (_desc('dims', 32, 2), 'unsupported network'),
    'H = 128': (lambda a, arr: (_desc('dims', 128, 1)(a, arr),
                                _desc('dims', 128, 2)(a, arr)),
                'unsupported network'),
    '33 inputs': (_desc('dims', 33, 0), 'unsupported network'),
    '9 outputs': (_desc('dims', 9, 3), 'unsupported network'),
    'relu': (_desc('hidden_act', 1), 'unsupported network'),
    'tanh head': (_desc('output_act', 1), 'unsupported network'),
    'layer norm': (_desc('layer_norm', 1), 'unsupported network'),
    'one hidden layer': (_desc('n_layers', 2), 'unsupported network'),
    'params row off a quad': (_member(1, 'params', BASE + 4), 'aligned'),
    'moments row off a quad': (_member(1, 'exp_avg_sq', BASE + 8), 'aligned'),
    'grads row off a quad': (_member(2, 'grads', BASE + 12), 'aligned'),
    'X off a quad': (_member(0, 'X', BASE + 4), 'aligned'),
    'ldx not a quad': (_member(0, 'ldx', 5), 'aligned'),
    'ldx too short': (_member(0, 'ldx', 0), 'aligned'),
    'lda not a quad': (_member(0, 'lda', 3), 'aligned'),
    'actions off a quad': (_member(2, 'actions', BASE + 4), 'aligned'),
    'partials off a quad': (_set('partials', BASE + 4), 'aligned'),
    'weights off a quad': (_desc('w_off', 6, 1), 'offsets'),
    'S = 0': (_member(2, 'S', 0), 'bad S'),
    'S < 0': (_member(0, 'S', -5), 'bad S'),
    'mb < 0': (_set('mb', -1), 'bad mb'),
    'step0 < 0': (_member(0, 'step0', -1), 'bad step0'),
    'kind 3': (_set('kind', 3), 'kind'),
    'kind -1': (_set('kind', -1), 'kind'),
    'algo 2': (_set('algo', 2), 'algo'),
    'algo -1': (_set('algo', -1), 'algo'),
}


@pytest.mark.parametrize('what', sorted(REFUSALS))
def test_refused_before_any_launch(what):
    lib = _lib.load()
    spoil, message = REFUSALS[what]
    a, keep = _args()
    spoil(a, keep[1])
    assert lib.ga_update_epoch_members(C.byref(a), None) < 0
    assert message in lib.ga_last_error().decode()


def test_null_args_and_small_scratch_are_refused():
    lib = _lib.load()
    assert lib.ga_update_epoch_members(None, None) < 0
    assert 'null pointer' in lib.ga_last_error().decode()
    for mb in (0, 64, 100):
        a, keep = _args(mb=mb)
        a.partials_floats -= 1
        assert lib.ga_update_epoch_members(C.byref(a), None) < 0
        assert 'partials too small' in lib.ga_last_error().decode()
    # the value function's pass reads returns, not the policy's arrays
    a, keep = _args(kind=1, out_w=1)
    keep[1][1].returns = None
    assert lib.ga_update_epoch_members(C.byref(a), None) < 0
    assert 'returns' in lib.ga_last_error().decode()


def test_scratch_size():
    lib = _lib.load()
    for H, in_w in ((64, 4), (32, 17)):
        net = FlatMLP(in_w, 2, (H, H), CPU)
        stride = H * round4(in_w) + H + H * H + H + 8 * H + 8
        for n, rows in ((1, 1), (3, 64), (5, 65), (64, 256), (1024, 200)):
            tiles = -(-rows // 64)
            assert lib.ga_update_members_partials_floats(
                C.byref(net._desc), n, rows) == n * tiles * (4 + stride)
        for n, rows in ((0, 64), (1025, 64), (3, 0), (3, 1 << 31)):
            assert lib.ga_update_members_partials_floats(
                C.byref(net._desc), n, rows) == 0
    assert lib.ga_update_members_partials_floats(None, 3, 64) == 0


def _narrow_step_takes(net):
    """``ga_narrow_step_supported`` as the lone epoch loop applies it: the scratch of
    a one-tile step has the narrow kernel's layout."""
    H, in_w = net.dims[1], net.dims[0]
    stride = H * round4(in_w) + H + H * H + H + 8 * H + 8
    return _lib.load().ga_update_partials_floats(C.byref(net._desc),
                                                 64) == 4 + stride


@pytest.mark.parametrize('hidden', [(32, 32), (64, 64), (128, 128), (64, 32),
                                    (32, 64)])
def test_supported_networks_are_the_narrow_step_s(hidden):
    lib = _lib.load()
    for in_w in (1, 32, 33):
        for out_w in (1, 8, 9):
            net = FlatMLP(in_w, out_w, hidden, CPU)
            want = (hidden in ((32, 32), (64, 64)) and in_w <= 32
                    and out_w <= 8)
            got = lib.ga_update_members_supported(C.byref(net._desc))
            assert got == int(want), (hidden, in_w, out_w)
            assert bool(got) == _narrow_step_takes(net), (hidden, in_w, out_w)
    assert lib.ga_update_members_supported(None) == 0
    for kw in (dict(hidden_act='relu'), dict(output_act='tanh'),
               dict(layer_norm=True)):
        net = FlatMLP(4, 2, (64, 64), CPU, **kw)
        assert lib.ga_update_members_supported(C.byref(net._desc)) == 0
    assert lib.ga_update_members_supported(
        C.byref(FlatMLP(4, 2, (64, ), CPU)._desc)) == 0


def test_members_loop_under_address_sanitizer():
    """``make asan-members``: the population's epoch loop (update_members.cpp) compiled
    with ``-fsanitize=address,undefined`` for the CPU and run against fakes of its two
    launches and of the HIP calls it makes (tests/host/update_members_harness.cpp):
    which ids form member ``m``'s step ``k``, which members are active in which step,
    the Adam table against ``ga_adam_coeffs(step0_m + k + 1)``, the launch count of a
    pass, tables of exactly the sizes allocated, nothing launched after a refusal;
    S = (130, 64, 200, 1, 65), mb in {0, 64, 100}."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-members'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'members loop ok' in out.stdout


def test_profile_kind_is_appended():
    lib = _lib.load()
    assert lib.ga_launch_count(15) >= 0
    assert lib.ga_launch_count(16) == -1
    assert lib.ga_abi_version() == 5


# -- PopulationPPO's constructor ---------------------------------------------------
SPEC = EnvSpec(Box(-1, 1, (4, )), Box(-1, 1, (2, )), max_episode_length=8)


def _learner(cls=None, hidden=(32, 32), vf_hidden=None, lr=1e-3, mb=64, epochs=2,
            permutation='device', optimizer=None, policy_kw=None, seed=0, **kw):
    from garage_amd.algos import PPO
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    cls = cls or PPO
    pol = GaussianMLPPolicy(SPEC, hidden_sizes=hidden, device=CPU,
                            **(policy_kw or {}))
    vf = GaussianMLPValueFunction(SPEC, hidden_sizes=vf_hidden or hidden,
                                  device=CPU)
    opt = optimizer or (torch.optim.Adam, dict(lr=lr))
    return cls(env_spec=SPEC, policy=pol, value_function=vf, sampler=None,
               policy_optimizer=OptimizerWrapper(opt, pol, epochs, mb,
                                                 permutation=permutation,
                                                 seed=seed),
               vf_optimizer=OptimizerWrapper((torch.optim.Adam, dict(lr=lr)),
                                             vf, epochs, mb,
                                             permutation=permutation,
                                             seed=seed + 100), **kw)


def _vpg():
    from garage_amd.algos import VPG
    return VPG


def _trpo():
    """Stands for anything that is not exactly a PPO or a VPG."""
    from garage_amd.algos import TRPO
    return object.__new__(TRPO)


def test_population_ppo_takes_members_that_differ_where_they_may():
    from garage_amd.algos import PopulationPPO, VPG
    members = [_learner(lr=1e-3 * (m + 1), lr_clip_range=0.1 * (m + 1), seed=m,
                       policy_ent_coeff=0.01 * m, entropy_method='regularized')
               for m in range(3)]
    before = [a.policy.net.params.clone() for a in members]
    pop = PopulationPPO(members)
    n_flat = members[0].policy.net.n_flat
    assert pop.member_params.shape == (3, n_flat)
    for m, a in enumerate(members):
        # a member's buffers ARE its rows
        for which, mod in (('policy', a.policy), ('vf', a._value_function)):
            for name in ('params', 'grads', 'exp_avg', 'exp_avg_sq'):
                assert getattr(mod.net, name).data_ptr() == \
                    pop._rows[which][name][m].data_ptr()
        assert torch.equal(pop.member_params[m], before[m])
    PopulationPPO([_learner(cls=VPG), _learner(cls=VPG)])


@pytest.mark.parametrize('what,make,message', [
    ('no members', lambda: [], 'at least one member'),
    ('a TRPO member', lambda: [_learner(), _trpo()], 'PPO or VPG'),
    ('PPO with VPG', lambda: [_learner(), _learner(cls=_vpg())], 'algorithm'),
    ('hidden sizes', lambda: [_learner(), _learner(hidden=(64, 64))],
     'network shape'),
    ('a wide member', lambda: [_learner(hidden=(128, 128))], 'unsupported'),
    ('a wide value function', lambda: [_learner(vf_hidden=(32, 16))],
     'unsupported'),
    ('relu', lambda: [_learner(policy_kw=dict(hidden_nonlinearity=torch.relu))],
     'unsupported'),
    ('minibatch size', lambda: [_learner(), _learner(mb=32)], 'minibatch_size'),
    ('epochs', lambda: [_learner(), _learner(epochs=3)],
     'max_optimization_epochs'),
    ('permutation', lambda: [_learner(), _learner(permutation='numpy')],
     'permutation'),
    ('entropy', lambda: [_learner(), _learner(entropy_method='regularized',
                                            policy_ent_coeff=0.01)],
     'entropy_method'),
    ('std options', lambda: [_learner(), _learner(policy_kw=dict(min_std=0.1))],
     'std options'),
    ('betas', lambda: [_learner(), _learner(optimizer=(
        torch.optim.Adam, dict(lr=1e-3, betas=(0.8, 0.999))))], 'betas'),
    ('SGD', lambda: [_learner(optimizer=(torch.optim.SGD, dict(lr=1e-3)))],
     'default-shaped Adam'),
    ('weight decay', lambda: [_learner(optimizer=(
        torch.optim.Adam, dict(lr=1e-3, weight_decay=0.1)))],
     'default-shaped Adam'),
])
def test_population_ppo_names_what_it_refuses(what, make, message):
    from garage_amd.algos import PopulationPPO
    members = make()
    with pytest.raises(ValueError) as e:
        PopulationPPO(members)
    assert message in str(e.value), str(e.value)


def test_population_ppo_refuses_a_shared_network_and_a_wrong_sampler():
    import types
    from garage_amd.algos import PopulationPPO
    a = _learner()
    with pytest.raises(ValueError) as e:
        PopulationPPO([a, a])
    assert 'of its own' in str(e.value)
    with pytest.raises(ValueError) as e:
        PopulationPPO([_learner(), _learner()],
                      sampler=types.SimpleNamespace(n_members=3))
    assert 'rolls out 3' in str(e.value)
    with pytest.raises(ValueError) as e:
        PopulationPPO([_learner()]).train(None)
    assert 'GpuPopulationSampler' in str(e.value)
