"""The host side of the population's joint diagnostics without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_members_diag_host_under_address_sanitizer():
    """``make asan-members-diag``: members_diag_host.cpp and the per-layer dispatch
    it asks for the members' forward plans (mlp_layers.cpp), compiled with
    ``-fsanitize=address,undefined`` for the CPU and run as a program against a fake
    kernel side of its own (tests/host/members_diag_harness.cpp): every table
    entry of the joint forward against the struct the LONE entry point launches
    for the same arguments (pointers, rows, strides, plan, grid), which kernels
    members of different row counts take and how many launches that makes, every
    member's stretch of the partials (disjoint, inside an allocation of exactly
    ``ga_members_diag_partials_doubles``), one table copy a call, every argument
    error of every entry point, and that an error copies and launches nothing."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-members-diag'],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for suite in ('forward', 'losses', 'errors'):
        assert 'members diag {} ok'.format(suite) in out.stdout


def test_refusals_reach_python_without_a_gpu():
    from garage_amd import _lib
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_mlp_forward_members_f32', None, None, 1, None)
    assert 'null pointer' in str(e.value)
    arr = (_lib.MemberNll * 1)()
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_gaussian_nll_members_f32', arr, 1025, None, 0, None)
    assert 'n_members must be 1 .. 1024' in str(e.value)
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_gaussian_nll_members_f32', arr, 1, None, 0, None)
    assert 'member 0: null pointer' in str(e.value)
    rows = (C.c_int64 * 3)(1, 257, 1000)
    assert _lib.load().ga_members_diag_partials_doubles(rows, 3) == 2 * (1 + 2 + 4)


def test_the_forward_predicate_follows_the_developer_switch():
    """``ga_mlp_forward_members_supported``: what ``PopulationPPO`` asks at
    construction and before every iteration."""
    import torch
    from garage_amd import _lib
    from garage_amd.engine import FlatMLP
    lib = _lib.load()
    net = FlatMLP(4, 2, (64, 64), torch.device('cpu'))
    wide = FlatMLP(4, 2, (128, 128), torch.device('cpu'))
    assert lib.ga_mlp_forward_members_supported(C.byref(net._desc)) == 1
    assert lib.ga_mlp_forward_members_supported(C.byref(wide._desc)) == 0
    lib.ga_set_fused_forward(1)
    try:
        assert lib.ga_mlp_forward_members_supported(C.byref(net._desc)) == 0
        assert b'ga_set_fused_forward' in lib.ga_last_error()
    finally:
        lib.ga_set_fused_forward(0)
    assert lib.ga_mlp_forward_members_supported(C.byref(net._desc)) == 1


def test_population_ppo_takes_the_keyword():
    """The flag exists, is off by default, and an old pickle's state gets it."""
    import inspect
    from garage_amd.algos import PopulationPPO
    sig = inspect.signature(PopulationPPO.__init__)
    assert sig.parameters['joint_diagnostics'].default is False
    assert list(sig.parameters)[:3] == ['self', 'members', 'sampler']
