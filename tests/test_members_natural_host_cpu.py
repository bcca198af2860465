"""The host side of the population's natural-gradient step without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_members_natural_host_under_address_sanitizer():
    """``make asan-members-natural``: members_natural_host.cpp compiled with
    ``-fsanitize=address,undefined`` for the CPU and run as a program against fakes of
    the launch seam (tests/host/members_natural_harness.cpp): the launch sequence of a
    solve (2 (cg_iters + 1) + 2), a product and a backtrack round, the table's
    contents, every member's stretch of an exactly sized workspace, one table copy a
    call, and that every refusal copies and launches nothing."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-members-natural'],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'members natural ok' in out.stdout


def test_refusals_reach_python_without_a_gpu():
    from garage_amd import _lib
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_members_natural_solve', None, None)
    assert 'null pointer' in str(e.value)
    assert _lib.load().ga_members_natural_supported(None) == 0
    a = _lib.MembersNaturalArgs()
    with pytest.raises(_lib.GarageAmdError) as e:
        _lib.call('ga_members_natural_candidates', C.byref(a), 0, None)
    assert 'null pointer' in str(e.value)
