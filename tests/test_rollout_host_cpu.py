"""CPU check of the rollout step's host side (rollout_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, 'garage_amd', '_C', 'rollout_host_asan_test')


def test_host_side_of_the_rollout_step_under_address_sanitizer():
    """The argument checks, the conversions of the C-ABI structs, the kernel choice,
    grid, member split and profile counts of the rollout step's launches, compiled
    with ``-fsanitize=address,undefined`` for the CPU and run as a stand-alone
    program against fakes of the launch seam (tests/host/rollout_host_harness.cpp):
    every fake touches what its kernel would in exactly-sized buffers, the expected
    variant of every network, option and switch setting is a literal table, and
    every refusal of every entry point precedes the first launch for every env
    kind."""
    subprocess.run(['make', '-C', ROOT, os.path.relpath(PROGRAM, ROOT)],
                   capture_output=True, text=True, timeout=300, check=True)
    out = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'rollout host ok' in out.stdout
