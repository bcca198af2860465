"""CPU check of the fused optimizer step's host side (fused_train_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, 'garage_amd', '_C', 'fused_host_asan_test')


def test_host_side_of_the_fused_step_under_address_sanitizer():
    """The argument checks, kernel choice, grids, slab offsets, optimizer grid and
    weight-plane cache of the fused launches, compiled with
    ``-fsanitize=address,undefined`` for the CPU and run as a stand-alone program
    against fakes of the launch seam (tests/host/fused_host_harness.cpp): every fake
    touches what its kernel would in exactly-sized buffers, the expected variant of
    every shape and switch setting is a literal table, and every refusal precedes
    the first launch."""
    subprocess.run(['make', '-C', ROOT, os.path.relpath(PROGRAM, ROOT)],
                   capture_output=True, text=True, timeout=300, check=True)
    out = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'fused host ok' in out.stdout
