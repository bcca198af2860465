"""CPU check of the host side of the stand-alone loss, statistics and optimizer kernels
(losses_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, 'garage_amd', '_C', 'losses_host_asan_test')


def test_host_side_of_the_loss_entries_under_address_sanitizer():
    """Every entry point of losses_host.cpp, compiled with
    ``-fsanitize=address,undefined`` for the CPU and run as a stand-alone program
    against fakes of the launch seam (tests/host/losses_host_harness.cpp): every fake
    touches what its kernel would in exactly-sized buffers; the refusals and their
    messages (each before any launch), the grids, one launch or two and the ticket's
    place in the workspace, the parameter structs field by field, the head kernels'
    LDS bytes and the optimizer coefficients are literal tables."""
    subprocess.run(['make', '-C', ROOT, os.path.relpath(PROGRAM, ROOT)],
                   capture_output=True, text=True, timeout=300, check=True)
    out = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'losses host ok' in out.stdout
