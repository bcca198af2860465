"""CPU check of which fused optimizer steps send their forward + loss launch and their
data-gradient launch out as one (``ga_set_fused_fwd_dgrad``)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_sequence_of_the_fused_forward_and_data_gradient_under_address_sanitizer():
    """``make asan-fwd-dgrad``: ``fused_step`` / ``run_minibatch_fused`` (update.cpp)
    compiled with ``-fsanitize=address,undefined`` for the CPU and run against fakes of
    every launch, with a kernel side that has the fused instantiation
    (tests/host/update_loop_harness.cpp, suite fwd-dgrad).  A step of one network with two hidden
    layers of the same width and a first layer the kernel computes is exactly: fused
    launch, middle-layer weight-gradient GEMM, optimizer launch, on one stream; the
    fused launch's two descriptors are one step's and carry no slab ranges; the
    optimizer launch gets no pre-summed region and reads the middle layer's regions as
    ``splits`` partials inside the slab workspace (the fake walks them).  The
    four-launch sequence comes back with the switch off, in the merged pair schedule,
    with one or three hidden layers, with hidden layers of different widths and with a
    first layer the kernel does not compute."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-fwd-dgrad'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'fused fwd dgrad ok' in out.stdout
