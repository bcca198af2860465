"""CPU check of which fused optimizer steps hand the middle layer's split-K slabs to
their data-gradient launch (``ga_set_slab_sum_in_dgrad``)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_ranges_of_the_fused_step_under_address_sanitizer():
    """``make asan-slab-sum``: ``fused_step`` (update.cpp) compiled with
    ``-fsanitize=address,undefined`` for the CPU and run against fakes of every launch
    (tests/host/update_loop_harness.cpp, suite slab-sum).  The data-gradient launch gets slab ranges
    exactly when the step has that launch, two hidden layers, more than one split and
    the switch is on -- one network per launch and the merged pair schedule alike --;
    the ranges lie inside ``[slabs, slabs + splits * n_flat)`` (the fake walks them in a
    workspace of exactly that size); the weight-gradient launch is the one right before
    on the same stream; the optimizer launch's pre-summed regions are the middle
    layer's two and no others; with the switch off every new field is null or zero."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-slab-sum'], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'slab sum ok' in out.stdout
