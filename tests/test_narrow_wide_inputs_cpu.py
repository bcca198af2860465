"""The shape rule of the narrow step's wide instantiations (33 .. 128 inputs) as the
host entry points apply it, without a GPU: opt-in at the C ABI (``ga_set_narrow_wide``),
what the population's passes then accept and size, which scratch layout -- so which
step -- a lone learner's epoch loop plans, and ``GARAGE_AMD_NARROW_WIDE=0`` in a fresh
process."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from garage_amd import _lib
from garage_amd.engine import FlatMLP, round4

PROG = ('import ctypes as C, torch\nfrom garage_amd import _lib\n'
        'from garage_amd.engine import FlatMLP\n'
        'd = FlatMLP(64, 6, (64, 64), torch.device("cpu"))._desc\n'
        'lib = _lib.load()\nlib.ga_set_narrow_wide(1)\n'
        'print(lib.ga_update_partials_floats(C.byref(d), 129))')


@pytest.mark.parametrize('H', [32, 64])
@pytest.mark.parametrize('in_w,taken', [(32, 1), (33, 1), (128, 1), (129, 0)])
def test_rule_sizes_and_switch(in_w, H, taken):
    lib = _lib.load()
    desc = C.byref(FlatMLP(in_w, 6, (H, H), torch.device('cpu'))._desc)
    # 129 rows: 3 tiles of loss sums and gradient shares
    need = 3 * (4 + H * round4(in_w) + H + H * H + H + 8 * H + 8)
    assert lib.ga_set_narrow_wide(0) == 0  # off unless asked for
    try:
        for on in (0, 1, 0):
            lib.ga_set_narrow_wide(on)
            want = int(taken and (on or in_w <= 32))
            assert lib.ga_update_members_supported(desc) == want
            assert lib.ga_update_members_partials_floats(desc, 5, 129) == 5 * need * want
            assert (lib.ga_update_partials_floats(desc, 129) == need) == bool(want)
    finally:
        assert lib.ga_set_narrow_wide(0) == 0
    if (in_w, H) == (128, 64):  # the environment's veto is read once per process
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        got = [int(subprocess.run(
            [sys.executable, '-c', PROG], capture_output=True, text=True, check=True,
            env=dict(os.environ, GARAGE_AMD_NARROW_WIDE=v, PYTHONPATH=root)).stdout)
            for v in ('1', '0')]
        assert got[0] == 3 * (4 + 64 * 64 + 64 + 64 * 64 + 64 + 8 * 64 + 8) != got[1]
