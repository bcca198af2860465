"""``ga_policy_step_wide_supported`` (host only): the one-launch rollout step
takes networks whose layer inputs are up to 512 wide; the predicate of the
kernels for widths up to 256 answers as before, and the ABI version stays."""
import ctypes as C

import pytest

from test_rollout_options_cpu import _desc


def _wide(d):
    from garage_amd import _lib
    return int(_lib.load().ga_policy_step_wide_supported(C.byref(d)))


def _narrow(d):
    from garage_amd import _lib
    return int(_lib.load().ga_policy_step_fused_supported(C.byref(d)))


def test_a_257_wide_layer_input_is_wide_only():
    d = _desc((17, 257, 256, 6))
    assert _wide(d) == 1
    assert _narrow(d) == 0


@pytest.mark.parametrize('dims', [
    (512, 512, 512, 32),
    (376, 512, 512, 512, 17),   # C5
    (12, ) + (260, ) * 7 + (4, ),  # eight layers
], ids=['widest', 'c5', 'eight-layers'])
def test_wide_networks_are_supported(dims):
    assert _wide(_desc(dims)) == 1
    assert _narrow(_desc(dims)) == 0


@pytest.mark.parametrize('act', [1, 2, 3, 4, 5, 6])
def test_every_option_of_a_wide_network_is_supported(act):
    dims = (300, 257, 511, 7)
    assert _wide(_desc(dims, hidden_act=act)) == 1
    assert _wide(_desc(dims, output_act=act)) == 1
    assert _wide(_desc(dims, hidden_act=act, layer_norm=1)) == 1


def test_the_limits_of_the_wide_step():
    assert _wide(_desc((513, 64, 6))) == 0
    assert _wide(_desc((17, 512, 513, 6))) == 0
    assert _wide(_desc((17, 512, 512, 33))) == 0  # a 33-wide head
    assert _wide(_desc((17, 512, 512, 32))) == 1
    dims = (17, 512, 512, 6)
    assert _wide(_desc(dims, hidden_act=7)) == 0
    assert _wide(_desc(dims, output_act=7)) == 0
    assert _wide(_desc(dims, hidden_act=-1)) == 0
    assert _wide(_desc(dims, output_act=-1)) == 0
    d = _desc((12, ) + (260, ) * 7 + (4, ))
    d.n_layers = 9  # (dims holds nine entries: the count alone is refused)
    assert _wide(d) == 0
    d.n_layers = 0
    assert _wide(d) == 0


def test_it_is_a_superset_of_the_predicate_for_widths_up_to_256():
    for dims in ((17, 256, 256, 6), (3, 2), (17, 256, 256, 32)):
        assert _narrow(_desc(dims)) == 1
        assert _wide(_desc(dims)) == 1
    d = _desc((17, 256, 256, 6), hidden_act=2, output_act=1, layer_norm=1)
    assert _narrow(d) == 1 and _wide(d) == 1
    # what neither takes
    assert _narrow(_desc((17, 256, 256, 33))) == 0
    assert _wide(_desc((17, 256, 256, 33))) == 0


def test_the_abi_version_is_unchanged():
    from garage_amd import _lib
    assert int(_lib.load().ga_abi_version()) == 5
    assert _lib.ABI_VERSION == 5
