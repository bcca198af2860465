"""The host rules on either side of ``ga_set_narrow_acts``; the Python flag's round trip."""
import ctypes as C

import pytest
import torch

# FlatMLP keywords, hidden_act code to force -> (narrow step, members) off and on
CASES = [(dict(), None, (True, True), (True, True)),
         (dict(hidden_act='relu'), None, (False, False), (True, True)),
         (dict(hidden_act='softplus'), None, (False, False), (True, True)),
         (dict(), 7, (False, False), (False, False)),
         (dict(hidden_act='relu', output_act='tanh'), None, (False, False), (False, False)),
         (dict(hidden_act='elu', layer_norm=True), None, (False, False), (False, False))]


@pytest.mark.parametrize('kw, code, off, on', CASES)
def test_rules_on_either_side_of_the_switch(kw, code, off, on):
    from garage_amd import _lib
    from garage_amd.engine import FlatMLP
    lib = _lib.load()
    net = FlatMLP(4, 2, (64, 64), torch.device('cpu'), **kw)
    if code is not None:
        net._desc.hidden_act = code
    d = C.byref(net._desc)
    for setting, want in ((0, off), (1, on), (0, off)):  # (ends with the default)
        lib.ga_set_narrow_acts(setting)
        assert lib.ga_narrow_acts_on() == setting
        assert (lib.ga_update_partials_floats(d, 65) > 0,
                bool(lib.ga_update_members_supported(d))) == want


def test_flag_round_trip():
    from garage_amd import _lib, engine
    on = _lib.narrow_wide_scope(_lib.load().ga_narrow_acts_on)
    assert engine.set_narrow_activations(True) is False and _lib.NARROW_ACTS is True
    try:
        assert on() == 1 and _lib.load().ga_narrow_acts_on() == 0  # (put back)
    finally:
        assert engine.set_narrow_activations(False) is True
    assert on() == 0
