"""``ga_policy_step_fused_supported`` (host only): the one-launch rollout step
takes every nonlinearity ``ga_mlp_desc`` can name and ``layer_norm``; the width
limits are what they were."""
import ctypes as C

import pytest


def _desc(dims, hidden_act=0, output_act=0, layer_norm=0):
    """A ``ga_mlp_desc`` filled by hand with FlatMLP's layout."""
    from garage_amd import _lib

    def round4(v):
        return (v + 3) // 4 * 4

    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    off = 4
    for i, v in enumerate(dims):
        d.dims[i] = v
    for l in range(len(dims) - 1):
        d.w_off[l] = off
        off += dims[l + 1] * round4(dims[l])
        d.b_off[l] = off
        off += round4(dims[l + 1])
    d.hidden_act, d.output_act, d.layer_norm = hidden_act, output_act, layer_norm
    if layer_norm:
        for l in range(len(dims) - 2):
            d.ln_off[l] = off
            off += 2 * round4(dims[l])
    return d


def _supported(d):
    from garage_amd import _lib
    return int(_lib.load().ga_policy_step_fused_supported(C.byref(d)))


DIMS = (17, 256, 256, 6)


def test_the_tanh_linear_shape_is_still_supported():
    assert _supported(_desc(DIMS)) == 1
    assert _supported(_desc((3, 2))) == 1


@pytest.mark.parametrize('act', [1, 2, 3, 4, 5, 6])
def test_every_hidden_nonlinearity_is_supported(act):
    assert _supported(_desc(DIMS, hidden_act=act)) == 1


@pytest.mark.parametrize('act', [1, 2, 3, 4, 5, 6])
def test_every_output_nonlinearity_is_supported(act):
    assert _supported(_desc(DIMS, output_act=act)) == 1


def test_layer_norm_is_supported():
    assert _supported(_desc(DIMS, layer_norm=1)) == 1
    assert _supported(_desc(DIMS, hidden_act=1, output_act=1, layer_norm=1)) == 1


def test_the_limits_are_what_they_were():
    assert _supported(_desc((17, 257, 256, 6))) == 0   # a 257-wide layer input
    assert _supported(_desc((17, 256, 257, 6))) == 0
    assert _supported(_desc((257, 64, 6))) == 0
    assert _supported(_desc((17, 256, 256, 33))) == 0  # a 33-wide head
    assert _supported(_desc((17, 256, 256, 32))) == 1
    assert _supported(_desc(DIMS, hidden_act=7)) == 0
    assert _supported(_desc(DIMS, output_act=7)) == 0
    assert _supported(_desc(DIMS, hidden_act=-1)) == 0
    assert _supported(_desc(DIMS, hidden_act=1, layer_norm=1,
                            output_act=7)) == 0
