"""The paired-column instantiation of the 128 x 128 weight-gradient GEMM
(gemm.hip: ``gemm_rr_paired_kernel``; ``ga_set_wgrad_paired_columns``) against the one
kernel it stands in for, bit for bit.

The instantiation keeps the tiles, the slabs, the k order per output element and the
column sums of ``gemm_f32_kernel<128, 128, 2, 4, false, false>`` and changes which lane
holds which column, how the slab leaves the registers and how addresses are formed, so
every slab of the weight and the bias gradient must carry the same BITS with the switch
on and off.

``test_slabs_same_bits_through_the_backward_entry`` goes through ``ga_mlp_backward_f32``
with a three-layer network obs 17 -> in_w -> out_w -> 6 actions, whose middle layer is
the product under test (dW = dZ^T H, ``out_w x in_w``, ``slabs`` slabs of the rows).  The
entry lays the activations, their gradients and the layer matrices out at the layers'
widths itself; the leading dimensions it takes from the caller -- ``ldx``, ``ldo`` and the
slab stride -- are all larger than what they hold, NaN fills every gap between rows and
slabs, and guard bands of NaN surround the observations, the output gradient and the
slabs.  The whole slab buffer (NaN fills included) is compared as integers.

====  =====  ====  =====  ========================================================
rows  out_w  in_w  slabs  what it catches
====  =====  ====  =====  ========================================================
256   128    128   1      one tile, one slab
520   256    128   3      slabs of 192, 192 and 136 rows: the last k-step of the
                          last slab holds 8 rows (k-tail masks)
1024  128    256   4      two column tiles
768   256    256   3      the bench's 2 x 2 tile grid
512   384    128   2      three row tiles against one column tile (an m / n swap)
512   192    128   2      does not qualify (192 is no multiple of 128)
====  =====  ====  =====  ========================================================

(The 64 x 64 x 128 tiles that ``ga_set_small_m_gemm`` gives one-slab products come first
in the plan and are switched off here: the first case is about the 128 x 128 tile.)

``ga_wgrad_paired_launches()`` counts the launches of the new instantiation, beside
``ga_launch_count(2)``, which counts the weight-gradient GEMM whichever kernel it takes.

``test_update_epoch_same_bits`` runs two optimizer steps of ``PPO._train_once`` (MLP(256,
256), obs 17, 4096-row minibatches: ``ga_update_epoch``) with the switch on and off:
parameters, gradients and both Adam moments of both networks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64
O, A = 17, 6
KIND_WGRAD = 2

# rows, out_w, in_w, slabs, takes the paired-column instantiation
CASES = [
    (256, 128, 128, 1, True),
    (520, 256, 128, 3, True),
    (1024, 128, 256, 4, True),
    (768, 256, 256, 3, True),
    (512, 384, 128, 2, True),
    (512, 192, 128, 2, False),
]


def _guarded(rows, w, ld, dev, values, zero_to):
    """``rows`` rows of ``w`` values, ``ld`` apart, between guard bands; zeros up to
    ``zero_to`` (padding the kernels may read), NaN everywhere else."""
    t = torch.full((2 * GUARD + rows * ld, ), NAN, dtype=torch.float32, device=dev)
    g = t[GUARD:GUARD + rows * ld].view(rows, ld)
    g[:, :zero_to] = 0.
    g[:, :w] = values.to(dev)
    return t, g


def _counts(lib):
    return [int(lib.ga_launch_count(KIND_WGRAD)), int(lib.ga_wgrad_paired_launches())]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'm%d_out%d_in%d_s%d' % c[:4])
def test_slabs_same_bits_through_the_backward_entry(case):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.engine import FlatMLP
    M, out_w, in_w, n_splits, qualifies = case
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(1009 * M + 7 * out_w + in_w)
    net = FlatMLP(O, A, (in_w, out_w), dev)
    for l in range(3):
        rows, cols = net.dims[l + 1], net.dims[l]
        net.weight(l).copy_(torch.from_numpy(
            (rng.randn(rows, cols) / np.sqrt(cols)).astype(np.float32)))
        net.bias(l).copy_(torch.from_numpy((0.1 * rng.randn(rows)).astype(np.float32)))
    ldx, ldo = 20 + 8, 8 + 4
    slab_stride = net.n_flat + 12
    assert slab_stride % 4 == 0
    Xt, X = _guarded(M, O, ldx, dev, torch.from_numpy(rng.randn(M, O).astype(np.float32)), 20)
    Gt, G = _guarded(M, A, ldo, dev, torch.from_numpy(rng.randn(M, A).astype(np.float32)), 8)
    slabs = {}
    launched = {}
    try:
        lib.ga_set_small_m_gemm(0)
        net.forward(X, M)
        inputs = [Xt.clone(), Gt.clone()]
        for on in (1, 0):
            lib.ga_set_wgrad_paired_columns(on)
            s = torch.full((2 * GUARD + n_splits * slab_stride, ), NAN,
                           dtype=torch.float32, device=dev)
            n0 = _counts(lib)
            call('ga_mlp_backward_f32', C.byref(net._desc), dptr(net.params), dptr(X), ldx,
                 None, M, dptr(net._acts), dptr(G), ldo, dptr(net._dacts),
                 C.c_void_p(s.data_ptr() + 4 * GUARD), slab_stride, n_splits, stream_ptr())
            torch.cuda.synchronize()
            launched[on] = [a - b for a, b in zip(_counts(lib), n0)]
            slabs[on] = s
        # which kernel took the middle layer
        assert launched[1] == [1, 1 if qualifies else 0], launched
        assert launched[0] == [1, 0], launched
        for t, before in zip((Xt, Gt), inputs):
            assert torch.equal(t.view(torch.int32), before.view(torch.int32)), 'input written'
        w0, b0 = net.w_off[1], net.b_off[1]
        for on in (1, 0):
            s = slabs[on]
            assert bool(torch.isnan(s[:GUARD]).all()) and bool(
                torch.isnan(s[GUARD + n_splits * slab_stride:]).all()), 'store in a guard band'
            body = s[GUARD:GUARD + n_splits * slab_stride].view(n_splits, slab_stride)
            assert bool(torch.isnan(body[:, net.n_flat:]).all()), 'store between slabs'
            # the middle layer's slabs: W[out_w][in_w] and b[out_w], every split
            assert bool(torch.isfinite(body[:, w0:w0 + out_w * in_w]).all())
            assert bool(torch.isfinite(body[:, b0:b0 + out_w]).all())
        body = slabs[1][GUARD:GUARD + n_splits * slab_stride].view(n_splits, slab_stride)
        assert bool((body[:, w0:w0 + out_w * in_w] != 0).any(dim=1).all()), 'an empty slab'
        assert torch.equal(slabs[1].view(torch.int32), slabs[0].view(torch.int32)), \
            'slabs differ between the two instantiations'
    finally:
        lib.ga_set_wgrad_paired_columns(1)
        lib.ga_set_small_m_gemm(1)
        # (NaN left in freed memory reaches tests that compare rows nobody wrote)
        for t in [Xt, Gt] + list(slabs.values()):
            t.zero_()
        torch.cuda.synchronize()


def test_update_epoch_same_bits():
    from garage_amd import _lib
    from test_fused_train_gpu import SHAPES, _algo, _problem
    lib = _lib.load()
    SHAPES['wgrad_paired_m4096'] = (O, A, (256, 256), 4096, False, {})
    # 8192 samples: two minibatches of 4096 rows, one epoch = two optimizer steps
    spec, batch = _problem('wgrad_paired_m4096', lens=[40] * 204 + [32])
    opt = (torch.optim.Adam, dict(lr=1e-3))
    state, launched = {}, {}
    try:
        for on in (1, 0):
            lib.ga_set_wgrad_paired_columns(on)
            algo, pol, vf = _algo('wgrad_paired_m4096', spec, opt, epochs=1)
            np.random.seed(11)
            n0 = _counts(lib)
            algo._train_once(0, batch)
            torch.cuda.synchronize()
            launched[on] = [a - b for a, b in zip(_counts(lib), n0)]
            state[on] = [t.clone() for net in (pol.net, vf.net)
                         for t in (net.params, net.grads, net.exp_avg, net.exp_avg_sq)]
    finally:
        lib.ga_set_wgrad_paired_columns(1)
    # every weight-gradient GEMM of the two steps through the new instantiation, or none
    assert launched[1][0] >= 2 and launched[1][1] == launched[1][0], launched
    assert launched[0] == [launched[1][0], 0], launched
    for a, b in zip(state[1], state[0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isfinite(state[1][0]).all())
