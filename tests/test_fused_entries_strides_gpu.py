"""The fused step's forward + loss and data-gradient entry points on rows that lie further
apart than they are wide.

``ga_update_epoch`` lays H1, dZ2 and the weights out at the layers' widths, so no test that
goes through it can tell a leading dimension from a width.  The kernels multiply every
leading dimension into their addresses, though: ``ldh`` into the H1 spill's lane offsets
and buffer extent, ``lddz`` into the dZ2 stores' lane and scalar offsets and extent,
``ldw`` into the lane and scalar offsets of the weight fragments of both k-loops and into
their extents (fused_train.hip, ``GaBuffer``).  The entry points that take them
(``ga_fused_fwd_dgrad``, ``ga_fused_fwd_head_loss``, ``ga_fused_dgrad_wgrad0``) are not part
of the C ABI; ``libgarage_amd_fused_entries.so`` is the library's own objects linked with
one exported wrapper (tests/host/fused_entries_shim.cpp, built by ``make``).

Every case runs the one-launch entry and then the two launches on fresh buffers, with
``ldx``, ``ldh``, ``ldw``, ``lddz``, ``lda`` and the head's ``ldw`` all larger than the
widths and all different.  Every buffer, input or output, lies between guard bands and is
NaN wherever it holds no element: a width in the place of a leading dimension reads a NaN
or leaves an element unwritten, whatever the other path does.  Checked: H1, dZ2 and the
head / loss / first-layer partials carry the same bits on both paths; every element is
finite; every gap between rows, every row beyond M and every guard band still holds NaN;
H1 against ``tanh(X W1^T + b1)`` in fp64 (the two paths share the forward k-loop, so for
H1 they are one implementation, not two).  The bound on H1: the kernel's products are
fp32 chains of ``in_w`` terms plus a bias, ``(in_w + 2) 2^-24 (|X| |W1|^T + |b1|)`` at
most, and ``ga_tanh`` is within 2e-7 of tanh (common.h), doubled for the reference's own
rounding to fp32.

One more case per leading dimension: 2^22 floats or more is refused with an error and
nothing is launched (the kernels hold byte offsets in 32 bits).

(The NaN fills are zeroed at the end of every case: left in freed memory they reach tests
that compare rows nobody wrote.)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64
PAD_ROWS = 3  # rows beyond M in H1 and dZ2

# width, M, in_w, A, gather: every width's kernel (256 with the pipelined and the plain
# forward loop), a lone row, a full tile, ragged last tiles of one to four tiles, the
# three epilogue instantiations (1 = value function, 4, 6), gathered rows and not
CASES = [
    (256, 65, 17, 6, True), (256, 200, 4, 1, False), (256, 1, 20, 4, True),
    (256, 64, 20, 1, False),
    (128, 65, 17, 6, True), (128, 200, 32, 1, False), (128, 1, 4, 4, True),
    (128, 130, 20, 4, False),
    (64, 65, 17, 6, True), (64, 200, 32, 1, False), (64, 1, 4, 4, True),
    (64, 130, 20, 6, False),
]


def _r4(n):
    return (n + 3) & ~3


_SHIM = []


def _shim():
    if not _SHIM:
        from garage_amd import _lib
        _lib.load()
        path = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)),
                            'libgarage_amd_fused_entries.so')
        lib = C.CDLL(path)
        p, i64, i32 = C.c_void_p, C.c_int64, C.c_int
        f = lib.ga_test_fused_fwd_and_dgrad
        f.restype = C.c_int
        f.argtypes = [i32, i64, i32, i32, i32, i32, p, i64, p, p, p, p, i64, p, i64, p, p,
                      i64, p, p, p, i64, p, p, p, p, i64, p, p, p, p]
        lib.ga_test_fused_fwd_dgrad_supported.restype = C.c_int
        lib.ga_test_fused_fwd_dgrad_supported.argtypes = [i32, i32]
        _SHIM.append(lib)
    return _SHIM[0]


class _Rows:
    """``rows`` rows of ``w`` elements, ``ld`` apart, between guard bands; NaN wherever
    there is no element.  ``values``: the elements ([rows][w]), or None for an output."""

    def __init__(self, rows, w, ld, dev, values=None, zero_to=None, dtype=torch.float32):
        self.rows, self.w, self.ld = rows, w, ld
        self.t = torch.full((2 * GUARD + rows * ld, ), NAN, dtype=dtype, device=dev)
        if values is not None:
            v = self.grid()
            if zero_to is not None:  # padding the kernels may read and mask
                v[:, :zero_to] = 0.
            v[:, :w] = values.to(dev)

    def grid(self):
        return self.t[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)

    def ptr(self):
        return self.t.data_ptr() + self.t.element_size() * GUARD

    def snapshot(self):
        return self.t.clone()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class _Problem:
    def __init__(self, case, dev):
        width, M, O, A, gather = case
        self.case, self.dev = case, dev
        rng = np.random.RandomState(7919 * width + 31 * M + 3 * O + A)
        self.kind = 1 if A == 1 else 0
        self.pool = pool = M + 9 if gather else M
        ld0 = _r4(O)
        # all different, all larger than what they hold
        self.ldx, self.ldh, self.ldw = ld0 + 8, width + 8, width + 12
        self.lddz, self.head_ldw, self.lda = width + 4, width + 16, _r4(A) + 4
        self.tiles = (M + 63) // 64
        X = rng.randn(pool, O)
        W1 = rng.randn(width, O) / np.sqrt(O)
        b1 = 0.1 * rng.randn(width)
        W2 = rng.randn(width, width) / np.sqrt(width)
        b2 = 0.1 * rng.randn(width)
        Wh = rng.randn(A, width) / np.sqrt(width)
        bh = 0.1 * rng.randn(A)
        self.X64, self.W164, self.b164 = X, W1, b1
        self.X = _Rows(pool, O, self.ldx, dev, _f32(X), zero_to=ld0)
        self.W1 = _Rows(width, O, ld0, dev, _f32(W1), zero_to=ld0)  # [K][round4(in_w)]
        self.b1 = _Rows(1, width, width, dev, _f32(b1[None]))
        self.W2 = _Rows(width, width, self.ldw, dev, _f32(W2))
        self.b2 = _Rows(1, width, width, dev, _f32(b2[None]))
        self.Wh = _Rows(A, width, self.head_ldw, dev, _f32(Wh))
        self.bh = _Rows(1, A, _r4(A), dev, _f32(bh[None]), zero_to=_r4(A))
        self.log_std = torch.full((1, ), -0.3, dtype=torch.float32, device=dev)
        acts = rng.randn(pool, A)
        self.actions = _Rows(pool, A, self.lda, dev, _f32(acts), zero_to=_r4(A))
        # old log-likelihoods within a few percent of the current ones: PPO ratios inside
        # the clip range, so that the rows carry a gradient
        h = X.astype(np.float32).astype(np.float64)
        for W, b, act in ((W1, b1, True), (W2, b2, True), (Wh, bh, False)):
            h = h @ W.astype(np.float32).astype(np.float64).T + b.astype(np.float32)
            h = np.tanh(h) if act else h
        std = np.exp(-0.3)
        ll = (-0.5 * ((acts.astype(np.float32) - h) / std) ** 2 - np.log(std) -
              0.5 * np.log(2 * np.pi)).sum(1)
        self.old_ll = _f32(ll + 0.05 * rng.randn(pool)).to(dev)
        self.adv = _f32(0.5 + rng.randn(pool)).to(dev)
        self.returns = _f32(h[:, 0] + rng.randn(pool)).to(dev)
        self.idx = None
        if gather:
            self.idx_host = rng.permutation(pool)[:M]
            self.idx = torch.from_numpy(self.idx_host.astype(np.int32)).to(dev)
        else:
            self.idx_host = np.arange(M)
        self.inputs = [self.X, self.W1, self.b1, self.W2, self.b2, self.Wh, self.bh,
                       self.actions]

    def outputs(self):
        width, M, O, A, _ = self.case
        dev = self.dev
        return dict(
            H1=_Rows(M + PAD_ROWS, width, self.ldh, dev),
            dZ2=_Rows(M + PAD_ROWS, width, self.lddz, dev),
            hpart=_Rows(self.tiles, 8 * width + 8, 8 * width + 8, dev),
            lpart=_Rows(self.tiles, 2, 2, dev, dtype=torch.float64),
            wpart=_Rows(self.tiles, width * _r4(O) + width, width * _r4(O) + width, dev))

    def run(self, fused, out, ldh=None, ldw=None, lddz=None):
        from garage_amd import _lib
        width, M, O, A, _ = self.case
        pol = self.kind == 0
        rc = _shim().ga_test_fused_fwd_and_dgrad(
            fused, M, width, O, A, self.kind, self.X.ptr(), self.ldx,
            None if self.idx is None else self.idx.data_ptr(), self.W1.ptr(), self.b1.ptr(),
            out['H1'].ptr(), self.ldh if ldh is None else ldh, self.W2.ptr(),
            self.ldw if ldw is None else ldw, self.b2.ptr(), self.Wh.ptr(), self.head_ldw,
            self.bh.ptr(), self.log_std.data_ptr(),
            self.actions.ptr() if pol else None, self.lda,
            self.old_ll.data_ptr() if pol else None, self.adv.data_ptr() if pol else None,
            None if pol else self.returns.data_ptr(), out['dZ2'].ptr(),
            self.lddz if lddz is None else lddz, out['hpart'].ptr(), out['lpart'].ptr(),
            out['wpart'].ptr(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def zero(self, *outs):
        for r in self.inputs:
            r.t.zero_()
        for out in outs:
            for r in out.values():
                r.t.zero_()
        torch.cuda.synchronize()


def _only_elements_written(name, r, rows_written):
    """Elements of the first ``rows_written`` rows finite, everything else still NaN."""
    g = r.grid()
    assert bool(torch.isfinite(g[:rows_written, :r.w]).all()), name + ': element not finite'
    assert bool(torch.isnan(g[:rows_written, r.w:]).all()), name + ': store between rows'
    assert bool(torch.isnan(g[rows_written:]).all()), name + ': store beyond the last row'
    assert bool(torch.isnan(r.t[:GUARD]).all()) and bool(
        torch.isnan(r.t[GUARD + r.rows * r.ld:]).all()), name + ': store in a guard band'


@pytest.mark.parametrize('case', CASES,
                         ids=lambda c: 'w%d_m%d_in%d_a%d_%s' % (c[:4] + ('idx' if c[4] else
                                                                         'lin', )))
def test_wide_strides_one_launch_against_two(case):
    width, M, O, A, gather = case
    dev = torch.device('cuda', 0)
    assert _shim().ga_test_fused_fwd_dgrad_supported(width, O) == 1
    prob = _Problem(case, dev)
    one, two = prob.outputs(), prob.outputs()
    try:
        before = [r.snapshot() for r in prob.inputs]
        assert prob.run(1, one) == 0
        assert prob.run(0, two) == 0
        for r, b in zip(prob.inputs, before):  # (bits: NaN fills included)
            assert torch.equal(r.t.view(torch.int32), b.view(torch.int32)), 'input written'
        for out in (one, two):
            _only_elements_written('H1', out['H1'], M)
            _only_elements_written('dZ2', out['dZ2'], M)
            for key in ('hpart', 'lpart', 'wpart'):
                _only_elements_written(key, out[key], prob.tiles)
        for key in one:
            a, b = one[key].t, two[key].t
            bits = torch.int32 if a.dtype == torch.float32 else torch.int64
            assert torch.equal(a.view(bits), b.view(bits)), key + ': bits differ'
        assert bool((one['dZ2'].grid()[:M, :width] != 0).any())
        # H1 against fp64
        x = prob.X64.astype(np.float32).astype(np.float64)[prob.idx_host]
        w = prob.W164.astype(np.float32).astype(np.float64)
        b = prob.b164.astype(np.float32).astype(np.float64)
        ref = np.tanh(x @ w.T + b)
        bound = (O + 2) * 2.0 ** -24 * (np.abs(x) @ np.abs(w).T + np.abs(b)) + 4e-7
        got = one['H1'].grid()[:M, :width].double().cpu().numpy()
        frac = float((np.abs(got - ref) / bound).max())
        print('H1 against fp64: largest error / bound = %.3f' % frac)
        assert frac <= 1.0
    finally:
        prob.zero(one, two)


@pytest.mark.parametrize('which', ['ldh', 'ldw', 'lddz'])
def test_leading_dimension_beyond_32_bit_byte_offsets_is_refused(which):
    """2^22 floats: 256 rows of them no longer fit 32-bit byte offsets.  Both entries
    return an error and launch nothing (the buffers are a few KB: a launch would fault, and
    what it wrote would show)."""
    dev = torch.device('cuda', 0)
    prob = _Problem((256, 1, 17, 6, False), dev)
    out = prob.outputs()
    try:
        for fused in (1, 0):
            assert prob.run(fused, out, **{which: 1 << 22}) != 0, (which, fused)
            for r in out.values():
                assert bool(torch.isnan(r.t).all())
        # (one float less is a size these buffers do not have: not launched here)
    finally:
        prob.zero(out)
