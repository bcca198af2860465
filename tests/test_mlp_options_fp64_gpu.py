"""Every MLP option of the per-layer passes -- hidden and output nonlinearities,
layer_normalization, narrow / wide / deep / ragged nets, gathered rows -- against fp64
autograd: outputs, hidden activations, every gradient (LayerNorm weight and bias
included) and the tangent pass ``ga_mlp_jvp_f32``.

Cases, reference and tolerances: ``tests/_mlp_option_cases.py``; that fp32 itself is
within half the tolerance on every case: ``test_mlp_option_cases_cpu.py``.  Each case
runs at every position of the dispatch's developer switches and each position is
compared with the reference, never with another position.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _mlp_option_cases as oc

pytestmark = pytest.mark.gpu

NAN = float('nan')

# (small_m, skinny, fused_head_forward, fused_head_dgrad); the first row is the defaults
SWITCHES = [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 2, 1), (0, 1, 2, 1)]


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


def _set_switches(lib, pos):
    small_m, skinny, head_forward, head_dgrad = pos
    lib.ga_set_small_m_gemm(small_m)
    lib.ga_set_skinny_kernels(skinny)
    lib.ga_set_fused_head_forward(head_forward)
    lib.ga_set_fused_head_dgrad(head_dgrad)


def _network(case, c, dev):
    """The case's FlatMLP with its parameters, the flat tangent (padding zero) and the
    device inputs."""
    from garage_amd.engine import FlatMLP, pad_rows
    dims = oc.dims_of(case)
    mlp = FlatMLP(dims[0], dims[-1], dims[1:-1], dev, hidden_act=case[1],
                  output_act=case[2], layer_norm=case[3])
    mlp.params.zero_()
    tangent = torch.zeros_like(mlp.params)
    for buf, src in ((mlp.params, c['params']), (tangent, c['tangent'])):
        for key, view in mlp.named_views(buf):
            if key != '_init_std':
                view.copy_(src[oc.PREFIX + key].to(dev).reshape(view.shape))
    X = pad_rows(c['X'])
    idx = None if c['row_idx'] is None else torch.from_numpy(c['row_idx']).to(dev)
    return mlp, tangent, X, idx


def _poison_slabs(mlp, slabs, n_splits):
    """NaN into every valid element of every slab (the log-std slot, which the loss
    kernels own, and the padding excepted): an element the backward pass fails to
    write shows up in the reduced gradient."""
    for s in range(n_splits):
        slab = slabs[s * mlp.n_flat:(s + 1) * mlp.n_flat]
        for key, view in mlp.named_views(slab):
            if key != '_init_std':
                view.fill_(NAN)


def _check(got, c, name, failures, where):
    ref = c['ref'][name]
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    tol = oc.tolerance(name, ref)
    err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float('inf')
    print('%-14s %-58s err %.3e  tol %.3e  dev32 %.3e' % (where, name, err, tol,
                                                          c['dev32'][name]))
    if not err <= tol:
        failures.append((where, name, err, tol))


@pytest.mark.parametrize('case', oc.CASES, ids=oc.case_id)
def test_mlp_options_match_fp64_autograd(dev, case):
    from garage_amd import _lib
    lib = _lib.load()
    c = oc.build(case)
    M, A = case[4], oc.dims_of(case)[-1]
    mlp, tangent, X, idx = _network(case, c, dev)
    G = c['G'].to(dev)
    failures = []
    try:
        for pos in SWITCHES:
            _set_switches(lib, pos)
            where = 'switches %d%d%d%d' % pos
            # ---- forward: outputs and every hidden layer's block of the workspace
            mlp._workspace(M)
            mlp._acts.fill_(NAN)
            mlp.out_view(M).fill_(NAN)
            out = mlp.forward(X, M, row_idx=idx)
            _check(out[:, :A], c, 'out', failures, where)
            for l, width in enumerate(mlp.hidden_sizes):
                ldh = (width + 3) // 4 * 4
                off = mlp.act_off[l] * mlp._cap
                h = mlp._acts[off:off + M * ldh].view(M, ldh)
                _check(h[:, :width], c, 'hidden.%d' % l, failures, where)
            # ---- backward of sum(out * G): padding columns of dout must not be read,
            # every valid slab element must be written
            dout = mlp.dout_view(M)
            dout.fill_(NAN)
            dout[:, :A] = G
            _poison_slabs(mlp, mlp._slabs, mlp._splits)
            mlp.grads.fill_(NAN)
            mlp.backward(X, M, dout, row_idx=idx)
            mlp.reduce_grads()
            for key, view in mlp.named_views(mlp.grads):
                if key != '_init_std':
                    _check(view, c, 'grad.' + key, failures, where)
            # ---- tangent of the outputs (after a forward at the same rows)
            mlp._tout = torch.full((mlp._cap * mlp.ld_out, ), NAN, device=dev)
            tout = mlp.jvp(X, M, tangent, row_idx=idx)
            _check(tout[:, :A], c, 'jv', failures, where)
    finally:
        _set_switches(lib, SWITCHES[0])
    torch.cuda.synchronize()
    assert not failures, failures


def test_backward_abi_with_more_splits_than_rows_fill(dev):
    """``ga_mlp_backward_f32`` lets the caller choose ``n_splits``: 8 splits over 100
    rows are 32 rows each, so splits 4 .. 7 hold no row.  Their slabs must come back
    as zeros in every valid element, and the sum of all 8 is the gradient."""
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    case = oc.ABI_CASE
    c = oc.build(case)
    M, A, n_splits = case[4], oc.dims_of(case)[-1], 8
    mlp, _, X, idx = _network(case, c, dev)
    assert idx is None
    mlp.forward(X, M)
    dout = mlp.dout_view(M)
    dout.fill_(NAN)
    dout[:, :A] = c['G'].to(dev)
    slabs = torch.zeros(n_splits * mlp.n_flat, dtype=torch.float32, device=dev)
    _poison_slabs(mlp, slabs, n_splits)
    call('ga_mlp_backward_f32', C.byref(mlp._desc), dptr(mlp.params), dptr(X),
         X.stride(0), None, M, dptr(mlp._acts), dptr(dout), dout.stride(0),
         dptr(mlp._dacts), dptr(slabs), mlp.n_flat, n_splits, stream_ptr())
    for s in range(n_splits):
        slab = slabs[s * mlp.n_flat:(s + 1) * mlp.n_flat]
        for key, view in mlp.named_views(slab):
            if key == '_init_std':
                continue
            assert torch.isfinite(view).all(), (s, key)
            if s * 32 >= M:
                assert not view.any(), (s, key)
    mlp.grads.fill_(NAN)
    call('ga_reduce_slabs_f32', dptr(slabs), n_splits, mlp.n_flat, mlp.n_flat, 1.0,
         dptr(mlp.grads), stream_ptr())
    failures = []
    for key, view in mlp.named_views(mlp.grads):
        if key != '_init_std':
            _check(view, c, 'grad.' + key, failures, 'n_splits 8')
    assert not failures, failures
