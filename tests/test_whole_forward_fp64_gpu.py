"""The whole-network forwards that run in ONE launch against an fp64 reference of the same
network, at row counts from one row to three 64-row tiles:

  ``mlp_eval_forward_kernel`` (fused_train.hip, the EVAL arm of ``fwd_head_loss_body``),
  reached through ``ga_mlp_forward_f32(..., acts = NULL, ...)``: the 128-unit, the plain
  256-unit and the pipelined 256-unit instantiations (and the split-operand one, below);
  ``mlp_train_fwd_fused_kernel`` (policy_fused.hip), reached through
  ``ga_mlp_forward_fused_f32``: outputs and every stored hidden activation.

Cases, reference and tolerance: ``tests/_whole_forward_cases.py``; that fp32 itself is
within half the tolerance on every case: ``test_whole_forward_cases_cpu.py``.  Every
launch is compared with the reference, never with another kernel of the library, and
everything around what it may write is poisoned: NaN in the input's padding columns and
in the pool rows no index names, one sentinel bit pattern in every element of the output
buffer (the rows behind the last one and the padding columns must keep it), 7.0 or NaN in
the activation workspace.

Split-operand mode.  When the suite runs with ``GARAGE_AMD_SPLIT_BF16=1`` the shapes with
256 units and at most 20 inputs take ``mlp_eval_forward_split_kernel``.  Its bound is
``(TOL_FORWARD + 2e-6) * max(1, max |ref|)``: the 2e-6 is the bar
``test_split_evaluation_forward_matches_the_exact_one`` sets between the split and the
exact kernel.  The pipelined loop is then not taken at all (the split loop comes first in
the host's choice), so the bit comparison of the pipelined with the plain loop would
compare a launch with itself: it is skipped in that mode.  The library has no query for
the mode in its C ABI and other modules switch it off when they are done, so the
environment only widens the bound; ``test_split_evaluation_forward_matches_fp64`` switches
the mode on itself and runs in every mode of the suite.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _whole_forward_cases as wc

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = 0x7FC0BEEF   # a quiet NaN no kernel produces
EVAL_KIND = 12          # prof.h: GA_PROF_EVAL_FWD
SPLIT_EXTRA = 2e-6
SPLIT_ENV = os.environ.get('GARAGE_AMD_SPLIT_BF16') == '1'


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


@pytest.fixture(scope='module')
def lib():
    from garage_amd import _lib
    return _lib.load()


def _split_shape(shape):
    """Does the split-operand instantiation take this evaluation shape?"""
    in_w, (K, width), _ = wc.EVAL_SHAPES[shape]
    return width == 256 and in_w <= 20 and K % 32 == 0


def _network(dims, c, dev, **options):
    """A FlatMLP of ``dims`` with the case's parameters; the padding columns of the
    weights stay zero (the layout contract)."""
    from garage_amd.engine import FlatMLP
    net = FlatMLP(dims[0], dims[-1], dims[1:-1], dev, **options)
    net.params.zero_()
    if c is not None:
        for key, view in net.named_views():
            if key != '_init_std':
                view.copy_(c['params'][wc.PREFIX + key].to(dev).reshape(view.shape))
    return net


def _poisoned_rows(c, dev):
    """The row pool with ldx = round4(in_w) + 4: NaN in every column >= in_w and in every
    row no index names.  -> (X, idx)"""
    Xh = c['X']
    pool, in_w = Xh.shape
    X = torch.full((pool, wc.round4(in_w) + 4), NAN, dtype=torch.float32, device=dev)
    X[:, :in_w] = Xh.to(dev)
    idx = None
    if c['row_idx'] is not None:
        named = np.zeros(pool, dtype=bool)
        named[c['row_idx']] = True
        assert not named.all()
        X[torch.from_numpy(~named).to(dev)] = NAN
        idx = torch.from_numpy(c['row_idx']).to(dev)
    return X, idx


def _sentinel_out(M, A, dev):
    """M + 64 rows of ldo = round4(A) + 4 floats, every element the sentinel."""
    bits = torch.full((M + wc.FT_ROWS, wc.round4(A) + 4), SENTINEL, dtype=torch.int32,
                      device=dev)
    return bits.view(torch.float32)


def _only_live_elements_written(out, M, A):
    """Columns A .. ldo - 1 of the live rows and all rows >= M still hold the sentinel."""
    bits = out.view(torch.int32).clone()
    bits[:M, :A] = SENTINEL
    return bool((bits == SENTINEL).all())


def _check(got, c, name, failures, kernel, where, extra=0.0):
    ref = c['ref'][name]
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    tol = wc.tolerance(name, ref)
    bound = tol + extra * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float('inf')
    print('WHOLECHK %-18s %-22s %-10s err %.3e  tol %.3e  frac %.3f  dev32 %.3e' % (
        kernel, where, name, err, bound, err / bound, c['dev32'][name]))
    if not err <= bound:
        failures.append((kernel, where, name, err, bound))


def _eval_forward(lib, net, X, idx, M, out):
    """``ga_mlp_forward_f32`` with ``acts = NULL``; the launch count must rise by one."""
    from garage_amd._lib import call, dptr, stream_ptr
    n0 = int(lib.ga_launch_count(EVAL_KIND))
    call('ga_mlp_forward_f32', C.byref(net._desc), dptr(net.params), dptr(X),
         X.stride(0), dptr(idx), M, None, dptr(out), out.stride(0), stream_ptr())
    torch.cuda.synchronize()
    return int(lib.ga_launch_count(EVAL_KIND)) - n0


def _eval_case(lib, dev, case, kernel, failures, extra=0.0):
    """One launch of the evaluation forward on ``case`` with everything around it
    poisoned -> the output buffer."""
    c = wc.build(case)
    shape, M, _ = case
    A = wc.dims_of(case)[-1]
    net = _network(wc.dims_of(case), c, dev)
    assert lib.ga_mlp_forward_eval_supported(C.byref(net._desc)) == 1
    X, idx = _poisoned_rows(c, dev)
    net._workspace(M + wc.FT_ROWS)
    net._acts.fill_(7.0)
    out = _sentinel_out(M, A, dev)
    assert _eval_forward(lib, net, X, idx, M, out) == 1
    assert torch.equal(net._acts, torch.full_like(net._acts, 7.0))
    assert torch.isfinite(out[:M, :A]).all()
    _check(out[:M, :A], c, 'out', failures, kernel, wc.case_id(case), extra)
    assert _only_live_elements_written(out, M, A), \
        'the launch wrote outside out[:M, :A] (%s)' % wc.case_id(case)
    return out


# ---- a. the evaluation forward ----------------------------------------------------------
@pytest.mark.parametrize('case', wc.EVAL_CASES, ids=wc.case_id)
def test_evaluation_forward_matches_fp64(dev, lib, case):
    shape = case[0]
    width = wc.EVAL_SHAPES[shape][1][1]
    split = SPLIT_ENV and _split_shape(shape)
    extra = SPLIT_EXTRA if split else 0.0
    failures = []
    if shape not in wc.PIPELINED:
        kernel = 'eval 256 split' if split else 'eval %d%s' % (
            width, ' plain' if width == 256 else '')
        _eval_case(lib, dev, case, kernel, failures, extra)
    else:
        outs = []
        try:
            for on in (1, 0):
                lib.ga_set_pipelined_kloop(on)
                kernel = 'eval 256 split' if split else (
                    'eval 256 pipelined' if on else 'eval 256 plain')
                outs.append(_eval_case(lib, dev, case, kernel, failures, extra))
        finally:
            lib.ga_set_pipelined_kloop(1)
        if not split:
            # the same k order per output element: the same bits, ragged tiles included
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert not failures, failures


@pytest.mark.parametrize('case', [c for c in wc.EVAL_CASES if _split_shape(c[0])],
                         ids=wc.case_id)
def test_split_evaluation_forward_matches_fp64(dev, lib, case):
    """``mlp_eval_forward_split_kernel``, switched on here whatever the suite's mode."""
    failures = []
    lib.ga_set_split_bf16(1)
    try:
        _eval_case(lib, dev, case, 'eval 256 split', failures, SPLIT_EXTRA)
    finally:
        lib.ga_set_split_bf16(1 if SPLIT_ENV else 0)
    assert not failures, failures


# ---- b. the rule's neighbours are refused, and the switch works -----------------------------
REFUSED = [
    ((25, 192, 256, 2), {}),     # over the LDS bound
    ((33, 128, 128, 3), {}),     # more than 32 inputs
    ((17, 256, 256, 9), {}),     # more than 8 outputs
    ((17, 96, 128, 3), {}),      # a width below 128
    ((17, 128, 64, 3), {}),
    ((17, 144, 128, 3), {}),     # K % 32 != 0
    ((17, 256, 256, 6), dict(hidden_act='relu')),
    ((17, 256, 256, 6), dict(output_act='tanh')),
    ((17, 256, 256, 6), dict(layer_norm=True)),
]


def _refused(lib, net, dev, M=65):
    """``acts = NULL`` on a network the evaluation forward does not take: the entry
    raises before anything is launched."""
    from garage_amd._lib import GarageAmdError
    in_w, A = net.dims[0], net.dims[-1]
    net._workspace(M)
    X = torch.ones(M, wc.round4(in_w) + 4, device=dev)
    out = _sentinel_out(M, A, dev)
    n0 = int(lib.ga_launch_count(EVAL_KIND))
    with pytest.raises(GarageAmdError, match='acts workspace needed'):
        _eval_forward(lib, net, X, None, M, out)
    torch.cuda.synchronize()
    assert int(lib.ga_launch_count(EVAL_KIND)) == n0
    assert bool((out.view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize('dims,options', REFUSED,
                         ids=['-'.join(map(str, d)) + ''.join('-%s' % v for v in o.values())
                              for d, o in REFUSED])
def test_neighbours_of_the_evaluation_rule_are_refused(dev, lib, dims, options):
    net = _network(dims, None, dev, **options)
    assert lib.ga_mlp_forward_eval_supported(C.byref(net._desc)) == 0
    _refused(lib, net, dev)


def test_evaluation_forward_switch(dev, lib):
    """``ga_set_eval_forward(0)``: the rule answers 0, the direct call is refused, and
    ``FlatMLP.forward(keep_acts=False)`` at its row threshold takes the per-layer kernels
    (no launch of the evaluation forward) with the same values to the tolerance; back at
    1 the same call is one launch of it."""
    from garage_amd.engine import FlatMLP, pad_rows
    case = wc.SWITCH_CASE
    c = wc.build(case)
    M, A = case[1], wc.dims_of(case)[-1]
    assert M == FlatMLP.EVAL_MIN_ROWS and c['row_idx'] is None
    net = _network(wc.dims_of(case), c, dev)
    X = pad_rows(c['X'])
    failures = []
    try:
        lib.ga_set_eval_forward(0)
        assert lib.ga_mlp_forward_eval_supported(C.byref(net._desc)) == 0
        _refused(lib, net, dev)
        n0 = int(lib.ga_launch_count(EVAL_KIND))
        out = net.forward(X, M, keep_acts=False)
        torch.cuda.synchronize()
        assert int(lib.ga_launch_count(EVAL_KIND)) == n0
        _check(out[:, :A], c, 'out', failures, 'per-layer', 'eval_forward(0)')
        lib.ga_set_eval_forward(1)
        assert lib.ga_mlp_forward_eval_supported(C.byref(net._desc)) == 1
        net.out_view(M).fill_(NAN)
        out = net.forward(X, M, keep_acts=False)
        torch.cuda.synchronize()
        assert int(lib.ga_launch_count(EVAL_KIND)) == n0 + 1
        _check(out[:, :A], c, 'out', failures,
               'eval 256 split' if SPLIT_ENV else 'eval 256 pipelined', 'eval_forward(1)',
               SPLIT_EXTRA if SPLIT_ENV else 0.0)
    finally:
        lib.ga_set_eval_forward(1)
    assert not failures, failures


# ---- c. the fused training forward ---------------------------------------------------------
@pytest.mark.parametrize('case', wc.TRAIN_CASES, ids=wc.case_id)
def test_fused_training_forward_matches_fp64(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c = wc.build(case)
    M, dims = case[1], wc.dims_of(case)
    A = dims[-1]
    net = _network(dims, c, dev)
    X, idx = _poisoned_rows(c, dev)
    cap = M + wc.FT_ROWS
    net._workspace(cap)
    assert net._cap == cap
    net._acts.fill_(NAN)
    out = _sentinel_out(M, A, dev)
    # (without a hidden layer there is no activation to keep: acts = NULL)
    acts = net._acts if net.hidden_sizes else None
    call('ga_mlp_forward_fused_f32', C.byref(net._desc), dptr(net.params), dptr(X),
         X.stride(0), dptr(idx), M, dptr(acts), dptr(out), out.stride(0), stream_ptr())
    torch.cuda.synchronize()
    failures = []
    where = wc.case_id(case)
    _check(out[:M, :A], c, 'out', failures, 'train forward', where)
    assert _only_live_elements_written(out, M, A), \
        'the launch wrote outside out[:M, :A] (%s)' % where
    for l, width in enumerate(net.hidden_sizes):
        ldh = wc.round4(width)
        off = net.act_off[l] * cap
        block = net._acts[off:off + cap * ldh].view(cap, ldh)
        _check(block[:M, :width], c, 'hidden.%d' % l, failures, 'train forward', where)
        assert torch.isnan(block[M:]).all(), (l, 'rows >= M of the workspace written')
    assert not failures, failures
