"""Precondition of ``test_whole_forward_fp64_gpu.py``: on every case of its table, fp32
arithmetic by itself (torch on the CPU) stays within HALF of the tolerance the one-launch
forwards are held to against the fp64 reference, and the table is what it claims: every
evaluation-forward shape is one the library's rule admits, and the shapes meant for the
pipelined instantiation, the LDS bound and the odd k-step counts are those.  A GPU
result outside the tolerance is then the kernel's doing, not the case's.  (No GPU.)"""
import numpy as np
import pytest

import _whole_forward_cases as wc


def test_evaluation_shapes_are_what_the_table_claims():
    for name, (in_w, (K, width), A) in wc.EVAL_SHAPES.items():
        assert K % 32 == 0, name
        assert K * wc.round4(in_w) <= wc.FT_W1_FLOATS, name
        assert width in (128, 256), name
        assert 1 <= A <= 8, name
        assert ((in_w + 3) // 4 == 5) == (name in wc.PIPELINED), name
    assert wc.PIPELINED == ('E1', 'E2', 'E8')
    in_w, (K, _), _ = wc.EVAL_SHAPES['E2']
    assert K * wc.round4(in_w) == wc.FT_W1_FLOATS
    # E7: the next input quad at K = 192 is over the bound
    in_w, (K, _), _ = wc.EVAL_SHAPES['E7']
    assert K * (wc.round4(in_w) + 4) > wc.FT_W1_FLOATS
    # E6: an odd number of 32-deep k-steps
    assert wc.EVAL_SHAPES['E6'][1][0] // 32 % 2 == 1
    # the pipelined instantiation exists at 256 units only
    assert all(wc.EVAL_SHAPES[s][1][1] == 256 for s in wc.PIPELINED)
    assert len(wc.EVAL_CASES) == 45 == len(set(wc.EVAL_CASES))
    assert len(wc.TRAIN_CASES) == 17 == len(set(wc.TRAIN_CASES))


def test_gathered_cases_repeat_rows_and_leave_rows_unnamed():
    for case in wc.CASES:
        if not case[2]:
            continue
        idx = wc.build(case)['row_idx']
        assert idx.shape == (wc.GATHER_M, ) and idx.min() >= 0
        assert idx.max() < wc.GATHER_POOL
        assert len(np.unique(idx)) < wc.GATHER_M, case
        assert len(np.unique(idx)) < wc.GATHER_POOL, case


def test_the_reference_without_a_hidden_layer_is_the_plain_product():
    c = wc.build(('F0', 65, False))
    W = c['params'][wc.PREFIX + '_mean_module._output_layers.0.linear.weight']
    b = c['params'][wc.PREFIX + '_mean_module._output_layers.0.linear.bias']
    assert list(c['ref']) == ['out']
    want = c['X'].double().numpy() @ W.double().numpy().T + b.double().numpy()
    assert np.array_equal(c['ref']['out'], want)


@pytest.mark.parametrize('case', wc.CASES, ids=wc.case_id)
def test_fp32_deviation_is_within_half_the_tolerance(case):
    c = wc.build(case)
    dims = wc.dims_of(case)
    M = case[1]
    n_hidden = len(dims) - 2
    assert list(c['ref']) == ['out'] + ['hidden.%d' % l for l in range(n_hidden)]
    assert len(c['params']) == 2 * (n_hidden + 1)
    assert c['ref']['out'].shape == (M, dims[-1])
    for l in range(n_hidden):
        assert c['ref']['hidden.%d' % l].shape == (M, dims[l + 1])
    worst = []
    for name, ref in c['ref'].items():
        assert np.isfinite(ref).all(), name
        tol = wc.tolerance(name, ref)
        print('WHOLECHK cpu %-10s %-10s dev32 %.3e  tol %.3e  frac %.3f' % (
            wc.case_id(case), name, c['dev32'][name], tol, c['dev32'][name] / tol))
        if not c['dev32'][name] <= 0.5 * tol:
            worst.append((name, c['dev32'][name], tol))
    assert not worst, worst
