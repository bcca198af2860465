"""Precondition of ``test_mlp_options_fp64_gpu.py``: on every case of its table, fp32
arithmetic by itself (torch on the CPU) stays within HALF of the tolerance the HIP
kernels are held to against the fp64 reference, and the kink resampling of the relu /
leaky_relu cases terminates.  A GPU result outside the tolerance is then the
kernel's doing, not the case's.  (No GPU.)"""
import numpy as np
import pytest

import _mlp_option_cases as oc


def test_table_covers_what_it_claims():
    from garage_amd.engine import FlatMLP
    assert [FlatMLP.HIDDEN_ACTS[k] for k in oc.HIDDEN_ACTS] == list(range(7))
    assert [FlatMLP.OUTPUT_ACTS[k] for k in oc.OUTPUT_ACTS] == list(range(7))
    for shape in ('S2', 'S3', 'S4'):
        opts = [c for c in oc.OPTIONS if c[0] == shape]
        assert {(c[1], c[3]) for c in opts} == {(h, ln) for h in oc.HIDDEN_ACTS
                                                for ln in (False, True)}
        for ln in (False, True):
            assert {c[2] for c in opts if c[3] == ln} == set(oc.OUTPUT_ACTS)
    for shape, ln in (('S1', True), ('S5', True), ('S6', False)):
        opts = [c for c in oc.OPTIONS if c[0] == shape]
        assert [c[1] for c in opts] == ['tanh', 'relu', 'softplus']
        assert all(c[3] == ln for c in opts)
    assert len(oc.CASES) == len(oc.OPTIONS) * len(oc.ROWS) == len(set(oc.CASES))


@pytest.mark.parametrize('case', oc.CASES + [oc.ABI_CASE], ids=oc.case_id)
def test_fp32_deviation_is_within_half_the_tolerance(case):
    c = oc.build(case)
    assert c['kink_rounds'] <= oc.KINK_ROUNDS
    dims = oc.dims_of(case)
    n_hidden = len(dims) - 2
    want = {'out', 'jv'} | {'hidden.%d' % l for l in range(n_hidden)} | {
        'grad.' + k[len(oc.PREFIX):] for k in c['params']}
    assert set(c['ref']) == want
    assert len(c['params']) == 2 * (n_hidden + 1) + (2 * n_hidden if case[3] else 0)
    if case[3]:  # the all-zero row of a LayerNorm case is among the rows used
        X = c['X'] if c['row_idx'] is None else c['X'][c['row_idx'].astype(np.int64)]
        assert (X.abs().sum(dim=1) == 0).any()
    worst = []
    for name, ref in c['ref'].items():
        assert np.isfinite(ref).all(), name
        tol = oc.tolerance(name, ref)
        print('%-60s dev32 %.3e  tol %.3e' % (name, c['dev32'][name], tol))
        if not c['dev32'][name] <= 0.5 * tol:
            worst.append((name, c['dev32'][name], tol))
    assert not worst, worst
