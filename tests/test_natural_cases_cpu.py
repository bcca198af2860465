"""The yardstick of tests/_natural_cases.py: plain fp32 torch stays within HALF of every
tolerance the GPU tests hold the population's natural-gradient kernels to (the project's
rule, as tests/test_loss_cases_cpu.py)."""
import pytest
import torch

from _natural_cases import CASES, TOL, fvp, gradient, make_case, rel_err


@pytest.mark.parametrize('i', range(len(CASES)))
def test_fp32_torch_is_within_half_of_the_tolerances(i):
    case = CASES[i]
    t = make_case(case, i)
    want = fvp(case, t, t['vec'])
    got = fvp(case, t, t['vec'], dtype=torch.float32)
    loss64, grad64 = gradient(case, t)
    loss32, grad32 = gradient(case, t, dtype=torch.float32)
    errs = dict(fvp=rel_err(got, want), grad=rel_err(grad32, grad64),
                loss=abs(float(loss32) - float(loss64)))
    print('natural case', i, case, errs)
    for k, e in errs.items():
        assert e <= 0.5 * TOL[k], (k, e)
