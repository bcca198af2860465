"""The population's natural-gradient kernels at 33 .. 128 inputs (the wide kernel of
``members_natural.hip``) against fp64 torch autograd (tests/_natural_cases.py).  The range
is opt-in at the C ABI, so every call runs under ``ga_set_narrow_wide(1)``."""
import contextlib

import pytest
import torch

from _natural_cases import HEADS, fvp, gradient, mean_kl, rel_err, surrogate
from test_members_natural_gpu import Population

pytestmark = pytest.mark.gpu

_H = (32, 64)
_IN = (33, 64, 65, 111, 128)  # both sides of NS_LDX = 68 | 132, no multiples of 4 or 8, the end
_OUT = (1, 6, 8)
_S = (1, 31, 33, 64, 65, 200, 1094)  # both sides of a 32- and a 64-row tile, ragged, > 16 tiles
CASES = [(_H[i % 2], _IN[(i // 2) % 5], _OUT[(i // 3) % 3], HEADS[i % 5],
          _S[(i // 5 + i) % 7]) for i in range(30)]
# Twice the largest error of plain fp32 torch against fp64 torch over CASES (seed 100 + i),
# measured on the CPU: product 4.45e-7 (case 27), gradient 2.19e-6 (case 5), loss 1.58e-7
# (case 15; absolute)
TOL = dict(fvp=8.9e-7, grad=4.4e-6, loss=3.2e-7)


@contextlib.contextmanager
def _wide():
    from garage_amd import _lib
    was = _lib.load().ga_set_narrow_wide(1)
    try:
        yield
    finally:
        _lib.load().ga_set_narrow_wide(was)


class WidePopulation(Population):
    def __init__(self, *args, **kw):
        with _wide():
            super().__init__(*args, **kw)

    def call(self, name, *more):
        with _wide():
            super().call(name, *more)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('i', range(len(CASES)))
def test_wide_product_and_gradient_against_fp64_autograd(i):
    case = CASES[i]
    pop = WidePopulation([(case, 100 + i)], cg_iters=0)
    lib = pop.lib.load()
    t = pop.data[0]['t']
    before = int(lib.ga_narrow_wide_launches())
    pop.call('ga_members_natural_fvp')  # (checks the guards behind the workspace)
    e_fvp = rel_err(pop.product(0), fvp(case, t, t['vec']))  # (and around the product)
    pop.call('ga_members_natural_solve')
    assert int(lib.ga_narrow_wide_launches()) - before == 3  # product, gradient, x's product
    loss, grad = gradient(case, t)
    e_grad = rel_err(pop.vector(0, 0), grad)
    e_loss = abs(pop.scalars(0)[3] - float(loss))
    print('natural wide case', i, case, dict(fvp=e_fvp, grad=e_grad, loss=e_loss))
    assert e_fvp <= TOL['fvp'] and e_grad <= TOL['grad'] and e_loss <= TOL['loss']


@pytest.mark.parametrize('head', ['gauss', 'cat_double'])
def test_a_wide_member_gets_the_same_bits_whatever_the_population(head):
    members = [((64, 111, 6, head, S), seed) for S, seed in ((1094, 1), (65, 2), (200, 3))]
    pop = WidePopulation(members, cg_iters=0)
    pop.call('ga_members_natural_fvp')
    pop.call('ga_members_natural_solve')
    for m, member in enumerate(members):
        one = WidePopulation([member], cg_iters=0)
        one.call('ga_members_natural_fvp')
        one.call('ga_members_natural_solve')
        assert torch.equal(_bits(pop.product(m)), _bits(one.product(0)))
        assert torch.equal(_bits(pop.vector(0, m)), _bits(one.vector(0, 0)))


@pytest.mark.parametrize('case', [(64, 128, 8, 'gauss', 200), (32, 65, 6, 'cat', 200)])
def test_wide_backtrack_round(case):
    """Round 2 after a solve: parameters exactly prev - ratio^2 descent, loss and KL of the
    candidate against fp64 at the parameters read back."""
    pop = WidePopulation([(case, 11), (case, 12)], cg_iters=3)
    pop.call('ga_members_natural_solve')
    pop.call('ga_members_natural_candidates', 2)
    ratio = torch.tensor(-(0.8 ** 2), dtype=torch.float32)
    for m in range(2):
        got = pop.data[m]['params'].cpu()
        assert torch.equal(_bits(got), _bits(pop.vector(6, m) + ratio * pop.vector(5, m)))
        t = pop.data[m]['t']
        loss = float(surrogate(case, got.double(), t))
        kl = float(mean_kl(case, t['params'], got.double(), t['X']))
        res = pop.result[m].cpu().numpy()
        print('natural wide candidate', case, m, abs(res[0] - loss), abs(res[1] - kl), kl)
        assert abs(res[0] - loss) <= TOL['loss']
        assert abs(res[1] - kl) <= 1e-4 * kl + 1e-7  # (the narrow candidates test's bar)
