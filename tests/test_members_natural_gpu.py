"""The population's natural-gradient kernels (``ga_members_natural_*``) against fp64 torch
autograd of the same network from the same flat parameters (tests/_natural_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _natural_cases import (CASES, REG, TOL, fvp, gradient, make_case, make_desc, r4,
                            rel_err, std_options)

pytestmark = pytest.mark.gpu

POISON = 12345.0
GUARD = 64
DELTA = 0.01
GA_PROF_MEMBERS_STEP = 15  # every launch of a population's step counts here


class Population:
    """Members (case, seed) of one network shape and head on the device, and the
    arguments of the entry points for them; the workspace and every product's output
    lie between poisoned guards."""

    def __init__(self, members, cg_iters=10):
        from garage_amd import _lib
        self.lib = _lib
        H, in_w, A, head, _ = members[0][0]
        self.desc, self.n_flat = make_desc(H, in_w, A)
        self.cat = head.startswith('cat')
        n = len(members)
        a = self.args = _lib.MembersNaturalArgs()
        a.desc, a.n_flat, a.n_members = C.pointer(self.desc), self.n_flat, n
        a.kind = 2 if self.cat else 0
        a.has_min, a.min_log_std, a.has_max, a.max_log_std, a.learn_std = std_options(head)
        a.double_softmax = int(head == 'cat_double')
        a.cg_iters = cg_iters
        self.arr = (_lib.MemberNatural * n)()
        a.members_host = self.arr
        self.data = []
        for u, (case, seed) in zip(self.arr, members):
            t = make_case(case, seed)
            S = case[4]
            X = torch.zeros(S, r4(in_w), device='cuda')
            X[:, :in_w] = t['X'].float()
            act = torch.zeros(S, 1 if self.cat else r4(A), device='cuda')
            act[:, :t['actions'].shape[1]] = t['actions'].float()
            d = dict(t=t, case=case, X=X, actions=act,
                     out=torch.full((self.n_flat + 2 * GUARD, ), POISON, device='cuda'))
            for k in ('params', 'adv', 'old_ll', 'vec'):
                d[k] = t[k].float().cuda()
            self.data.append(d)
            u.params, u.X, u.ldx, u.S = d['params'].data_ptr(), X.data_ptr(), X.stride(0), S
            u.actions, u.lda = act.data_ptr(), act.stride(0)
            u.old_ll, u.adv = d['old_ll'].data_ptr(), d['adv'].data_ptr()
            u.max_constraint_value, u.hvp_reg_coeff, u.backtrack_ratio = DELTA, REG, 0.8
            u.vec = d['vec'].data_ptr()
            u.out = d['out'][GUARD:].data_ptr()
        rows = (C.c_int64 * n)(*[m[0][4] for m in members])
        self.layout = (C.c_int64 * 5)()
        floats = int(_lib.load().ga_members_natural_floats(
            a.desc, self.n_flat, n, rows, self.layout))
        assert floats > 0
        self.ws = torch.full((floats + GUARD, ), POISON, device='cuda')
        a.workspace, a.workspace_floats = self.ws.data_ptr(), floats
        self.result = torch.zeros(n, 2, dtype=torch.float64, device='cuda')
        a.result = self.result.data_ptr()

    def call(self, name, *more):
        self.lib.call(name, C.byref(self.args), *more, self.lib.stream_ptr())
        torch.cuda.synchronize()
        floats = self.args.workspace_floats
        assert bool((self.ws[floats:] == POISON).all()), 'wrote past the workspace'

    def product(self, m):
        out = self.data[m]['out']
        assert bool((out[:GUARD] == POISON).all()) and bool(
            (out[GUARD + self.n_flat:] == POISON).all()), 'wrote around the product'
        return out[GUARD:GUARD + self.n_flat].cpu()

    def vector(self, v, m):
        n, nf = len(self.data), r4(self.n_flat)
        at = self.layout[0] + (v * n + m) * nf
        return self.ws[at:at + self.n_flat].cpu()

    def scalars(self, m):
        at = self.layout[1] + 16 * m
        return self.ws[at:at + 16].cpu().view(torch.float64).numpy()


@pytest.mark.parametrize('i', range(len(CASES)))
def test_product_and_gradient_against_fp64_autograd(i):
    case = CASES[i]
    pop = Population([(case, i)], cg_iters=0)
    t = pop.data[0]['t']
    pop.call('ga_members_natural_fvp')
    e_fvp = rel_err(pop.product(0), fvp(case, t, t['vec']))
    pop.call('ga_members_natural_solve')
    loss, grad = gradient(case, t)
    e_grad = rel_err(pop.vector(0, 0), grad)
    e_loss = abs(pop.scalars(0)[3] - float(loss))
    print('natural gpu case', i, case, dict(fvp=e_fvp, grad=e_grad, loss=e_loss))
    assert e_fvp <= TOL['fvp'] and e_grad <= TOL['grad'] and e_loss <= TOL['loss']


@pytest.mark.parametrize('head', ['gauss', 'cat_double'])
def test_a_member_gets_the_same_bits_whatever_the_population(head):
    """Three members with different S and parameters: product and gradient bit for bit
    those of a population of one."""
    members = [((64, 17, 6, head, S), seed) for S, seed in ((1094, 1), (65, 2), (200, 3))]
    pop = Population(members, cg_iters=0)
    pop.call('ga_members_natural_fvp')
    pop.call('ga_members_natural_solve')
    for m, member in enumerate(members):
        one = Population([member], cg_iters=0)
        one.call('ga_members_natural_fvp')
        one.call('ga_members_natural_solve')
        assert torch.equal(pop.product(m).view(torch.int32), one.product(0).view(torch.int32))
        assert torch.equal(pop.vector(0, m).view(torch.int32),
                           one.vector(0, 0).view(torch.int32))


def _cg_fp64(case, t, cg_iters):
    """ConjugateGradientOptimizer's recurrence (conjugate_gradient_optimizer.py:69-104,
    160-166) in fp64 numpy with the fp64 product."""
    def A(v):
        return fvp(case, t, torch.from_numpy(v)).numpy()
    b = gradient(case, t)[1].numpy()
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rdotr = r @ r
    iters = 0
    for _ in range(cg_iters):
        z = A(p)
        v = rdotr / (p @ z)
        x += v * p
        r -= v * z
        new = r @ r
        p = r + (new / rdotr) * p
        rdotr = new
        iters += 1
        if rdotr < 1e-10:
            break
    sAs = x @ A(x)
    return x, np.sqrt(2.0 * DELTA / (sAs + 1e-8)) * x, sAs, iters


@pytest.mark.parametrize('cg_iters', [1, 10])
@pytest.mark.parametrize('case', [(64, 17, 1, 'gauss', 200), (64, 17, 6, 'gauss_fixed', 200),
                                  (32, 3, 6, 'cat', 200)],
                         ids=['gauss17', 'gauss17_fixed', 'cat3'])
def test_cg_recurrence_against_fp64(case, cg_iters):
    """step_dir, descent_step and x.Ax against the fp64 recurrence.  This path replaces
    the lone TRPO's fp32 recurrence (same operations, dots in fp64), so the bars are the
    ones tests/test_trpo_gpu.py holds that one's first iteration to: 5e-4 of the largest
    magnitude for step_dir, 1e-3 for descent_step (and for x.Ax, which descent_step's
    length is a function of).  The launch count is 2 (cg_iters + 1) + 2 whatever the
    member count.

    The data are ones on which ANY fp32 recurrence can meet those bars: a numpy fp32
    recurrence with the fp64 product stays within 7e-7 of the fp64 one after 10
    iterations on these three.  A learned std beside SIX outputs does not qualify: its
    slot is an eigenvalue of 12 far above the rest, an fp32 recurrence finds it a second
    time around iteration 8 and the numpy fp32 recurrence itself ends 1.7e-2 away from
    fp64 (so did the kernels, 1.69e-2, at one iteration within 5e-4); that head's
    product and gradient are held to fp64 by the cases above."""
    pop = Population([(case, 5), (case, 6)], cg_iters=cg_iters)
    lib = pop.lib.load()
    before = int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP))
    pop.call('ga_members_natural_solve')
    after = int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP))
    assert after - before == 2 * (cg_iters + 1) + 2
    for m in range(2):
        x, descent, sAs, _ = _cg_fp64(case, pop.data[m]['t'], cg_iters)
        assert rel_err(pop.vector(1, m), x) <= 5e-4
        assert rel_err(pop.vector(5, m), descent) <= 1e-3
        assert abs(pop.scalars(m)[1] - sAs) <= 1e-3 * abs(sAs)


def test_a_finished_member_is_frozen_while_its_neighbour_runs_on():
    """One row: the Fisher matrix has rank <= 6 (+ reg I), so the recurrence falls under
    1e-10 within a few iterations; the 200-row neighbour uses all 10."""
    small, big = (32, 3, 6, 'gauss_fixed', 1), (32, 3, 6, 'gauss_fixed', 200)
    pop = Population([(small, 7), (big, 8)], cg_iters=10)
    pop.call('ga_members_natural_solve')
    x, descent, sAs, iters = _cg_fp64(small, pop.data[0]['t'], 10)
    s0, s1 = pop.scalars(0), pop.scalars(1)
    assert iters < 10 and s0[4] == 1.0 and s0[5] < 10
    assert s1[4] == 0.0 and s1[5] == 10
    assert rel_err(pop.vector(1, 0), x) <= 5e-4
    assert rel_err(pop.vector(5, 0), descent) <= 1e-3
    x1, _, _, _ = _cg_fp64(big, pop.data[1]['t'], 10)
    assert rel_err(pop.vector(1, 1), x1) <= 5e-4


def test_backtrack_round_composes_and_evaluates_candidates():
    """Round k: parameters exactly prev - ratio^k descent, loss and KL of the candidate
    against fp64, two launches; a rejected member gets prev back, an accepted one is left."""
    from _natural_cases import mean_kl, surrogate
    case = (64, 17, 6, 'gauss', 200)
    pop = Population([(case, 11), (case, 12), (case, 13)], cg_iters=3)
    lib = pop.lib.load()
    pop.call('ga_members_natural_solve')
    prev = [pop.vector(6, m) for m in range(3)]
    descent = [pop.vector(5, m) for m in range(3)]
    pop.arr[1].state = 1  # accepted earlier: untouched
    before = int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP))
    pop.call('ga_members_natural_candidates', 2)
    assert int(lib.ga_launch_count(GA_PROF_MEMBERS_STEP)) - before == 2
    ratio = torch.tensor(-(0.8 ** 2), dtype=torch.float32)
    for m in (0, 2):
        want = prev[m] + ratio * descent[m]
        got = pop.data[m]['params'].cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        t = dict(pop.data[m]['t'])
        loss = float(surrogate(case, got.double(), t))
        kl = float(mean_kl(case, t['params'], got.double(), t['X']))
        res = pop.result[m].cpu().numpy()
        assert abs(res[0] - loss) <= TOL['loss']
        assert abs(res[1] - kl) <= 1e-4 * kl + 1e-7  # (ga_gaussian_kl_f32's bar)
    assert torch.equal(pop.data[1]['params'].cpu(), prev[1])
    pop.arr[0].state, pop.arr[2].state = 2, 1
    pop.call('ga_members_natural_candidates', 3)
    assert torch.equal(pop.data[0]['params'].cpu(), prev[0])
    assert not torch.equal(pop.data[2]['params'].cpu(), prev[2])
