"""Precondition of ``test_loss_entries_fp64_gpu.py`` and ``test_loss_paths_fp64_gpu.py``:
the fp64 reference of ``_loss_cases.py`` says what ``oracle.networks`` says; its table
holds what it claims; no row of a case sits on a clip edge; and on every case fp32
arithmetic by itself (torch on the CPU, the same formulas) stays within HALF of the
tolerance the HIP kernels are held to.  A GPU result outside the tolerance is then the
kernel's doing, not the case's.  (No GPU, no library.)"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _loss_cases as lc

_SEEN = {}


def _measure(c):
    """{name: (fp32 deviation, bound, max |ref|)} of a case, computed once."""
    if c not in _SEEN:
        b = lc.build(c)
        out = OrderedDict()
        for name, ref in b['ref'].items():
            assert np.isfinite(ref).all(), (lc.case_id(c), name)
            out[name] = (b['dev32'][name], lc.tolerance(c, name, ref),
                         float(np.abs(ref).max()))
        _SEEN[c] = (out, b.get('edge_rows_left', 0), b['edge_rounds'])
    return _SEEN[c]


def test_table_covers_what_it_claims():
    g = lc.cases_of('gauss')
    assert {c.A for c in g} >= set(lc.GAUSS_A)
    for A in lc.GAUSS_A:
        assert {c.M for c in g if c.A == A} >= set(lc.ROWS)
    assert {c.A for c in g if c.M == lc.BIG} == {1, 2, 3, 4}
    assert {c.algo for c in g if c.M == lc.BIG} == {0, 1, 2}
    assert {c.std for c in g} == set(lc.LOG_STD)
    assert {c.ent_flags for c in g} == set(lc.ENT_FLAGS)
    assert {c.algo for c in g} == {0, 1, 2} and {c.layout for c in g} == set(lc.LAYOUTS)
    assert {c.clip for c in g} == {lc.CLIP, lc.CLIP_ONCE}
    for M in lc.ROWS:
        assert {c.algo for c in g if c.M == M} == {0, 1, 2}
    # the softplus entropy on both sides of its threshold of 20
    past = {}
    for c in g:
        if c.ent_flags & 2:
            o = lc.options(c)
            p = torch.tensor([lc.LOG_STD[c.std][0]], dtype=torch.float64)
            ent = lc.gaussian(torch.zeros(1, c.A, dtype=torch.float64), p,
                              o).entropy().item()
            past.setdefault(ent > 20.0, set()).add(c.A)
    assert past[True] == {17, 32} and past[False] >= {1, 2, 8, 9}
    # an active clamp with every algo; the parameter on the clamp
    assert {c.algo for c in g if c.std in lc.ACTIVE} == {0, 1, 2}
    cat = lc.cases_of('cat')
    for A in lc.CAT_A:
        assert {(c.scores, c.dsm) for c in cat if c.A == A} == {
            (s, d) for s in lc.SCORES for d in (0, 1)}
    assert {c.M for c in cat} == set(lc.ROWS) | {lc.BIG, lc.CAPPED}
    assert {c.M for c in cat if c.scores == 'randn'} >= set(lc.ROWS)
    for sc in ('shift', 'x30'):
        assert {c.M for c in cat if c.scores == sc} >= set(lc.ROWS[1:])
    assert {c.ent_flags for c in cat} == set(lc.ENT_FLAGS)
    assert {c.algo for c in cat} == {0, 1, 2}
    assert all(c.A <= 4 for c in lc.CASES if c.M in (lc.BIG, lc.CAPPED))
    assert {c.M for c in lc.cases_of('nll')} == set(lc.ROWS) | {lc.BIG, lc.CAPPED}
    # the grid's boundaries of every two-phase entry, at a width of 1 or 3
    assert lc.BOUNDARY_ROWS == (1, 257, 256 * 512 + 1)
    for kind in ('gauss', 'cat', 'nll'):
        for M in lc.BOUNDARY_ROWS:
            assert any(c.M == M and c.A in lc.BOUNDARY_A for c in lc.cases_of(kind)), (kind, M)
    for M in lc.BOUNDARY_ROWS:
        assert {c.A for c in g if c.M == M} >= set(lc.BOUNDARY_A)
    h = lc.cases_of('hgauss')
    for hidden in lc.HEAD_HIDDEN:
        assert {c.A for c in h if c.hidden == hidden} >= set(lc.HEAD_A)
        assert {c.M for c in h if c.hidden == hidden} >= set(lc.HEAD_ROWS)
    assert [c.hidden for c in h if c.A == 64] == [64, 64]
    assert [c.hidden for c in h if c.M == lc.HEAD_BIG] == [64]
    assert {c.std for c in h} == set(lc.LOG_STD) and {c.algo for c in h} == {0, 1, 2}
    n = lc.cases_of('hnll')
    assert {c.hidden for c in n} == set(lc.HEAD_HIDDEN)
    assert {c.M for c in n} == set(lc.HEAD_ROWS) | {lc.HEAD_BIG}
    # gathered rows, repeats included, with strides wider than the head
    for kind in ('gauss', 'cat', 'nll', 'hgauss', 'hnll'):
        assert any(c.gather and c.layout == 'wide' for c in lc.cases_of(kind)), kind
    for c in lc.CASES:
        ld, lda = lc.strides(c)
        assert ld >= c.A and lda >= c.A
    assert all(b <= lc.CEILING and b >= 2 * m for b, m in lc.WIDENED.values())


def test_path_tables_cover_what_they_claim():
    """The case tables of ``test_loss_paths_fp64_gpu.py``."""
    import _loss_path_cases as pc
    pc.check_tables()
    for cases in (pc.NARROW, pc.FUSED, pc.SMALL, pc.HEAD, pc.PER_LAYER):
        assert len({pc.case_id(c) for c in cases}) == len(cases)


def _golden_params(g, prefix):
    return OrderedDict((k[len(prefix):], torch.from_numpy(g[k].copy()))
                       for k in g.files if k.startswith(prefix))


@pytest.mark.parametrize('ent_flags', lc.ENT_FLAGS)
def test_reference_reproduces_the_oracle_on_the_golden_policy(golden, ent_flags):
    """The item-1 formulas in fp32 on the head outputs of the golden ``tiny`` networks
    against ``oracle.networks``' own distributions and loss, to 1e-6."""
    from oracle import networks as nets
    g = golden('networks')
    pol, vf = _golden_params(g, 'tiny_pol:'), _golden_params(g, 'tiny_vf:')
    rng = np.random.RandomState(3)
    M, O, A = 97, 4, 2
    obs = torch.from_numpy(rng.randn(M, O).astype(np.float32))
    act = torch.from_numpy(rng.randn(M, A).astype(np.float32))
    adv = torch.from_numpy(rng.randn(M).astype(np.float32))
    noise = torch.from_numpy((0.3 * rng.randn(M)).astype(np.float32))
    lo = pol['_module.min_std_param'].item()
    p = pol['_module._init_std']
    close = lambda a, b: torch.allclose(a, b, rtol=1e-6, atol=1e-6)

    def oracle_loss(dist, a, o):
        # _ppo_oracle_loss of test_kernels_gpu.py, + the TRPO surrogate and the
        # stop-gradient option
        ll = dist.log_prob(a)
        old = ll.detach() + noise
        if o.algo == 1:
            obj = ll * adv
        else:
            ratio = (ll - old).exp()
            obj = ratio * adv if o.algo == 2 else torch.min(
                ratio * adv, torch.clamp(ratio, 1 - o.clip, 1 + o.clip) * adv)
        if o.ent_flags & 1:
            e = dist.entropy()
            if o.ent_flags & 2:
                e = torch.nn.functional.softplus(e)
            obj = obj + o.coeff * (e.detach() if o.ent_flags & 4 else e)
        return -obj.mean(), ll, old

    head = nets.mlp_mean(pol, '_module.', obs)
    for sp in (False, True):
        for algo in (0, 1, 2):
            o = lc.Opt(lo, None, sp, algo, lc.CLIP, ent_flags, lc.ENT_COEFF, 0)
            with nets.std_parameterization('softplus' if sp else 'exp'):
                dist = nets.gaussian_dist(pol, '_module.', obs)
            want, ll_o, old = oracle_loss(dist, act, o)
            mine = lc.gaussian(head, p, o)
            assert close(mine.stddev, dist.stddev)
            loss, ll, ent = lc.policy_loss(mine, act, old, adv, o)
            assert close(ll, ll_o) and close(loss, want), (sp, algo)
            e = dist.entropy()
            assert close(ent, torch.nn.functional.softplus(e) if ent_flags & 2 else e)
    cls = torch.from_numpy(rng.randint(0, A, size=M))
    for dsm in (0, 1):
        for algo in (0, 1, 2):
            o = lc.Opt(None, None, False, algo, lc.CLIP, ent_flags, lc.ENT_COEFF, dsm)
            dist = nets.categorical_dist(pol, '_module.', obs, double_softmax=bool(dsm))
            want, ll_o, old = oracle_loss(dist, cls, o)
            loss, ll, _ = lc.policy_loss(lc.categorical(head, o), cls, old, adv, o)
            assert close(ll, ll_o) and close(loss, want), (dsm, algo)
    ret = torch.from_numpy(rng.randn(M).astype(np.float32))
    v = nets.mlp_mean(vf, 'module.', obs)
    assert close(lc.value_loss(v, vf['module._init_std'], ret),
                 nets.value_loss(vf, obs, ret))


def test_fisher_seed_reference_is_the_closed_form():
    """The double backward of the fp64 KL against what the header documents: the
    Gaussian block is tangent * exp(-2 s) / M."""
    rng = np.random.RandomState(5)
    M, A = 7, 3
    mean = torch.from_numpy(rng.randn(M, A))
    t = torch.from_numpy(rng.randn(M, A))
    p = torch.tensor([-0.3125], dtype=torch.float64)
    o = lc.Opt(None, None, False, 0, lc.CLIP, 0, 0.0, 0)
    got = lc.fisher_seed(lambda h: lc.gaussian(h, p, o), mean, t)
    assert torch.allclose(got, t * np.exp(2 * 0.3125) / M, rtol=1e-12)


@pytest.mark.parametrize('case', lc.CASES, ids=lc.case_id)
def test_fp32_deviation_is_within_half_the_tolerance(case):
    res, edge_left, rounds = _measure(case)
    assert edge_left == 0 and rounds <= lc.CLIP_EDGE_ROUNDS
    want = {'nll': {'loss', 'seed', 'dlogstd'},
            'hnll': {'loss', 'seed', 'dlogstd', 'head'},
            'gauss': {'loss', 'll', 'seed', 'dlogstd', 'kl', 'fisher'},
            'hgauss': {'loss', 'll', 'seed', 'dlogstd', 'head'},
            'cat': {'loss', 'll', 'ent', 'ent_sum', 'seed', 'kl', 'fisher'}}[case.kind]
    assert set(res) == want
    if case.std in lc.ACTIVE and 'dlogstd' in res:
        assert lc.build(case)['ref']['dlogstd'].item() == 0.0
    elif 'dlogstd' in res and case.M > 1:  # (a single PPO row may be a clipped one)
        assert lc.build(case)['ref']['dlogstd'].item() != 0.0
    worst = []
    for name, (dev, tol, scale) in res.items():
        print('%-8s dev32 %.3e  tol %.3e  max|ref| %.3e' % (name, dev, tol, scale))
        if not dev <= 0.5 * tol:
            worst.append((name, dev, tol))
    assert not worst, worst


def test_worst_fp32_deviation_per_class():
    """The figure ``_loss_cases.WIDENED`` records: per (class, kind, A) the worst fp32
    deviation as a fraction of the bound, over the whole table."""
    worst = {}
    for c in lc.CASES:
        for name, (dev, tol, scale) in _measure(c)[0].items():
            frac = dev / tol if tol > 0 else (0.0 if dev == 0 else float('inf'))
            key = (name, c.kind, c.A)
            if frac > worst.get(key, (-1.0, ))[0]:
                worst[key] = (frac, dev / scale if scale else 0.0, lc.case_id(c))
    over = []
    for key in sorted(worst, key=lambda k: -worst[k][0]):
        frac, rel, cid = worst[key]
        print('%-28s %.3f of the bound  (%.3e of max|ref|)  %s' % (key, frac, rel, cid))
        if frac > 0.5:
            over.append((key, frac, rel, cid))
    assert not over, over
