"""Every loss entry point of the C ABI, called directly, against the fp64 reference of
``tests/_loss_cases.py``: loss, log-likelihoods, entropies, gradient seed, the log-std
gradient slot, KL sums, Fisher seeds and -- for the head-in-loss entries -- the head
outputs.  Nothing goes through a network.

Cases, reference and tolerances: ``_loss_cases.py``; that fp32 itself stays within half
of every tolerance: ``test_loss_cases_cpu.py``.

What no kernel may read is NaN: the padding columns of every strided input, the pool
rows a gathered case does not name, the partial-sum slots of the reduction workspace,
the slabs, the old log-likelihoods of a VPG case.  Every output starts as NaN.  Launches
of more than one block, and the rows of ``_loss_cases.BOUNDARY_ROWS`` (one block
included: it finishes in its own launch whatever the switch says), run at both
positions of ``ga_set_one_launch_losses`` and each position is compared with the
reference, never with the other.
"""
import numpy as np
import pytest
import torch

import _loss_cases as lc

pytestmark = pytest.mark.gpu

NAN = float('nan')
N_SPLITS, SLAB_STRIDE = 3, 16


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


def _wide(t, ld, dev):
    """[n] or [n, w] fp32 -> device [n, ld] with NaN in the columns from w on."""
    t = t.reshape(t.shape[0], -1)
    out = torch.full((t.shape[0], ld), NAN, dtype=torch.float32)
    out[:, :t.shape[1]] = t
    return out.to(dev)


def _rows(c, b, key):
    """The minibatch rows of a per-sample input (what a forward pass at the gathered
    rows produces)."""
    t = b[key]
    return t if b['idx'] is None else t[torch.from_numpy(b['idx']).long()]


def _workspace(dev):
    """Partial slots NaN, the ticket / fault pair behind them zero."""
    from garage_amd import _lib
    n = int(_lib.load().ga_reduction_workspace_doubles())
    ws = torch.full((n, ), NAN, dtype=torch.float64, device=dev)
    ws[-2:] = 0.0
    return ws


def _ws_clean(ws):
    return bool((ws[-2:].view(torch.int64) == 0).all())


class _Checker:
    def __init__(self, entry, c, b):
        self.entry, self.c, self.b, self.failures = entry, c, b, []

    def __call__(self, name, got, where=''):
        ref = self.b['ref'][name]
        got = got.detach().double().cpu().numpy().reshape(ref.shape)
        tol = lc.tolerance(self.c, name, ref)
        err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float('inf')
        frac = err / tol if tol > 0 else (0.0 if err == 0 else float('inf'))
        print('LOSSCHK %-32s %-8s %-12s err %.3e  tol %.3e  frac %.3f  dev32 %.3e' % (
            self.entry, name, where, err, tol, frac, self.b['dev32'][name]))
        if not err <= tol:
            self.failures.append((name, where, err, tol))

    def slabs(self, slabs, dlogstd, where=''):
        """Slot 0 of slab 0 holds the log-std gradient (None: 0, the categorical
        head has no such parameter), slot 0 of every other slab 0, and nothing else
        was written."""
        s = slabs.view(N_SPLITS, SLAB_STRIDE).cpu()
        if dlogstd is None:
            if not (s[0, 0] == 0).item():
                self.failures.append(('slab0', where, float(s[0, 0]), 0.0))
        else:
            self('dlogstd', s[0, 0], where)
            if self.c.std in lc.ACTIVE and not (s[0, 0] == 0).item():
                self.failures.append(('active clamp', where, float(s[0, 0]), 0.0))
        if not bool((s[1:, 0] == 0).all()):
            self.failures.append(('slabs 1..', where, s[1:, 0].tolist(), 0.0))
        if not bool(torch.isnan(s[:, 1:]).all()):
            self.failures.append(('slab body written', where, 0.0, 0.0))


def _positions(M, per_block):
    return lc.ONE_LAUNCH if M > per_block or M in lc.BOUNDARY_ROWS else (0, )


def _sample(c, b, dev):
    """The per-sample device inputs of a policy case: actions (strided, class ids in
    column 0 for the categorical head), old log-likelihoods (all NaN for VPG, which
    must not read them), advantages, row ids."""
    _, lda = lc.strides(c)
    act = _wide(b['actions'], lda, dev)
    old = b['old_ll'].to(dev)
    if c.algo == 1:
        old = torch.full_like(old, NAN)
    idx = None if b['idx'] is None else torch.from_numpy(b['idx']).to(dev)
    return act, lda, old, b['adv'].to(dev), idx


def _outputs(M, ld, dev):
    return (torch.full((M, ld), NAN, device=dev), torch.full((M, ), NAN, device=dev),
            torch.full((1, ), NAN, device=dev),
            torch.full((N_SPLITS * SLAB_STRIDE, ), NAN, device=dev))


@pytest.mark.parametrize('case', lc.cases_of('gauss'), ids=lc.case_id)
def test_ppo_gaussian_loss(dev, case):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    lib = _lib.load()
    c, b = case, lc.build(case)
    ld, _ = lc.strides(c)
    mean = _wide(_rows(c, b, 'head'), ld, dev)
    act, lda, old, adv, idx = _sample(c, b, dev)
    log_std = torch.tensor([b['p']], dtype=torch.float32, device=dev)
    has_min, lo, has_max, hi = lc.log_std_args(c)
    check = _Checker('ga_ppo_gaussian_loss_f32', c, b)
    try:
        for pos in _positions(c.M, 256):
            lib.ga_set_one_launch_losses(pos)
            ws = _workspace(dev)
            dmean, ll, loss, slabs = _outputs(c.M, ld, dev)
            call('ga_ppo_gaussian_loss_f32', dptr(mean), ld, dptr(act), lda, dptr(old),
                 dptr(adv), dptr(idx), dptr(log_std), has_min, lo, has_max, hi, c.M,
                 c.A, c.algo, c.clip, lc.ENT_COEFF, c.ent_flags, dptr(dmean), dptr(ll),
                 dptr(loss), dptr(slabs), SLAB_STRIDE, N_SPLITS, dptr(ws), stream_ptr())
            where = 'one_launch %d' % pos
            check('loss', loss, where)
            check('ll', ll, where)
            check('seed', dmean[:, :c.A], where)
            check.slabs(slabs, True, where)
            assert _ws_clean(ws), where
    finally:
        lib.ga_set_one_launch_losses(0)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('cat'), ids=lc.case_id)
def test_ppo_categorical_loss(dev, case):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    lib = _lib.load()
    c, b = case, lc.build(case)
    ld, _ = lc.strides(c)
    scores = _wide(_rows(c, b, 'head'), ld, dev)
    act, lda, old, adv, idx = _sample(c, b, dev)
    check = _Checker('ga_ppo_categorical_loss_f32', c, b)
    try:
        for pos in _positions(c.M, 256):
            lib.ga_set_one_launch_losses(pos)
            ws = _workspace(dev)
            dsc, ll, loss, slabs = _outputs(c.M, ld, dev)
            ent = torch.full((c.M, ), NAN, device=dev)
            ent_sum = torch.full((1, ), NAN, dtype=torch.float64, device=dev)
            call('ga_ppo_categorical_loss_f32', dptr(scores), ld, dptr(act), lda,
                 dptr(old), dptr(adv), dptr(idx), c.M, c.A, c.dsm, c.algo, c.clip,
                 lc.ENT_COEFF, c.ent_flags, dptr(dsc), dptr(ll), dptr(ent), dptr(loss),
                 dptr(ent_sum), dptr(slabs), SLAB_STRIDE, N_SPLITS, dptr(ws),
                 stream_ptr())
            where = 'one_launch %d' % pos
            check('loss', loss, where)
            check('ll', ll, where)
            check('ent', ent, where)
            check('ent_sum', ent_sum, where)
            check('seed', dsc[:, :c.A], where)
            check.slabs(slabs, None, where)
            assert _ws_clean(ws), where
    finally:
        lib.ga_set_one_launch_losses(0)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('nll'), ids=lc.case_id)
def test_gaussian_nll_loss(dev, case):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    lib = _lib.load()
    c, b = case, lc.build(case)
    ld, _ = lc.strides(c)
    v = _wide(_rows(c, b, 'head'), ld, dev)
    ret = b['returns'].to(dev)
    idx = None if b['idx'] is None else torch.from_numpy(b['idx']).to(dev)
    log_std = torch.tensor([b['p']], dtype=torch.float32, device=dev)
    check = _Checker('ga_gaussian_nll_loss_f32', c, b)
    try:
        for pos in _positions(c.M, 256):
            lib.ga_set_one_launch_losses(pos)
            ws = _workspace(dev)
            dv, _, loss, slabs = _outputs(c.M, ld, dev)
            call('ga_gaussian_nll_loss_f32', dptr(v), ld, dptr(ret), dptr(idx),
                 dptr(log_std), c.M, dptr(dv), dptr(loss), dptr(slabs), SLAB_STRIDE,
                 N_SPLITS, dptr(ws), stream_ptr())
            where = 'one_launch %d' % pos
            check('loss', loss, where)
            check('seed', dv[:, :1], where)
            check.slabs(slabs, True, where)
            assert _ws_clean(ws), where
    finally:
        lib.ga_set_one_launch_losses(0)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('gauss'), ids=lc.case_id)
def test_gaussian_kl(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    ld, _ = lc.strides(c)
    old, new = (_wide(_rows(c, b, k), ld, dev) for k in ('head', 'head2'))
    ws = _workspace(dev)
    out = torch.full((1, ), NAN, dtype=torch.float64, device=dev)
    call('ga_gaussian_kl_f32', dptr(old), dptr(new), ld, c.M, c.A, b['s_old'],
         b['s_new'], dptr(out), dptr(ws), stream_ptr())
    check = _Checker('ga_gaussian_kl_f32', c, b)
    check('kl', out)
    assert _ws_clean(ws)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('cat'), ids=lc.case_id)
def test_categorical_kl(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    ld, _ = lc.strides(c)
    old, new = (_wide(_rows(c, b, k), ld, dev) for k in ('head', 'head2'))
    ws = _workspace(dev)
    out = torch.full((1, ), NAN, dtype=torch.float64, device=dev)
    call('ga_categorical_kl_f32', dptr(old), dptr(new), ld, c.M, c.A, c.dsm, dptr(out),
         dptr(ws), stream_ptr())
    check = _Checker('ga_categorical_kl_f32', c, b)
    check('kl', out)
    assert _ws_clean(ws)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('gauss'), ids=lc.case_id)
def test_fisher_seed_gaussian(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    ldt, ldd = lc.strides(c)  # (the seed takes the other stride)
    t = _wide(_rows(c, b, 'tangent'), ldt, dev)
    log_std = torch.tensor([b['p']], dtype=torch.float32, device=dev)
    has_min, lo, has_max, hi = lc.log_std_args(c)
    dout = torch.full((c.M, ldd), NAN, device=dev)
    call('ga_fisher_seed_gaussian_f32', dptr(t), ldt, c.M, c.A, dptr(log_std), has_min,
         lo, has_max, hi, dptr(dout), ldd, stream_ptr())
    check = _Checker('ga_fisher_seed_gaussian_f32', c, b)
    check('fisher', dout[:, :c.A])
    assert torch.isfinite(dout).all()  # (the padding columns are written too)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('cat'), ids=lc.case_id)
def test_fisher_seed_categorical(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    ld, ldd = lc.strides(c)
    scores = _wide(_rows(c, b, 'head'), ld, dev)
    t = _wide(_rows(c, b, 'tangent'), ldd, dev)
    dout = torch.full((c.M, ld), NAN, device=dev)
    call('ga_fisher_seed_categorical_f32', dptr(scores), ld, dptr(t), ldd, c.M, c.A,
         c.dsm, dptr(dout), ld, stream_ptr())
    check = _Checker('ga_fisher_seed_categorical_f32', c, b)
    check('fisher', dout[:, :c.A])
    assert torch.isfinite(dout).all()
    assert not check.failures, check.failures


def _head_layer(c, b, dev):
    """H at the minibatch rows, W and the bias; 'wide': rows of H and W 4 and 8
    floats longer than the hidden width, NaN there."""
    K = c.hidden
    ldh, ldw = (K + 4, K + 8) if c.layout == 'wide' else (K, K)
    return (_wide(_rows(c, b, 'H'), ldh, dev), ldh, _wide(b['W'], ldw, dev), ldw,
            b['b'].to(dev))


@pytest.mark.parametrize('case', lc.cases_of('hgauss'), ids=lc.case_id)
def test_head_ppo_gaussian_loss(dev, case):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    assert _lib.load().ga_head_loss_supported(c.hidden, c.A)
    ldm, ldd = lc.strides(c)
    H, ldh, W, ldw, bias = _head_layer(c, b, dev)
    act, lda, old, adv, idx = _sample(c, b, dev)
    log_std = torch.tensor([b['p']], dtype=torch.float32, device=dev)
    has_min, lo, has_max, hi = lc.log_std_args(c)
    ws = _workspace(dev)
    dmean, ll, loss, slabs = _outputs(c.M, ldd, dev)
    mean = torch.full((c.M, ldm), NAN, device=dev)
    call('ga_head_ppo_gaussian_loss_f32', dptr(H), ldh, dptr(W), ldw, dptr(bias),
         c.hidden, dptr(mean), ldm, dptr(act), lda, dptr(old), dptr(adv), dptr(idx),
         dptr(log_std), has_min, lo, has_max, hi, c.M, c.A, c.algo, c.clip,
         lc.ENT_COEFF, c.ent_flags, dptr(dmean), ldd, dptr(ll), dptr(loss), dptr(slabs),
         SLAB_STRIDE, N_SPLITS, dptr(ws), stream_ptr())
    check = _Checker('ga_head_ppo_gaussian_loss_f32', c, b)
    check('head', mean[:, :c.A])
    check('loss', loss)
    check('ll', ll)
    check('seed', dmean[:, :c.A])
    check.slabs(slabs, True)
    assert _ws_clean(ws)
    assert not check.failures, check.failures


@pytest.mark.parametrize('case', lc.cases_of('hnll'), ids=lc.case_id)
def test_head_gaussian_nll_loss(dev, case):
    from garage_amd._lib import call, dptr, stream_ptr
    c, b = case, lc.build(case)
    ldv, ldd = lc.strides(c)
    K = c.hidden
    ldh = K + 4 if c.layout == 'wide' else K
    H = _wide(_rows(c, b, 'H'), ldh, dev)
    W, bias = b['W'].to(dev), b['b'].to(dev)  # (one row: no stride)
    ret = b['returns'].to(dev)
    idx = None if b['idx'] is None else torch.from_numpy(b['idx']).to(dev)
    log_std = torch.tensor([b['p']], dtype=torch.float32, device=dev)
    ws = _workspace(dev)
    dv, _, loss, slabs = _outputs(c.M, ldd, dev)
    v = torch.full((c.M, ldv), NAN, device=dev)
    call('ga_head_gaussian_nll_loss_f32', dptr(H), ldh, dptr(W), dptr(bias), K, dptr(v),
         ldv, dptr(ret), dptr(idx), dptr(log_std), c.M, dptr(dv), ldd, dptr(loss),
         dptr(slabs), SLAB_STRIDE, N_SPLITS, dptr(ws), stream_ptr())
    check = _Checker('ga_head_gaussian_nll_loss_f32', c, b)
    check('head', v[:, :1])
    check('loss', loss)
    check('seed', dv[:, :1])
    check.slabs(slabs, True)
    assert _ws_clean(ws)
    assert not check.failures, check.failures
