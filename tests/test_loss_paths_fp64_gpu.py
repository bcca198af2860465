"""Every update path -- the per-layer kernels, the GEMM-epilogue kernels of
fused_train.hip (with and without the first layer inside), narrow_step.hip,
small_step.hip and the head-in-loss kernels -- against fp64 autograd of network plus
objective: the loss and the whole flat gradient, the log-std slot included.

The reference is ``oracle.networks.mlp_mean`` on float64 copies of the parameters,
composed with the objective of ``tests/_loss_cases.py`` (pinned to ``oracle.networks``
by ``test_loss_cases_cpu.py``).  Each path is compared with the reference, never with
another path, and each run asserts that the path it means was the one taken.

``VPG._minibatch_step`` stops at the reduced gradient when the optimizer has a
``grad_hook`` (``phase = 1`` of ``ga_update_epoch``): that serves every path but
small_step.hip, which does not run under ``phase = 1``; see ``_small_step``.
"""
import ctypes as C
import types
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _loss_cases as lc
import _loss_path_cases as pc
import _mlp_option_cases as oc
from _loss_path_cases import FUSED, HEAD, NARROW, PER_LAYER, SMALL

pytestmark = pytest.mark.gpu

NAN = float('nan')
PREFIX = oc.PREFIX
# GA_PROF_* of csrc/prof.h
FUSED_FWD, NARROW_STEP = 9, 11
@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class _Problem:
    """The algorithm object, the network under test with drawn parameters, and a
    minibatch: observations, samples (NaN in the pool rows no minibatch row names) and
    row ids.  ``lead``: that many more samples behind the M of the minibatch (rows
    M .. M + lead - 1), with LEAD_SIGNAL of the usual advantages / returns noise: the
    first minibatch of a pass whose ragged tail is the case (``_small_step``)."""

    LEAD_SIGNAL = 0.05

    def __init__(self, p, dev, opt, lead=0):
        from garage_amd._dtypes import Box, Discrete, EnvSpec
        from garage_amd.algos import PPO, VPG
        from garage_amd.engine import pad_rows
        from garage_amd.optimizers import OptimizerWrapper
        from garage_amd.policies import (CategoricalMLPPolicy, GaussianMLPPolicy,
                                         GaussianMLPValueFunction)
        self.p, self.dev, self.lead = p, dev, lead
        assert not (lead and p.gather)
        O, A, hidden = p.dims[0], p.dims[-1], p.dims[1:-1]
        discrete = p.kind == 'cat'
        act_dim = 2 if p.kind == 'nll' else A
        spec = EnvSpec(Box(-np.inf, np.inf, (O, )),
                       Discrete(act_dim) if discrete else Box(-np.inf, np.inf,
                                                              (act_dim, )),
                       max_episode_length=10)
        param, lo, hi, sp = lc.LOG_STD[p.std]
        if discrete:
            pol = CategoricalMLPPolicy(spec, hidden_sizes=hidden,
                                       double_softmax=bool(p.dsm))
        else:
            pol = GaussianMLPPolicy(
                spec, hidden_sizes=hidden, learn_std=p.learn_std,
                min_std=None if lo is None else float(np.exp(lo)),
                max_std=None if hi is None else float(np.exp(hi)),
                std_parameterization='softplus' if sp else 'exp')
        vf = GaussianMLPValueFunction(spec, hidden_sizes=hidden)
        kw = {}
        if p.ent == 'reg_sp':
            kw = dict(entropy_method='regularized', policy_ent_coeff=lc.ENT_COEFF,
                      use_softplus_entropy=True)
        elif p.ent == 'max_stop':
            kw = dict(entropy_method='max', policy_ent_coeff=lc.ENT_COEFF,
                      center_adv=False, stop_entropy_gradient=True)
        self.algo = (VPG if p.vpg else PPO)(
            env_spec=spec, policy=pol, value_function=vf, sampler=None,
            policy_optimizer=OptimizerWrapper(opt, pol),
            vf_optimizer=OptimizerWrapper(opt, vf), **kw)
        self.module = vf if p.kind == 'nll' else pol
        self.opt = (self.algo._vf_optimizer if p.kind == 'nll' else
                    self.algo._policy_optimizer)
        self.kind = 1 if p.kind == 'nll' else 0
        net = self.net = self.module.net
        assert net.dims == p.dims
        # parameters: weights ~ N(0, 1 / fan_in), biases ~ 0.1 N(0, 1); the log-std
        # parameter of the case (exactly on the clamp for 'at_lo')
        rng = _rng('path', p)
        net.params.zero_()
        for key, view in net.named_views():
            if key.endswith('weight'):
                view.copy_(_f32(rng.randn(*view.shape) / np.sqrt(view.shape[1])))
            elif key.endswith('bias'):
                view.copy_(_f32(0.1 * rng.randn(*view.shape)))
        if p.kind == 'gauss':
            net.params[0] = pol._min_log_std if p.std == 'at_lo' else param
            self.lo, self.hi, self.sp = pol._min_log_std, pol._max_log_std, sp
        elif p.kind == 'nll':
            net.params[0] = -0.3125
        self.p0 = net.params.clone()
        # the minibatch
        pool = pc.GATHER_POOL if p.gather else p.M + lead
        signal = np.ones(pool)
        signal[p.M:p.M + lead] = self.LEAD_SIGNAL
        self.idx = rng.randint(0, pool, size=p.M).astype(np.int64) if p.gather else None
        used = np.ones(pool, dtype=bool)
        if self.idx is not None:
            used[:] = False
            used[self.idx] = True
        self.X = _f32(rng.randn(pool, O))
        o = self.options()
        with torch.no_grad():
            params = self.params64(self.p0)
            head = self.head64(params, self.X.double())
            p64 = params[PREFIX + '_init_std']
            self.adv = self.old_ll = self.returns = None
            if p.kind == 'nll':
                self.actions = torch.zeros(pool, act_dim)
                self.returns = _f32(head[:, 0].numpy() +
                                    1.5 * float(p64.exp()) * signal * rng.randn(pool))
            else:
                if discrete:
                    self.actions = _f32(rng.randint(0, A, size=pool))
                    dist = lc.categorical(head, o)
                    ll = dist.log_prob(self.actions.long())
                else:
                    std = lc.gaussian(head[:1], p64, o).stddev[0, 0].item()
                    self.actions = _f32(head.numpy() + 1.25 * std * rng.randn(pool, A))
                    ll = lc.gaussian(head, p64, o).log_prob(self.actions.double())
                self.adv = _f32(signal * (0.5 + rng.randn(pool)))
                ll64 = ll.numpy()
                ll32 = ll64.astype(np.float32)
                old = ll32 + (0.3 * rng.randn(pool)).astype(np.float32)
                edge = types.SimpleNamespace(clip=o.clip if o.clip else lc.CLIP)
                for _ in range(lc.CLIP_EDGE_ROUNDS):
                    bad = lc.edge_rows(edge, ll64, old) & used
                    if not bad.any():
                        break
                    old[bad] = ll32[bad] + (0.3 * rng.randn(int(bad.sum()))).astype(
                        np.float32)
                assert not (lc.edge_rows(edge, ll64, old) & used).any()
                self.old_ll = _f32(old)
        unused = torch.from_numpy(~used)
        for t in (self.X, self.actions, self.adv, self.old_ll, self.returns):
            if t is not None:
                t[unused] = NAN
        self.batch = types.SimpleNamespace(
            n_samples=pool, obs_dev=pad_rows(self.X),
            actions_dev=pad_rows(self.actions.reshape(pool, -1)))
        up = lambda t: None if t is None else t.to(dev)
        self.adv_dev, self.old_dev, self.ret_dev = up(self.adv), up(self.old_ll), up(
            self.returns)
        self.idx_dev = None if self.idx is None else torch.from_numpy(
            self.idx.astype(np.int32)).to(dev)

    def options(self):
        a, p = self.algo, self.p
        lo = hi = None
        sp = False
        if p.kind == 'gauss':
            lo, hi, sp = self.lo, self.hi, self.sp
        return lc.Opt(lo, hi, sp, a._algo_id, float(np.float32(a._lr_clip_range)),
                      a._ent_flags(), float(np.float32(a._policy_ent_coeff)), p.dsm)

    def params64(self, flat):
        return OrderedDict((PREFIX + key, view.detach().double().cpu().clone())
                           for key, view in self.net.named_views(flat))

    @staticmethod
    def head64(params, X):
        from oracle import networks as nets
        return nets.mlp_mean(params, PREFIX, X)

    def reference(self, flat, rows=None):
        """fp64 autograd of network + objective at the parameters ``flat`` on the
        minibatch (``rows``: other row ids) -> (loss, {key: gradient})."""
        p, o = self.p, self.options()
        params = self.params64(flat)
        for t in params.values():
            t.requires_grad_(True)
        if rows is None:
            rows = np.arange(self.p.M, dtype=np.int64) if self.lead else self.idx
        take = (lambda t: t.double()) if rows is None else (
            lambda t: t.double()[torch.from_numpy(rows)])
        head = self.head64(params, take(self.X))
        p64 = params[PREFIX + '_init_std']
        if p.kind == 'nll':
            loss = lc.value_loss(head, p64, take(self.returns))
        else:
            if p.kind == 'cat':
                dist, act = lc.categorical(head, o), take(self.actions).long()
            else:
                dist, act = lc.gaussian(head, p64, o), take(self.actions)
            loss, _, _ = lc.policy_loss(dist, act, take(self.old_ll), take(self.adv), o)
        grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
        out = OrderedDict()
        for key, g in zip(params, grads):
            g = torch.zeros_like(params[key]) if g is None else g
            if key.endswith('_init_std') and not getattr(self.module, '_learn_std', True):
                g = torch.zeros_like(g)  # a buffer: no gradient, no step
            out[key[len(PREFIX):]] = g.numpy()
        return loss.item(), out

    def reset(self):
        net = self.net
        net.params.copy_(self.p0)
        net.grads.fill_(NAN)
        net.exp_avg.zero_()
        net.exp_avg_sq.zero_()
        net.adam_steps = 0

    def gradient_step(self):
        """One minibatch through ``ga_update_epoch`` stopping at the reduced gradient
        -> (loss, flat gradient)."""
        got = []
        self.opt.grad_hook = lambda g: got.append(g.clone())
        try:
            loss = self.algo._minibatch_step(self.opt, self.module, self.kind, self.batch,
                                             self.adv_dev, self.ret_dev, self.old_dev,
                                             self.idx_dev)
        finally:
            self.opt.grad_hook = None
        torch.cuda.synchronize()
        if not self.p.learn_std or self.p.kind == 'cat':
            # the optimizer step that followed did not move the log-std slot
            assert self.net.params[0].item() == self.p0[0].item()
        return float(loss.item()), got[0]


def _compare(prob, where, loss, flat, ref_loss, ref, failures, extra=None):
    """``extra``: {key: per-element widening of the gradient bound}."""
    loss_case = types.SimpleNamespace(kind='path', A=prob.p.dims[-1])
    tol = lc.tolerance(loss_case, 'loss', np.asarray(ref_loss))
    err = abs(loss - ref_loss) if np.isfinite(loss) else float('inf')
    print('PATHCHK %-12s %-40s err %.3e  tol %.3e  frac %.3f' % (where, 'loss', err, tol,
                                                                err / tol))
    if not err <= tol:
        failures.append((where, 'loss', err, tol))
    for key, view in prob.net.named_views(flat):
        r = ref[key]
        got = view.detach().double().cpu().numpy().reshape(r.shape)
        tol = oc.tolerance('grad.' + key, r)
        bound = tol if extra is None else tol + extra[key]
        d = np.abs(got - r)
        frac = float((d / bound).max()) if np.isfinite(got).all() else float('inf')
        print('PATHCHK %-12s %-40s err %.3e  tol %.3e  frac %.3f' % (
            where, key, float(d.max()), tol, frac))
        if not frac <= 1.0:
            failures.append((where, key, float(d.max()), tol))
        if key == '_init_std' and prob.p.kind == 'gauss' and (
                prob.p.std in lc.ACTIVE or not prob.p.learn_std):
            if not (got == 0.0).all():  # an active clamp, or a buffer: exactly 0
                failures.append((where, 'log-std slot not 0', float(got[0]), 0.0))


def _switches(lib, fused_train=1, small_step=1, narrow=1, first_layer=1):
    lib.ga_set_fused_train(fused_train)
    lib.ga_set_small_step(small_step)
    lib.ga_set_narrow_step(narrow)
    lib.ga_set_fused_first_layer(first_layer)


def _counts(lib):
    return (int(lib.ga_launch_count(FUSED_FWD)), int(lib.ga_launch_count(NARROW_STEP)),
            int(lib.ga_small_step_launches()))


ADAM = (torch.optim.Adam, dict(lr=1e-3))


@pytest.mark.parametrize('p', PER_LAYER, ids=pc.case_id)
def test_per_layer_path(dev, p):
    from garage_amd import _lib
    lib = _lib.load()
    prob = _Problem(p, dev, ADAM)
    ref_loss, ref = prob.reference(prob.p0)
    failures = []
    try:
        _switches(lib, fused_train=0, small_step=0)
        prob.reset()
        before = _counts(lib)
        loss, flat = prob.gradient_step()
        assert _counts(lib) == before  # no fused, narrow or small-step launch
        _compare(prob, 'per-layer', loss, flat, ref_loss, ref, failures)
    finally:
        _switches(lib)
    assert not failures, failures


@pytest.mark.parametrize('p', NARROW, ids=pc.case_id)
def test_narrow_step_path(dev, p):
    from garage_amd import _lib
    lib = _lib.load()
    prob = _Problem(p, dev, ADAM)
    ref_loss, ref = prob.reference(prob.p0)
    failures = []
    _switches(lib)
    prob.reset()
    before = _counts(lib)
    loss, flat = prob.gradient_step()
    after = _counts(lib)
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, 1, 0)
    _compare(prob, 'narrow', loss, flat, ref_loss, ref, failures)
    assert not failures, failures


@pytest.mark.parametrize('p', FUSED, ids=pc.case_id)
def test_fused_gemm_epilogue_path(dev, p):
    """With the first layer inside the last-hidden-layer kernel and without it: both
    against the reference; at two hidden layers of 128 or 256 units (where
    test_fused_train_gpu.py shows the kernel takes the first layer) and more than a
    tile of rows, the two are different kernels and give different bits."""
    from garage_amd import _lib
    lib = _lib.load()
    prob = _Problem(p, dev, ADAM)
    ref_loss, ref = prob.reference(prob.p0)
    failures, flats = [], []
    try:
        for first in (0, 1):
            _switches(lib, narrow=0, first_layer=first)
            prob.reset()
            before = _counts(lib)
            loss, flat = prob.gradient_step()
            after = _counts(lib)
            assert (after[0] - before[0], after[1] - before[1],
                    after[2] - before[2]) == (1, 0, 0)
            _compare(prob, 'fused first %d' % first, loss, flat, ref_loss, ref, failures)
            flats.append(flat)
    finally:
        _switches(lib)
    if len(p.dims) == 4 and p.dims[1] == p.dims[2] >= 128 and p.M >= 127:
        assert not torch.equal(flats[0], flats[1])
    assert not failures, failures


@pytest.mark.parametrize('p', HEAD, ids=pc.case_id)
def test_head_in_loss_path(dev, p):
    """``algo.fuse_head = True``: the per-layer kernels with the head layer computed
    inside the loss kernel -- other bits than the per-layer path with the head GEMM."""
    from garage_amd import _lib
    lib = _lib.load()
    prob = _Problem(p, dev, ADAM)
    assert lib.ga_head_loss_supported(p.dims[-2], p.dims[-1])
    ref_loss, ref = prob.reference(prob.p0)
    failures, flats = [], []
    try:
        for fuse in (False, True):
            _switches(lib, fused_train=0, small_step=0)
            prob.algo.fuse_head = fuse
            prob.reset()
            before = _counts(lib)
            loss, flat = prob.gradient_step()
            assert _counts(lib) == before
            if fuse:
                _compare(prob, 'head-in-loss', loss, flat, ref_loss, ref, failures)
            flats.append(flat)
    finally:
        _switches(lib)
        lib.ga_set_fused_head_loss(0)
    assert not torch.equal(flats[0], flats[1])
    assert not failures, failures


def _small_step(prob, lib):
    """small_step.hip does the optimizer step itself, so the gradient is recovered from
    the step.  Adam with lr = 1, beta1 = beta2 = 0, eps = 1 moves a parameter by
    u = g / (|g| + 1) (both bias corrections are 1), so with u = p_before - p_after,
    g = u / (1 - |u|).  p_after is rounded to fp32: u is off by up to
    ulp(max(|p_before|, |p_after|)), and d g / d u = 1 / (1 - |u|)^2 = (1 + |g|)^2, so
    the recovered gradient carries ulp(max(|p_before|, |p_after|)) (1 + |g|)^2 on top
    of its own error.  That term widens the bound element by element; parameters here
    are of order 1 (ulp ~ 1e-7) and gradients at most ~10 (a single row's), so it stays
    under the gradient tolerance's 1e-5, which the test asserts.

    The kernel takes minibatches of up to 64 rows but needs activation workspaces sized
    for 32 rows or more, so a minibatch of fewer than 32 rows reaches it only as the
    ragged tail of a pass.  Such a case runs a pass of 32 + M rows with minibatches of
    32 from the case's parameters: the parameters after the first step come from a
    pass of those 32 rows alone, the tail's step is the difference of the two passes'
    results, and the reference is taken at the parameters the tail's step started
    from.  That first step is at lr = 1 too, so the 32 leading samples carry a twentieth
    of the usual signal (_Problem.LEAD_SIGNAL): at full size it moves a 256-unit value
    net far enough for the tail's log-std gradient to reach ~50, which the recovery
    above cannot hold to the tolerance (the first step of both passes is the same launch on the same inputs, and the
    kernel's sums have a fixed order: the same bits).
    -> (loss, recovered flat gradient, parameters before the step, widening)."""
    from garage_amd._lib import call, stream_ptr
    p, net, algo = prob.p, prob.net, prob.algo
    before = _counts(lib)
    if p.M >= 32:
        prob.reset()
        loss = algo._minibatch_step(prob.opt, prob.module, prob.kind, prob.batch,
                                    prob.adv_dev, prob.ret_dev, prob.old_dev, prob.idx_dev)
        torch.cuda.synchronize()
        start, end, n_steps = prob.p0, net.params.clone(), 1
        loss = float(loss.item())
    else:
        assert not p.gather
        # rows 0 .. M-1 are the tail; 32 more samples in front of them
        ids = torch.cat([torch.arange(p.M, p.M + 32), torch.arange(p.M)]).to(
            torch.int32).to(prob.dev)
        a, keep, _ = algo._update_args(prob.opt, prob.module, prob.kind, prob.batch,
                                       prob.adv_dev, prob.ret_dev, prob.old_dev, 0,
                                       rows=32)
        losses = torch.full((2, ), NAN, device=prob.dev)
        res = []
        for S in (32, 32 + p.M):
            prob.reset()
            a.S, a.mb, a.n_mb, a.perm = S, 32, 0, ids.data_ptr()
            a.phase, a.step0, a.losses = 0, 0, losses.data_ptr()
            call('ga_update_epoch', C.byref(a), stream_ptr())
            torch.cuda.synchronize()
            res.append(net.params.clone())
        del keep
        start, end, n_steps = res[0], res[1], 3
        loss = float(losses[1].item())
    after = _counts(lib)
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (
        0, 0, n_steps)
    u = start.double() - end.double()
    assert float(u.abs().max()) < 1.0
    g = u / (1.0 - u.abs())
    ulp = torch.from_numpy(np.spacing(torch.maximum(start.abs(), end.abs()).cpu().numpy()))
    widen = (ulp.double() * (1.0 + g.abs().cpu()) ** 2)
    return loss, g.float(), start, widen


@pytest.mark.parametrize('p', SMALL, ids=pc.case_id)
def test_small_step_path(dev, p):
    from garage_amd import _lib
    lib = _lib.load()
    opt = (torch.optim.Adam, dict(lr=1.0, betas=(0.0, 0.0), eps=1.0))
    prob = _Problem(p, dev, opt, lead=32 if p.M < 32 else 0)
    failures = []
    _switches(lib)
    loss, flat, start, widen = _small_step(prob, lib)
    ref_loss, ref = prob.reference(start)
    extra = OrderedDict((key, view.numpy().reshape(ref[key].shape))
                        for key, view in prob.net.named_views(widen))
    assert max(float(v.max()) for v in extra.values()) < oc.TOL_GRAD
    _compare(prob, 'small step', loss, flat, ref_loss, ref, failures, extra)
    if not p.learn_std or p.kind == 'cat':
        assert prob.net.params[0].item() == prob.p0[0].item()
    assert not failures, failures
