"""``fwd_dgrad_kernel``'s addressing and epilogue order against the two-launch path.

The fused launch (fused_train.hip) reaches W2, this layer's weights, H1 and dZ2 through
buffer descriptors with scalar offsets, and issues its dZ2 stores before the head's weight
gradient, keeping the quads in registers until the staged activation has been read.
Neither changes an operation or its order: one optimizer step through
``ga_update_epoch`` with ``ga_set_fused_fwd_dgrad(1)`` must leave the BITS that the
forward + loss launch and the data-gradient launch leave with the switch off -- in H1,
dZ2, the head / first-layer / loss partials, the reduced gradient, the parameters and both
Adam moments -- and must write nowhere else: every buffer the step writes lies between
guard bands and is filled with NaN beforehand (the workspaces have rows beyond M), and
what no kernel owns must still be NaN afterwards.

Shapes, the smallest at which an address or the reordering can go wrong: M of 1, 63, 64,
65, 130 and 200 rows (a lone row, ragged last tiles, one to four tiles) at every width the
kernel is compiled for (64, 128, 256), first layers of 4, 17, 20 and 32 inputs (the
``KSC = 5`` loop at 17 and 20 inputs and 256 units, the plain loop elsewhere; 32 inputs
fit the kernel's first-layer stage at 64 and 128 units only), heads of 1 (the value
function), 4 and 6 outputs (the epilogue's three instantiations), rows gathered through an
index and not.  The observation and action rows are further apart than they are wide, with
NaN between them.  The strides of H1, dZ2 and the weights are not a caller's to choose
here: ``ga_update_epoch`` lays them out at the layers' widths
(tests/test_fused_entries_strides_gpu.py runs the entry points themselves on wider rows).

What the two-launch path is a reference FOR: the staged data-gradient loop's W2 loads, the
reordered epilogue and its dZ2 stores exist in the fused kernel only, and the two launches
check them independently.  The forward k-loop (its weight-fragment loads and H1 spill
stores) is one body that both paths run: there the comparison cannot see a wrong offset.
That loop is held by the finite / NaN row checks below, by H1 against fp64 in the strides
test, and by the suite's parity tests of the fused forward against torch and the
per-layer path (test_fused_train_gpu.py, test_loss_paths_fp64_gpu.py).

(The NaN fills are zeroed at the end of every case: left in freed memory they reach tests
that compare rows nobody wrote.)
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64  # floats in front of and behind every buffer
FUSED_FWD, FUSED_DGRAD = 9, 10  # prof.h: GA_PROF_FUSED_FWD, GA_PROF_FUSED_DGRAD
N_KINDS = 16
MS = (1, 63, 64, 65, 130, 200)
INPUTS = {64: (4, 17, 20, 32), 128: (4, 17, 20, 32), 256: (4, 17, 20)}
HEADS = (1, 4, 6)


def _cases():
    """Every (width, M) twice: inputs, head width and gathering rotate against each other
    so that each value meets each width and both kinds of last tile."""
    out = []
    for wi, width in enumerate((64, 128, 256)):
        ins = INPUTS[width]
        for sweep in (0, 1):
            for i, m in enumerate(MS):
                out.append((width, m, ins[(i + wi + 2 * sweep) % len(ins)],
                            HEADS[(i + sweep) % 3], (i + sweep) % 2 == 0))
    # the bench's kernel and head pair at a ragged tile, both ways of addressing the rows
    out += [(256, 200, 17, 6, True), (256, 200, 17, 1, False)]
    return sorted(set(out))


def _r4(n):
    return (n + 3) & ~3


class _Guarded:
    """A float buffer of ``n`` elements between two guard bands, everything NaN."""

    def __init__(self, n, dev, init=None):
        self.n = n
        self.t = torch.full((n + 2 * GUARD, ), NAN, dtype=torch.float32, device=dev)
        if init is not None:
            self.body().copy_(init)

    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def guards_intact(self):
        return bool(torch.isnan(self.t[:GUARD]).all()) and bool(
            torch.isnan(self.t[GUARD + self.n:]).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _step(case, on):
    """One optimizer step of the case's network on its minibatch -> the buffers."""
    from garage_amd import _lib
    from garage_amd._dtypes import Box, EnvSpec
    from garage_amd.algos import PPO
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy, GaussianMLPValueFunction
    lib = _lib.load()
    width, M, O, A, gather = case
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(1000 * width + 7 * M + O + A)
    spec = EnvSpec(Box(-np.inf, np.inf, (O, )), Box(-np.inf, np.inf, (max(A, 2), )),
                   max_episode_length=10)
    torch.manual_seed(3)
    pol = GaussianMLPPolicy(spec, hidden_sizes=(width, width))
    vf = GaussianMLPValueFunction(spec, hidden_sizes=(width, width))
    opt = (torch.optim.Adam, dict(lr=1e-3))
    algo = PPO(env_spec=spec, policy=pol, value_function=vf, sampler=None,
               policy_optimizer=OptimizerWrapper(opt, pol),
               vf_optimizer=OptimizerWrapper(opt, vf))
    # a head of one output is the value function's; 4 and 6 are Gaussian policies
    module, wrapper, kind = ((vf, algo._vf_optimizer, 1) if A == 1 else
                             (pol, algo._policy_optimizer, 0))
    net = module.net
    assert tuple(net.dims) == (O, width, width, A)
    g = torch.Generator(device='cpu').manual_seed(5)
    for l in range(3):
        net.bias(l).copy_(0.1 * torch.randn(net.dims[l + 1], generator=g))
    net.params[0] = -0.3
    # the pool of samples: rows ldx / lda apart, NaN between the padded rows
    pool = M + 9 if gather else M
    ldx, lda = _r4(O) + 8, _r4(A) + 4
    X = torch.full((pool, ldx), NAN)
    X[:, :_r4(O)] = 0.
    X[:, :O] = torch.from_numpy(rng.randn(pool, O).astype(np.float32))
    acts = torch.full((pool, lda), NAN)
    acts[:, :_r4(A)] = 0.
    acts[:, :A] = torch.from_numpy(rng.randn(pool, A).astype(np.float32))
    X, acts = X.to(dev), acts.to(dev)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    adv, ret = up(0.5 + rng.randn(pool)), up(rng.randn(pool))
    # old log-likelihoods within a few percent of the current ones: ratios inside PPO's
    # clip range, so that the rows carry a gradient
    with torch.no_grad():
        h = X[:, :O]
        for l in range(3):
            h = h @ net.weight(l).T + net.bias(l)
            h = torch.tanh(h) if l < 2 else h
        std = float(np.exp(-0.3))
        ll = (-0.5 * ((acts[:, :A] - h) / std) ** 2 - np.log(std) -
              0.5 * np.log(2 * np.pi)).sum(1)
    old = (ll + up(0.05 * rng.randn(pool))).contiguous()
    idx = None
    if gather:
        idx = torch.from_numpy(rng.permutation(pool)[:M].astype(np.int32)).to(dev)
    batch = types.SimpleNamespace(n_samples=M, obs_dev=X[:, :_r4(O)],
                                  actions_dev=acts[:, :_r4(A)])
    cap = M + 3  # rows of the workspaces: three that no kernel owns
    a, keep, _ = algo._update_args(wrapper, module, kind, batch, adv, ret, old, 0, rows=cap)
    assert a.ldx == ldx and (kind == 1 or a.lda == lda)
    floats = int(lib.ga_update_partials_floats(a.desc, M))
    assert floats > 0
    buf = dict(acts=_Guarded(2 * cap * width, dev), dacts=_Guarded(2 * cap * width, dev),
               partials=_Guarded(floats, dev), grads=_Guarded(net.n_flat, dev),
               params=_Guarded(net.n_flat, dev, net.params),
               exp_avg=_Guarded(net.n_flat, dev, net.exp_avg),
               exp_avg_sq=_Guarded(net.n_flat, dev, net.exp_avg_sq),
               losses=_Guarded(1, dev))
    try:
        a.acts, a.dacts = buf['acts'].ptr(), buf['dacts'].ptr()
        a.partials, a.partials_floats = buf['partials'].ptr(), floats
        a.params, a.grads = buf['params'].ptr(), buf['grads'].ptr()
        a.exp_avg, a.exp_avg_sq = buf['exp_avg'].ptr(), buf['exp_avg_sq'].ptr()
        a.losses = buf['losses'].ptr()
        a.S, a.mb, a.n_mb = M, M, 0
        a.perm = None if idx is None else idx.data_ptr()
        a.phase, a.step0 = 0, 0
        n0 = [int(lib.ga_launch_count(k)) for k in (FUSED_FWD, FUSED_DGRAD)]
        lib.ga_set_fused_fwd_dgrad(on)
        lib.ga_prof_enable(1)
        try:
            _lib.call('ga_update_epoch', C.byref(a), _lib.stream_ptr())
            torch.cuda.synchronize()
        finally:
            lib.ga_prof_enable(0)
            prof = (C.c_double * (3 * N_KINDS))()
            lib.ga_prof_collect(prof, N_KINDS)
        steps = [int(lib.ga_launch_count(k)) - n for k, n in zip((FUSED_FWD, FUSED_DGRAD), n0)]
        timed = [int(prof[3 * k + 2]) for k in (FUSED_FWD, FUSED_DGRAD)]
        out = {k: b.body().clone() for k, b in buf.items()}
        intact = {k: b.guards_intact() for k, b in buf.items()}
    finally:
        for b in buf.values():
            b.t.zero_()
        X.zero_()
        acts.zero_()
        torch.cuda.synchronize()
    del keep
    return out, intact, steps, timed, cap, net


@pytest.fixture(scope='module')
def switches():
    from garage_amd import _lib
    lib = _lib.load()
    # the wide step's kernels at 64 units and at 64 rows or fewer
    lib.ga_set_narrow_step(0)
    lib.ga_set_small_step(0)
    yield lib
    lib.ga_set_narrow_step(1)
    lib.ga_set_small_step(1)
    lib.ga_set_fused_fwd_dgrad(1)


@pytest.mark.parametrize('case', _cases(),
                         ids=lambda c: 'w%d_m%d_in%d_a%d_%s' % (c[:4] + ('idx' if c[4] else
                                                                         'lin', )))
def test_fused_launch_leaves_the_two_launches_bits_and_nothing_else(switches, case):
    width, M, O, A, gather = case
    try:
        new, intact, steps, timed, cap, net = _step(case, 1)
        ref, ref_intact, ref_steps, ref_timed, _, _ = _step(case, 0)
    finally:
        switches.ga_set_fused_fwd_dgrad(1)
    # which kernels ran: both counters advance once per network step either way, but only
    # a launch of its own is timed -- the fused launch is timed as the forward's
    assert steps == [1, 1] and timed == [1, 0], (steps, timed)
    assert ref_steps == [1, 1] and ref_timed == [1, 1], (ref_steps, ref_timed)
    # no stray store: the guard bands, the workspace rows beyond M and the regions of the
    # activations no kernel stores (H2 and dZ1 stay on the CU)
    assert all(intact.values()), intact
    assert all(ref_intact.values()), ref_intact
    h1 = new['acts'][:cap * width].view(cap, width)
    dz2 = new['dacts'][cap * width:].view(cap, width)
    for name, t in (('H1', h1), ('dZ2', dz2)):
        assert bool(torch.isfinite(t[:M]).all()), name
        assert bool(torch.isnan(t[M:]).all()), name + ': a store beyond row M'
    assert bool(torch.isnan(new['acts'][cap * width:]).all()), 'H2 region written'
    assert bool(torch.isnan(new['dacts'][:cap * width]).all()), 'dZ1 region written'
    # the same bits as the two launches, NaN fills included
    for key in ('acts', 'dacts', 'partials', 'grads', 'params', 'exp_avg', 'exp_avg_sq',
                'losses'):
        same = torch.equal(_bits(new[key]), _bits(ref[key]))
        if not same:
            d = (_bits(new[key]) != _bits(ref[key])).nonzero().flatten()
            print('%s: %d of %d words differ, first at %s' % (key, d.numel(),
                                                              new[key].numel(), d[:8].tolist()))
        assert same, key
    for key in ('params', 'exp_avg', 'exp_avg_sq', 'losses'):
        assert bool(torch.isfinite(new[key]).all()), key
    # (the flat layout pads its slots to quads: the gradient's padding words are nobody's)
    for key, view in net.named_views(new['grads']):
        assert bool(torch.isfinite(view).all()), 'gradient of ' + key
    # (the rows carried a gradient)
    assert bool((dz2[:M] != 0).any()) and bool((new['exp_avg_sq'][1:] > 0).any())
