"""The ``ga_*_members_f32`` entry points, called directly, against the lone entry
points on the same inputs member by member: ``ga_mlp_forward_f32``,
``ga_ppo_gaussian_loss_f32``, ``ga_ppo_categorical_loss_f32``, ``ga_gaussian_kl_f32``,
``ga_categorical_kl_f32``, ``ga_gaussian_nll_loss_f32``, ``ga_episode_sums_f32``.
Outputs bit for bit; every written array lies inside a tensor of sentinels that must
survive; the per-member losses also against the fp64 references and tolerances of
``_loss_cases`` (a mistake both paths shared would pass the first check).

M in {1, 2, 5}, rows per member from {1, 255, 256, 257, 1000} mixed within a call
(both sides of one 256-row block and of the forward kernels' tiles); input widths
1, 4, 32; hidden 32 and 64; outputs 1, 3, 8; row strides wider than the width.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _loss_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 32
ROWS = {1: [257], 2: [1, 1000], 5: [1, 255, 256, 257, 1000]}


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda')


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


class Guarded:
    """``n`` elements inside a tensor of sentinels."""

    def __init__(self, n, dtype, dev, fill=None):
        self.full = torch.full((n + 2 * PAD, ), SENTINEL, dtype=dtype, device=dev)
        self.t = self.full[PAD:PAD + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def intact(self):
        return bool((self.full[:PAD] == SENTINEL).all()) and \
            bool((self.full[-PAD:] == SENTINEL).all())


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _randn(rng, *shape):
    return torch.from_numpy(rng.randn(*shape).astype(np.float32))


def _strided(src, ld, dev):
    """[rows, width] values at row stride ``ld``, sentinels between the rows."""
    rows, width = src.shape
    g = Guarded(rows * ld, torch.float32, dev)
    g.t.view(rows, ld)[:, :width] = src.to(dev)
    return g


def _rows_intact(g, rows, ld, width):
    """The gaps between the rows of a strided array hold sentinels still."""
    if ld == width:
        return True
    return bool((g.t.view(rows, ld)[:, width:] == SENTINEL).all())


def _partials(rows, dev, per=2):
    from garage_amd import _lib
    arr = (C.c_int64 * len(rows))(*rows)
    need = int(_lib.load().ga_members_diag_partials_doubles(arr, len(rows)))
    assert need == 2 * sum(max(1, -(-r // 256)) for r in rows)
    return Guarded(need * per // 2, torch.float64, dev), need * per // 2


# ---- forward ---------------------------------------------------------------------------
@pytest.mark.parametrize('M', sorted(ROWS))
@pytest.mark.parametrize('in_dim,hidden,out_dim', [(1, 32, 1), (4, 64, 3), (32, 64, 8),
                                                   (4, 32, 8), (32, 32, 3)])
def test_forward_members_equals_lone_forwards(dev, in_dim, hidden, out_dim, M):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.engine import FlatMLP, round4
    rows = ROWS[M]
    net = FlatMLP(in_dim, out_dim, (hidden, hidden), dev)
    ldx, ldo, aw = round4(in_dim) + 4, round4(out_dim) + 4, 2 * round4(hidden)
    rng = _rng('fwd', in_dim, hidden, out_dim, M)
    params = [(0.3 * _randn(rng, net.n_flat)).to(dev) for _ in rows]
    X = [_strided(_randn(rng, r, in_dim), ldx, dev) for r in rows]
    joint = [(Guarded(r * aw, torch.float32, dev), Guarded(r * ldo, torch.float32, dev))
             for r in rows]
    lone = [(Guarded(r * aw, torch.float32, dev), Guarded(r * ldo, torch.float32, dev))
            for r in rows]
    arr = (_lib.MemberForward * M)()
    for m, r in enumerate(rows):
        u = arr[m]
        u.params, u.X, u.ldx, u.rows = params[m].data_ptr(), X[m].t.data_ptr(), ldx, r
        u.acts, u.out, u.ldo = joint[m][0].t.data_ptr(), joint[m][1].t.data_ptr(), ldo
    call('ga_mlp_forward_members_f32', C.byref(net._desc), arr, M, stream_ptr())
    for m, r in enumerate(rows):
        desc = _lib.MlpDesc.from_buffer_copy(net._desc)
        desc.act_off[0], desc.act_off[1] = 0, round4(hidden) * r
        call('ga_mlp_forward_f32', C.byref(desc), dptr(params[m]), dptr(X[m].t), ldx,
             None, r, dptr(lone[m][0].t), dptr(lone[m][1].t), ldo, stream_ptr())
    torch.cuda.synchronize()
    for m, r in enumerate(rows):
        got = joint[m][1].t.view(r, ldo)[:, :out_dim]
        want = lone[m][1].t.view(r, ldo)[:, :out_dim]
        assert torch.equal(_bits(got), _bits(want)), m
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        # the hidden activations too, and everything around what was written
        assert torch.equal(_bits(joint[m][0].t), _bits(lone[m][0].t)), m
        assert torch.equal(_bits(joint[m][1].t), _bits(lone[m][1].t)), m
        for g in joint[m] + (X[m], ):
            assert g.intact(), m
        assert _rows_intact(joint[m][1], r, ldo, out_dim)
        # fp64 of the same network (tanh hidden layers, linear head)
        h = X[m].t.view(r, ldx)[:, :in_dim].double()
        p = params[m].double()
        for l in range(3):
            W = p[net.w_off[l]:net.w_off[l] + net.dims[l + 1] * round4(net.dims[l])]
            W = W.view(net.dims[l + 1], round4(net.dims[l]))[:, :net.dims[l]]
            h = h @ W.t() + p[net.b_off[l]:net.b_off[l] + net.dims[l + 1]]
            if l < 2:
                h = torch.tanh(h)
        # (_mlp_option_cases.TOL_FORWARD's figure: 5e-6 of max(1, max |ref|))
        tol = 5e-6 * max(1.0, float(h.abs().max()))
        assert float((got.double() - h).abs().max()) <= tol, m
    if M > 1:  # the members are different problems
        assert not torch.equal(joint[0][1].t[:out_dim], joint[1][1].t[:out_dim])


# ---- policy losses ---------------------------------------------------------------------
def _loss_inputs(kind, A, rows, dev, rng):
    """Per member: head outputs, actions, old log-likelihoods, advantages."""
    ld, lda = (A + 3) // 4 * 4 + 4, (A + 3) // 4 * 4 + 8
    out = []
    for r in rows:
        head = _randn(rng, r, A)
        if kind == 'cat':
            acts = torch.from_numpy(rng.randint(0, A, size=(r, 1)).astype(np.float32))
        else:
            acts = head + 0.5 * _randn(rng, r, A)
        out.append(dict(head=head, actions=acts, old_ll=-1.0 + 0.1 * _randn(rng, r),
                        adv=_randn(rng, r), ld=ld, lda=lda if kind != 'cat' else 5))
    return out


@pytest.mark.parametrize('M', sorted(ROWS))
@pytest.mark.parametrize('kind,A,algo,ent_flags,std', [
    ('gauss', 1, 0, 0, 'plain'), ('gauss', 3, 0, 1, 'clamped'),
    ('gauss', 8, 1, 3, 'softplus'), ('cat', 3, 0, 1, None), ('cat', 8, 0, 7, None),
    ('cat', 2, 1, 0, None)])
def test_loss_members_equals_lone_losses(dev, kind, A, algo, ent_flags, std, M):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.engine import reduction_workspace
    rows = ROWS[M]
    rng = _rng('loss', kind, A, algo, ent_flags, M)
    ins = _loss_inputs(kind, A, rows, dev, rng)
    # (has_min | softplus bit, min, has_max, max) and the fp64 reference's options
    std_args, lo, hi, sp = {
        None: ((0, 0.0, 0, 0.0), None, None, False),
        'plain': ((0, 0.0, 0, 0.0), None, None, False),
        'clamped': ((1, -0.5, 1, 0.25), -0.5, 0.25, False),
        'softplus': ((3, -1.0, 0, 0.0), -1.0, None, True)}[std]
    dsm = int(kind == 'cat' and A != 2)
    clips = [float(np.float32(0.1 + 0.05 * m)) for m in range(M)]
    coeffs = [float(np.float32(0.01 * (m + 1))) for m in range(M)]
    log_std = [torch.tensor([0.4 - 0.3 * m, 0, 0, 0], dtype=torch.float32, device=dev)
               for m in range(M)]
    heads = [_strided(i['head'], i['ld'], dev) for i in ins]
    acts = [_strided(i['actions'], i['lda'], dev) for i in ins]
    old_ll = [i['old_ll'].to(dev) for i in ins]
    adv = [i['adv'].to(dev) for i in ins]
    loss = Guarded(M, torch.float32, dev)
    ent = Guarded(M, torch.float64, dev)
    part, need = _partials(rows, dev)
    a = _lib.MembersLossArgs()
    a.kind, a.A, a.algo, a.ent_flags = (2 if kind == 'cat' else 0), A, algo, ent_flags
    a.has_min, a.min_log_std, a.has_max, a.max_log_std = std_args
    a.double_softmax = dsm
    arr = (_lib.MemberLoss * M)()
    for m, r in enumerate(rows):
        u = arr[m]
        u.head, u.ld = heads[m].t.data_ptr(), ins[m]['ld']
        u.actions, u.lda = acts[m].t.data_ptr(), ins[m]['lda']
        u.old_ll = None if algo == 1 else old_ll[m].data_ptr()
        u.adv, u.log_std, u.rows = adv[m].data_ptr(), log_std[m].data_ptr(), r
        u.clip, u.ent_coeff = clips[m], coeffs[m]
        u.loss_out = loss.t[m:].data_ptr()
        u.ent_sum_out = ent.t[m:].data_ptr() if kind == 'cat' else None
    call('ga_ppo_loss_members_f32', C.byref(a), arr, M, dptr(part.t), need, stream_ptr())
    ws = reduction_workspace(dev)
    want = torch.zeros(M, dtype=torch.float32, device=dev)
    want_ent = torch.zeros(M, dtype=torch.float64, device=dev)
    for m, r in enumerate(rows):
        o = None if algo == 1 else dptr(old_ll[m])
        if kind == 'cat':
            call('ga_ppo_categorical_loss_f32', dptr(heads[m].t), ins[m]['ld'],
                 dptr(acts[m].t), ins[m]['lda'], o, dptr(adv[m]), None, r, A, dsm, algo,
                 clips[m], coeffs[m], ent_flags, None, None, None, dptr(want[m:]),
                 dptr(want_ent[m:]), None, 0, 0, dptr(ws), stream_ptr())
        else:
            call('ga_ppo_gaussian_loss_f32', dptr(heads[m].t), ins[m]['ld'],
                 dptr(acts[m].t), ins[m]['lda'], o, dptr(adv[m]), None,
                 dptr(log_std[m]), *std_args, r, A, algo, clips[m], coeffs[m],
                 ent_flags, None, None, dptr(want[m:]), None, 0, 0, dptr(ws),
                 stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(loss.t), _bits(want))
    assert loss.intact() and ent.intact() and part.intact()
    if kind == 'cat':
        assert torch.equal(_bits(ent.t), _bits(want_ent))
    else:
        assert bool((ent.t == SENTINEL).all())
    assert len({float(x) for x in want.cpu()}) == M
    # ... and both against fp64
    case = lc.Case(kind, A, max(rows), False, 'wide', algo, clips[0], ent_flags, None,
                   'randn', dsm, 0)
    for m, r in enumerate(rows):
        o = lc.Opt(lo, hi, sp, algo, clips[m], ent_flags, coeffs[m], dsm)
        head = ins[m]['head'].double()
        if kind == 'cat':
            dist, actions = lc.categorical(head, o), ins[m]['actions'][:, 0].double()
        else:
            dist = lc.gaussian(head, log_std[m][:1].cpu().double(), o)
            actions = ins[m]['actions'].double()
        ref, _, ent_rows = lc.policy_loss(dist, actions, ins[m]['old_ll'].double(),
                                          ins[m]['adv'].double(), o)
        ref = ref.numpy()
        assert abs(float(loss.t[m]) - float(ref)) <= lc.tolerance(case, 'loss', ref), m
        if kind == 'cat':
            ref = ent_rows.sum().numpy()
            assert abs(float(ent.t[m]) - float(ref)) <= lc.tolerance(
                case, 'ent_sum', ref), m


# ---- KL --------------------------------------------------------------------------------
@pytest.mark.parametrize('M', sorted(ROWS))
@pytest.mark.parametrize('categorical,A', [(0, 1), (0, 3), (0, 8), (1, 3), (1, 8)])
def test_kl_members_equals_lone_kls(dev, categorical, A, M):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.engine import reduction_workspace
    from torch.distributions import kl_divergence
    rows = ROWS[M]
    rng = _rng('kl', categorical, A, M)
    ld = (A + 3) // 4 * 4 + 4
    old = [_randn(rng, r, A) for r in rows]
    new = [_randn(rng, *o.shape) for o in old]  # (far apart: a well-conditioned KL)
    g_old = [_strided(o, ld, dev) for o in old]
    g_new = [_strided(n, ld, dev) for n in new]
    s_old = [float(np.float32(0.1 * m)) for m in range(M)]
    s_new = [float(np.float32(0.1 * m - 0.05)) for m in range(M)]
    dsm = int(categorical and A == 8)
    out = Guarded(M, torch.float64, dev)
    part, need = _partials(rows, dev, per=1)
    arr = (_lib.MemberKl * M)()
    for m, r in enumerate(rows):
        u = arr[m]
        u.head_old, u.head_new = g_old[m].t.data_ptr(), g_new[m].t.data_ptr()
        u.ld, u.rows, u.log_std_old, u.log_std_new = ld, r, s_old[m], s_new[m]
        u.kl_sum_out = out.t[m:].data_ptr()
    call('ga_kl_members_f32', categorical, A, dsm, arr, M, dptr(part.t), need,
         stream_ptr())
    ws = reduction_workspace(dev)
    want = torch.zeros(M, dtype=torch.float64, device=dev)
    for m, r in enumerate(rows):
        if categorical:
            call('ga_categorical_kl_f32', dptr(g_old[m].t), dptr(g_new[m].t), ld, r, A,
                 dsm, dptr(want[m:]), dptr(ws), stream_ptr())
        else:
            call('ga_gaussian_kl_f32', dptr(g_old[m].t), dptr(g_new[m].t), ld, r, A,
                 s_old[m], s_new[m], dptr(want[m:]), dptr(ws), stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.t), _bits(want))
    assert out.intact() and part.intact()
    assert len({float(x) for x in want.cpu()}) == M
    case = lc.Case('cat' if categorical else 'gauss', A, max(rows), False, 'wide', 0,
                   0.2, 0, None, 'randn', dsm, 0)
    for m in range(M):
        o = lc.Opt(None, None, False, 0, 0.2, 0, 0.0, dsm)
        if categorical:
            d_old, d_new = (lc.categorical(x[m].double(), o) for x in (old, new))
        else:
            d_old = lc.gaussian(old[m].double(), torch.tensor([s_old[m]]).double(), o)
            d_new = lc.gaussian(new[m].double(), torch.tensor([s_new[m]]).double(), o)
        ref = kl_divergence(d_old, d_new).sum().numpy()
        assert abs(float(out.t[m]) - float(ref)) <= lc.tolerance(case, 'kl', ref), m


# ---- value loss ------------------------------------------------------------------------
@pytest.mark.parametrize('M', sorted(ROWS))
def test_nll_members_equals_lone_losses(dev, M):
    from garage_amd import _lib
    from garage_amd._lib import call, dptr, stream_ptr
    from garage_amd.engine import reduction_workspace
    rows = ROWS[M]
    rng = _rng('nll', M)
    ldv = 8
    v = [_randn(rng, r, 1) for r in rows]
    ret = [x[:, 0] + 0.3 * _randn(rng, len(x)) for x in v]
    g_v = [_strided(x, ldv, dev) for x in v]
    d_ret = [x.to(dev) for x in ret]
    log_std = [torch.tensor([0.2 * m - 0.3, 0, 0, 0], dtype=torch.float32, device=dev)
               for m in range(M)]
    out = Guarded(M, torch.float32, dev)
    part, need = _partials(rows, dev)
    arr = (_lib.MemberNll * M)()
    for m, r in enumerate(rows):
        u = arr[m]
        u.v, u.ldv, u.returns = g_v[m].t.data_ptr(), ldv, d_ret[m].data_ptr()
        u.log_std, u.rows, u.loss_out = log_std[m].data_ptr(), r, out.t[m:].data_ptr()
    call('ga_gaussian_nll_members_f32', arr, M, dptr(part.t), need, stream_ptr())
    ws = reduction_workspace(dev)
    want = torch.zeros(M, dtype=torch.float32, device=dev)
    for m, r in enumerate(rows):
        call('ga_gaussian_nll_loss_f32', dptr(g_v[m].t), ldv, dptr(d_ret[m]), None,
             dptr(log_std[m]), r, None, dptr(want[m:]), None, 0, 0, dptr(ws),
             stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.t), _bits(want))
    assert out.intact() and part.intact()
    assert len({float(x) for x in want.cpu()}) == M
    case = lc.Case('nll', 1, max(rows), False, 'wide', 0, 0.2, 0, None, 'randn', 0, 0)
    for m in range(M):
        ref = lc.value_loss(v[m].double(), log_std[m][:1].cpu().double(),
                            ret[m].double()).numpy()
        assert abs(float(out.t[m]) - float(ref)) <= lc.tolerance(case, 'loss', ref), m


# ---- log_performance ---------------------------------------------------------------------
@pytest.mark.parametrize('M', sorted(ROWS))
def test_episode_stats_members_equals_the_lone_passes(dev, M):
    from garage_amd import _lib
    from garage_amd._dtypes import StepType
    from garage_amd._lib import call, dptr, stream_ptr
    n_eps = {1: [300], 2: [1, 257], 5: [1, 2, 255, 256, 7]}[M]
    rng = _rng('episodes', M)
    term = int(StepType.TERMINAL)
    outs, wants, keep = [], [], []
    arr = (_lib.MemberEpisodes * M)()
    for m, n in enumerate(n_eps):
        lengths = rng.randint(1, 9, size=n)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)])).to(dev)
        S = int(off[-1])
        rewards, returns = _randn(rng, S).to(dev), _randn(rng, S).to(dev)
        st = torch.from_numpy(rng.randint(0, 4, size=S).astype(np.uint8)).to(dev)
        out = Guarded(3 * n, torch.float64, dev)
        u = arr[m]
        u.rewards, u.ep_off, u.n_eps = rewards.data_ptr(), off.data_ptr(), n
        u.returns, u.step_types, u.out = returns.data_ptr(), st.data_ptr(), \
            out.t.data_ptr()
        sums = torch.empty(n, dtype=torch.float64, device=dev)
        call('ga_episode_sums_f32', dptr(rewards), dptr(off), n, dptr(sums), stream_ptr())
        wants.append(torch.cat([sums, returns[off[:-1]].double(),
                                (st[off[1:] - 1] == term).double()]))
        outs.append(out)
        keep.append((off, rewards, returns, st))
    call('ga_episode_stats_members_f32', arr, M, term, stream_ptr())
    torch.cuda.synchronize()
    for m, (out, want) in enumerate(zip(outs, wants)):
        assert torch.equal(_bits(out.t), _bits(want)), m
        assert out.intact(), m
    flags = torch.cat([w[-n:] for w, n in zip(wants, n_eps)])
    assert bool(((flags == 0) | (flags == 1)).all())
    if M == 1:
        assert 0 < float(flags.sum()) < len(flags)
