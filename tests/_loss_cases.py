"""Case table and fp64 reference of the loss layer: the objective every update path
computes between the MLP passes and the optimizer.

Shared by ``test_loss_cases_cpu.py`` (is fp32 itself close enough to fp64 on these
cases, and does the reference say what ``oracle.networks`` says?),
``test_loss_entries_fp64_gpu.py`` (the loss entry points of the C ABI, called
directly) and ``test_loss_paths_fp64_gpu.py`` (every update path, network included).

One reference: plain torch under autograd, on float64 copies of fp32-representable
inputs, straight from the head outputs --

  Gaussian     ``Independent(Normal(mean, std), 1)``, ``std`` from the scalar
               parameter as ``oracle.networks.gaussian_dist`` derives it (clamp, then
               ``exp`` or ``exp().exp().add(1).log()``)
  categorical  ``Categorical(logits=scores)`` or ``Categorical(logits=softmax(scores))``
  value        ``-log_prob(returns).mean()``
  objectives   PPO's clipped surrogate (algo 0), VPG's ``ll * adv`` (1), TRPO's
               ``ratio * adv`` (2); entropy bits 0 regularized, 1 softplus, 2
               stop-gradient (``ent_flags`` of the C ABI)

For a case it yields ``loss``, ``ll``, ``ent`` / ``ent_sum`` (categorical), ``seed`` =
d loss / d head outputs, ``dlogstd`` = d loss / d log-std parameter, ``kl`` (the sum
over rows of KL(old || new) against a second set of head outputs), ``fisher`` (the
Hessian of the mean KL at old == new applied to a tangent, by double backward) and,
for the head-in-loss cases, ``head`` = H W^T + b.

The same formulas in fp32 on the CPU give ``dev32``, what fp32 arithmetic alone costs.
"""
import functools
import zlib
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Categorical, Independent, Normal, kl_divergence

# ---- the reference ---------------------------------------------------------------

# lo / hi: clamp of the log-std parameter (None: absent); softplus_std: the 'softplus'
# std parameterisation; algo / clip / ent_flags / coeff: the objective
Opt = namedtuple('Opt', 'lo hi softplus_std algo clip ent_flags coeff double_softmax')


def gaussian(mean, p, o):
    """The policy distribution from the means and the scalar parameter ``p`` ([1])."""
    log_std = torch.zeros_like(mean) + p
    if o.lo is not None or o.hi is not None:
        log_std = log_std.clamp(min=o.lo, max=o.hi)
    std = log_std.exp().exp().add(1.).log() if o.softplus_std else log_std.exp()
    return Independent(Normal(mean, std), 1)


def categorical(scores, o):
    return Categorical(
        logits=torch.softmax(scores, dim=-1) if o.double_softmax else scores)


def surrogate(ll, old_ll, adv, o):
    if o.algo == 1:
        return ll * adv
    ratio = (ll - old_ll).exp()
    if o.algo == 2:
        return ratio * adv
    return torch.min(ratio * adv, torch.clamp(ratio, 1 - o.clip, 1 + o.clip) * adv)


def policy_loss(dist, actions, old_ll, adv, o):
    """-> (loss, log-likelihoods, per-row entropies as the options shape them)."""
    ll = dist.log_prob(actions)
    obj = surrogate(ll, old_ll, adv, o)
    ent = dist.entropy()
    if o.ent_flags & 2:
        ent = F.softplus(ent)
    if o.ent_flags & 1:
        obj = obj + o.coeff * (ent.detach() if o.ent_flags & 4 else ent)
    return -obj.mean(), ll, ent


def value_loss(v, p, returns):
    """``v`` [M, 1]; the value function's log-std has no clamp."""
    dist = Independent(Normal(v, (torch.zeros_like(v) + p).exp()), 1)
    return -dist.log_prob(returns.reshape(-1, 1)).mean()


def fisher_seed(make_dist, head, tangent):
    """(d^2 / d head^2 of mean_i KL(dist(head_0) || dist(head))) tangent at
    head == head_0, by double backward."""
    h = head.detach().clone().requires_grad_(True)
    old = make_dist(head.detach())
    kl = kl_divergence(old, make_dist(h)).mean()
    g, = torch.autograd.grad(kl, h, create_graph=True)
    out, = torch.autograd.grad((g * tangent).sum(), h)
    return out


# ---- the table -------------------------------------------------------------------

# kind: 'gauss' / 'cat' / 'nll' (the stand-alone entries), 'hgauss' / 'hnll' (the head
# layer inside the loss kernel: hidden > 0)
# gather: rows are M draws with repeats from a pool of GATHER_POOL samples
# layout: 'tight' ld = lda = A; 'pad4' ld = lda = round4(A); 'wide' ld = round4(A) + 4
#         and lda = round4(A) + 8
# std: a key of LOG_STD; scores: 'randn' / 'shift' (+100 in every class) / 'x30'
Case = namedtuple('Case', 'kind A M gather layout algo clip ent_flags std scores dsm '
                          'hidden')

GATHER_M, GATHER_POOL = 1000, 1500
# the first row count at which the stand-alone kernels take two rows per thread
# (512 blocks of 256), and the head-in-loss kernels more than one chunk per block
BIG = 512 * 256 + 257
HEAD_BIG = 512 * 64 + 65
# the grid's boundaries of the two-phase entries (policy losses, value NLL): one block,
# two blocks (the first finalize launch), the first row count past the cap of 512 blocks
# (one thread, and only one, takes a second row)
CAPPED = 512 * 256 + 1
BOUNDARY_ROWS = (1, 257, CAPPED)
BOUNDARY_A = (1, 3)
ROWS = (1, 255, 256, 257, GATHER_M)
ENT_FLAGS = (0, 1, 3, 5, 7)
ENT_COEFF = 0.02
CLIP = float(np.float32(0.2))
CLIP_ONCE = float(np.float32(0.1))

# log-std parameter, lower clamp, upper clamp, softplus parameterisation (all exact
# in fp32)
LOG_STD = OrderedDict([
    ('free', (-0.3125, None, None, False)),
    ('lo_inactive', (-0.3125, float(np.float32(np.log(1e-6))), None, False)),
    ('lo_active', (-1.5, -0.5, None, False)),
    ('hi_active', (0.75, float(np.float32(np.log(1e-6))), 0.25, False)),
    ('at_lo', (-0.375, -0.375, None, False)),  # torch.clamp passes the gradient
    ('sp_free', (-0.3125, None, None, True)),
    ('sp_hi_active', (0.75, None, 0.25, True)),
])
ACTIVE = ('lo_active', 'hi_active', 'sp_hi_active')  # dlogstd == 0.0 exactly

GAUSS_A = (1, 2, 8, 9, 17, 32)
CAT_A = (2, 8, 9, 32)
SCORES = ('randn', 'shift', 'x30')
LAYOUTS = ('tight', 'pad4', 'wide')

# Both positions of ga_set_one_launch_losses for every launch of more than one block
ONE_LAUNCH = (0, 1)

HEAD_HIDDEN = (64, 128, 256, 512)
HEAD_A = (1, 6, 17)
HEAD_ROWS = (1, 63, 64, 65, GATHER_M)


def _cases():
    out = []
    # Gaussian: every width at every row count; algo, entropy flags, log-std mode and
    # layout walk with different periods (3, 5, 7, 3 -- k steps by 1 and there are
    # 5 row counts per width, so each width sees every flag set and each row count
    # every algo)
    k = 0
    for A in GAUSS_A:
        for M in ROWS[1:] + ROWS[:1] + ((BIG, ) if A <= 2 else ()):
            out.append(Case('gauss', A, M, M == GATHER_M, LAYOUTS[(k + k // 3) % 3],
                            k % 3, CLIP, ENT_FLAGS[k % 5],
                            list(LOG_STD)[k % 7], None, 0, 0))
            k += 1
    # named pairs the walk does not promise: the softplus entropy past its threshold
    # of 20 at A = 17 and 32 (with and without stop-gradient), below it at A = 9 at the
    # same options; clip 0.1; VPG and PPO at the large size
    out += [
        Case('gauss', 17, 257, False, 'wide', 0, CLIP, 3, 'sp_free', None, 0, 0),
        Case('gauss', 32, 257, False, 'wide', 0, CLIP, 7, 'free', None, 0, 0),
        Case('gauss', 32, 256, False, 'pad4', 1, CLIP, 3, 'lo_inactive', None, 0, 0),
        Case('gauss', 9, 257, False, 'wide', 0, CLIP, 3, 'sp_free', None, 0, 0),
        Case('gauss', 8, GATHER_M, True, 'wide', 0, CLIP_ONCE, 1, 'lo_inactive', None,
             0, 0),
        Case('gauss', 4, BIG, False, 'wide', 1, CLIP, 1, 'lo_inactive', None, 0, 0),
        Case('gauss', 3, BIG, False, 'tight', 0, CLIP, 0, 'free', None, 0, 0),
    ]
    # categorical: every (scores, double_softmax) at every width; rows, algo, flags
    # and layout walk.  A single row goes with the ordinary scores only: alone, a
    # saturated row's seed, KL and Fisher seed are all rounding (their own max |ref| is
    # ~1e-20), and the KL of one row of scores near 100 cancels to the rounding of 100
    k = 0
    for A in CAT_A:
        for sc in SCORES:
            for dsm in (1, 0):
                M = ROWS[k % 5] if sc == 'randn' else ROWS[1 + k % 4]
                out.append(Case('cat', A, M, M == GATHER_M, LAYOUTS[k % 3], (k // 2) % 3, CLIP,
                                ENT_FLAGS[(k + k // 5) % 5], None, sc, dsm, 0))
                k += 1
    out += [
        Case('cat', 2, BIG, False, 'pad4', 0, CLIP, 3, None, 'randn', 1, 0),
        Case('cat', 4, BIG, False, 'wide', 2, CLIP, 7, None, 'shift', 0, 0),
        Case('cat', 9, 257, False, 'wide', 0, CLIP, 5, None, 'randn', 1, 0),
        Case('cat', 8, GATHER_M, True, 'wide', 0, CLIP, 1, None, 'randn', 0, 0),
    ]
    # value NLL
    for k, M in enumerate(ROWS + (BIG, )):
        out.append(Case('nll', 1, M, M == GATHER_M, LAYOUTS[(k + 1) % 3], 0, CLIP, 0,
                        'free', None, 0, 0))
    # the grid's boundaries: each two-phase entry at every BOUNDARY_ROWS count with a width
    # of BOUNDARY_A (the rows the walks above do not already hold; a categorical head of
    # one class has nothing to compare, so it goes with 3; its single row takes the scores
    # as logits: the KL of ONE row of doubly-softmaxed scores is ~1e-3, and the fp32
    # formulas on the CPU are 1.4e-7 away from it, 1.7e-4 of the result)
    out += [
        Case('gauss', 1, CAPPED, False, 'tight', 0, CLIP, 1, 'lo_inactive', None, 0, 0),
        Case('gauss', 3, 1, False, 'wide', 0, CLIP, 1, 'free', None, 0, 0),
        Case('gauss', 3, 257, False, 'pad4', 2, CLIP, 5, 'at_lo', None, 0, 0),
        Case('gauss', 3, CAPPED, False, 'wide', 1, CLIP, 3, 'sp_free', None, 0, 0),
        Case('cat', 3, 1, False, 'tight', 0, CLIP, 1, None, 'randn', 0, 0),
        Case('cat', 3, 257, False, 'wide', 2, CLIP, 3, None, 'randn', 1, 0),
        Case('cat', 3, CAPPED, False, 'pad4', 0, CLIP, 5, None, 'randn', 1, 0),
        Case('nll', 1, CAPPED, False, 'wide', 0, CLIP, 0, 'free', None, 0, 0),
    ]
    # the head layer inside the loss kernel: every hidden width sees every row count
    # and every head width twice (the row counts shifted per width), A = 64 at 64
    # units, the grid-stride size at 64 units; options walk as above
    k = 0
    for hi, hidden in enumerate(HEAD_HIDDEN):
        for j in range(6):
            M = HEAD_ROWS[(j + hi) % 5]
            out.append(Case('hgauss', HEAD_A[j % 3], M, M == GATHER_M,
                            'wide' if k % 2 else 'pad4', k % 3, CLIP, ENT_FLAGS[k % 5],
                            list(LOG_STD)[k % 7], None, 0, hidden))
            k += 1
    out += [
        Case('hgauss', 64, 65, False, 'pad4', 0, CLIP, 3, 'lo_inactive', None, 0, 64),
        Case('hgauss', 64, GATHER_M, True, 'wide', 1, CLIP, 1, 'free', None, 0, 64),
        Case('hgauss', 6, HEAD_BIG, False, 'pad4', 0, CLIP, 1, 'lo_inactive', None, 0,
             64),
        Case('hgauss', 17, 63, False, 'wide', 2, CLIP, 7, 'sp_free', None, 0, 512),
    ]
    k = 0
    for hidden in HEAD_HIDDEN:
        for r in range(2):
            M = HEAD_ROWS[k % 5]
            out.append(Case('hnll', 1, M, M == GATHER_M, 'pad4' if k % 2 else 'wide',
                            0, CLIP, 0, 'free', None, 0, hidden))
            k += 1
    out += [
        Case('hnll', 1, 65, False, 'pad4', 0, CLIP, 0, 'free', None, 0, 512),
        Case('hnll', 1, 63, False, 'wide', 0, CLIP, 0, 'free', None, 0, 128),
        Case('hnll', 1, HEAD_BIG, False, 'wide', 0, CLIP, 0, 'free', None, 0, 64),
    ]
    dup = [c for c in out if out.count(c) > 1]
    assert not dup, dup
    return out


CASES = _cases()


def cases_of(*kinds):
    return [c for c in CASES if c.kind in kinds]


def case_id(c):
    bits = [c.kind, 'A%d' % c.A, 'M%d%s' % (c.M, 'g' if c.gather else ''), c.layout]
    if c.hidden:
        bits.insert(1, 'H%d' % c.hidden)
    if c.kind not in ('nll', 'hnll'):
        bits += ['algo%d' % c.algo, 'ent%d' % c.ent_flags]
        if c.clip != CLIP:
            bits.append('clip%.1f' % c.clip)
    if c.std is not None and c.kind not in ('nll', 'hnll'):
        bits.append(c.std)
    if c.kind == 'cat':
        bits += [c.scores, 'dsm%d' % c.dsm]
    return '-'.join(bits)


def strides(c):
    """(ld of the head outputs / seeds / tangents, lda of the actions)."""
    r4 = (c.A + 3) // 4 * 4
    return {'tight': (c.A, c.A), 'pad4': (r4, r4), 'wide': (r4 + 4, r4 + 8)}[c.layout]


def options(c):
    p, lo, hi, sp = LOG_STD[c.std] if c.std else (0.0, None, None, False)
    if c.kind in ('nll', 'hnll'):
        lo = hi = None
    return Opt(lo, hi, sp, c.algo, c.clip, c.ent_flags, ENT_COEFF, c.dsm)


def log_std_args(c):
    """(has_min, min_log_std, has_max, max_log_std) of the C ABI: bit 1 of has_min is
    the softplus parameterisation."""
    _, lo, hi, sp = LOG_STD[c.std]
    return ((0 if lo is None else 1) | (2 if sp else 0), 0.0 if lo is None else lo,
            0 if hi is None else 1, 0.0 if hi is None else hi)


# ---- tolerances --------------------------------------------------------------------
# Per tensor, relative to the tensor's own max |ref| (the seeds carry a factor 1 / M:
# an absolute bound would check nothing).  The project's figures:
#   loss                       rtol 1e-5, atol 1e-6
#   ll, ent                    1e-5 * max(1, max |ref|)
#   seed, dlogstd, fisher, kl,
#   ent_sum                    1e-5 * max |ref|
#   head (H W^T + b)           5e-6 * max(1, max |ref|), _mlp_option_cases.TOL_FORWARD
# test_loss_cases_cpu.py measures what fp32 alone costs (torch on the CPU, the same
# formulas); where a class exceeds half its figure there, the figure is replaced by
# twice the worst measured fp32 deviation (never more than CEILING, the loosest figure
# of the existing loss tests).  WIDENED: (class, kind, A) -> (bound, measured worst
# fp32 deviation), both relative to max |ref|.
CEILING = 1e-4
REL = {'loss': 1e-5, 'll': 1e-5, 'ent': 1e-5, 'seed': 1e-5, 'dlogstd': 1e-5,
       'fisher': 1e-5, 'kl': 1e-5, 'ent_sum': 1e-5, 'head': 5e-6}
WIDENED = {
    ('kl', 'cat', 32): (3.5e-5, 1.739e-5),      # shift, double softmax, M 255
    ('kl', 'cat', 2): (2.6e-5, 1.289e-5),       # one row
    ('dlogstd', 'hgauss', 64): (1.6e-5, 7.628e-6),  # PPO, 65 rows, most of them clipped
    ('fisher', 'cat', 9): (2.0e-5, 9.843e-6),   # saturated scores (x30)
    ('fisher', 'cat', 32): (1.5e-5, 7.394e-6),  # the same
    ('fisher', 'cat', 2): (1.5e-5, 7.351e-6),   # scores near 100
    ('fisher', 'cat', 4): (1.5e-5, 7.109e-6),   # the same
    ('seed', 'hgauss', 64): (1.1e-5, 5.438e-6),     # PPO: ll ~ -110 enters the ratio
    ('seed', 'gauss', 32): (1.3e-5, 6.455e-6),      # the same at ll ~ -55
    ('seed', 'hgauss', 17): (1.2e-5, 5.691e-6),     # TRPO: the same at ll ~ -30
}
CLIP_EDGE_MARGIN = CEILING  # no fp32 ratio can land on the other side of the kink
CLIP_EDGE_ROUNDS = 5


def rel_bound(c, name):
    b = WIDENED.get((name, c.kind, c.A), (REL[name], None))[0]
    assert b <= CEILING
    return b


def tolerance(c, name, ref):
    """The absolute bound for the result ``name`` of case ``c``."""
    scale = float(np.abs(ref).max()) if np.size(ref) else 0.0
    rel = rel_bound(c, name)
    if name == 'loss':
        return 1e-6 + rel * scale
    if name in ('ll', 'ent', 'head'):
        return rel * max(1.0, scale)
    return rel * scale


# ---- inputs ------------------------------------------------------------------------


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _dist_of(c, o, head, p):
    return categorical(head, o) if c.kind == 'cat' else gaussian(head, p, o)


def evaluate(c, inp, dtype):
    """Every compared quantity of the case in ``dtype`` -> {name: float64 numpy}."""
    o = options(c)
    t = lambda x: None if x is None else x.to(dtype)
    rows = None if inp['idx'] is None else torch.from_numpy(inp['idx']).long()
    take = lambda x: t(x) if rows is None else t(x)[rows]
    p = torch.tensor([inp['p']], dtype=dtype, requires_grad=True)
    res = OrderedDict()
    if c.hidden:
        H, W, b = t(inp['H']), t(inp['W']), t(inp['b'])
        head = take(H) @ W.t() + b
        res['head'] = head
        head = head.detach().requires_grad_(True)
    else:
        head = take(inp['head']).detach().requires_grad_(True)
    if c.kind in ('nll', 'hnll'):
        loss = value_loss(head, p, take(inp['returns']))
        res['loss'] = loss
        res['seed'], res['dlogstd'] = torch.autograd.grad(loss, [head, p])
    else:
        actions = take(inp['actions'])
        if c.kind == 'cat':
            actions = actions.long()
        old_ll = take(inp['old_ll']) if 'old_ll' in inp else None
        adv = take(inp['adv'])
        if old_ll is None:  # before the old log-likelihoods exist: ll only
            with torch.no_grad():
                return OrderedDict(ll=_dist_of(c, o, head, p).log_prob(actions).double()
                                   .numpy())
        loss, ll, ent = policy_loss(_dist_of(c, o, head, p), actions, old_ll, adv, o)
        res['loss'], res['ll'] = loss, ll
        if c.kind == 'cat':
            res['ent'], res['ent_sum'] = ent, ent.sum()
            res['seed'], = torch.autograd.grad(loss, [head])
        else:
            res['seed'], res['dlogstd'] = torch.autograd.grad(loss, [head, p])
        if not c.hidden:
            head2, tangent = take(inp['head2']), take(inp['tangent'])
            pd = p.detach()
            with torch.no_grad():
                if c.kind == 'cat':
                    # kl_divergence's own formula without its fp32 special case: where
                    # a class probability of `new` underflows to 0 and that of `old`
                    # does not, torch returns inf (the CPU test pins the two to each
                    # other in fp64, where neither underflows)
                    old, new = categorical(head, o), categorical(head2, o)
                    res['kl'] = (old.probs * (old.logits - new.logits)).sum()
                    if dtype == torch.float64:
                        res['kl_torch'] = kl_divergence(old, new).sum()
                else:
                    s_old, s_new = inp['s_old'], inp['s_new']
                    res['kl'] = kl_divergence(
                        Independent(Normal(head, torch.full_like(head, s_old).exp()), 1),
                        Independent(Normal(head2, torch.full_like(head2, s_new).exp()),
                                    1)).sum()
            res['fisher'] = fisher_seed(lambda h: _dist_of(c, o, h, pd), head, tangent)
    return OrderedDict((k, v.detach().to(torch.float64).numpy()) for k, v in res.items())


def edge_rows(c, ll64, old_ll):
    """Rows whose fp64 likelihood ratio lies within the margin of 1 - clip or
    1 + clip."""
    ratio = np.exp(ll64 - old_ll.astype(np.float64))
    bad = np.zeros(ratio.shape, dtype=bool)
    for edge in (1 - c.clip, 1 + c.clip):
        bad |= np.abs(ratio - edge) <= CLIP_EDGE_MARGIN * edge
    return bad


@functools.lru_cache(maxsize=None)
def build(c):
    """The inputs of ``c`` (fp32 tensors / numpy), its fp64 reference and its fp32
    deviation.  Results are shared: treat them as read-only.

    Gathered cases: every per-sample input has GATHER_POOL rows, ``idx`` (int32 [M],
    with repeats) names the sample of each minibatch row, and the pool rows no
    minibatch row names are NaN."""
    rng = _rng('loss', c)
    o = options(c)
    pool = GATHER_POOL if c.gather else c.M
    idx = rng.randint(0, pool, size=c.M).astype(np.int32) if c.gather else None
    used = np.ones(pool, dtype=bool)
    if idx is not None:
        used[:] = False
        used[idx] = True
    inp = dict(idx=idx, p=LOG_STD[c.std][0] if c.std else 0.0)
    A = c.A
    p64 = torch.tensor([inp['p']], dtype=torch.float64)
    if c.hidden:
        K = c.hidden
        inp['H'] = _f32(np.tanh(rng.randn(pool, K)))
        inp['W'] = _f32(rng.randn(A, K) / np.sqrt(K))
        inp['b'] = _f32(0.1 * rng.randn(A))
        head64 = inp['H'].double() @ inp['W'].double().t() + inp['b'].double()
    elif c.kind == 'cat':
        sc = rng.randn(pool, A)
        sc = sc + 100.0 if c.scores == 'shift' else (30.0 * sc if c.scores == 'x30'
                                                     else sc)
        inp['head'] = _f32(sc)
        head64 = inp['head'].double()
    else:
        inp['head'] = _f32(0.5 * rng.randn(pool, A))
        head64 = inp['head'].double()
    if c.kind in ('nll', 'hnll'):
        # (1.5 std of noise: the log-std gradient, mean(1 - z), is then about -1.25
        # and not a sum that cancels to ~ 1 / sqrt(M))
        std = float(np.exp(inp['p']))
        ret = head64[:, 0].numpy() + 1.5 * std * rng.randn(pool)
        inp['returns'] = _f32(ret)
    elif c.kind == 'cat':
        inp['actions'] = _f32(rng.randint(0, A, size=pool))
    else:
        # 1.25 std of noise and (below) advantages of mean 0.5: the log-std gradient,
        # -mean(g (q - A)), then has terms of one sign on average; with E q = A and
        # E adv = 0 it is a sum that cancels to ~ 1 / sqrt(M) of its terms, and its own
        # magnitude is no scale for what fp32 can hold
        std = gaussian(head64[:1], p64, o).stddev[0, 0].item()
        inp['actions'] = _f32(head64.numpy() + 1.25 * std * rng.randn(pool, A))
    rounds = 0
    if c.kind not in ('nll', 'hnll'):
        inp['adv'] = _f32(0.5 + rng.randn(pool))
        # old log-likelihoods: the fp32-rounded reference ones plus noise, no ratio on
        # a clip edge (rows are redrawn, never dropped)
        full = dict(inp, idx=None)
        ll64 = evaluate(c._replace(gather=False), full, torch.float64)['ll']
        ll32 = ll64.astype(np.float32)
        old = (ll32 + (0.3 * rng.randn(pool)).astype(np.float32)).astype(np.float32)
        while True:
            bad = edge_rows(c, ll64, old) & used
            if not bad.any() or rounds >= CLIP_EDGE_ROUNDS:
                break
            rounds += 1
            old[bad] = ll32[bad] + (0.3 * rng.randn(int(bad.sum()))).astype(np.float32)
        inp['edge_rows_left'] = int((edge_rows(c, ll64, old) & used).sum())
        inp['old_ll'] = _f32(old)
        if not c.hidden:
            if c.kind == 'cat':
                # another policy, not a small step: the KL of two close categorical
                # distributions is a sum of terms ~ delta that cancels to ~ delta^2,
                # which no fp32 evaluation holds to 1e-5 of the result
                scale = 30.0 if c.scores == 'x30' else 1.0
                inp['head2'] = _f32(inp['head'].numpy() + scale * rng.randn(pool, A))
            else:
                inp['head2'] = _f32(inp['head'].numpy() + 0.1 * rng.randn(pool, A))
                dist = gaussian(head64[:1], p64, o)
                inp['s_old'] = float(np.float32(dist.stddev[0, 0].log().item()))
                inp['s_new'] = float(np.float32(inp['s_old'] - 0.125))
            inp['tangent'] = _f32(rng.randn(pool, A))
    # the samples no minibatch row names
    for key in ('actions', 'adv', 'old_ll', 'returns'):
        if key in inp:
            inp[key][torch.from_numpy(~used)] = float('nan')
    ref = evaluate(c, inp, torch.float64)
    kl_torch = ref.pop('kl_torch', None)
    assert kl_torch is None or np.isclose(kl_torch, ref['kl'], rtol=1e-12, atol=0)
    f32 = evaluate(c, inp, torch.float32)
    dev32 = OrderedDict((k, float(np.abs(f32[k] - ref[k]).max())) for k in ref)
    return dict(inp, ref=ref, dev32=dev32, edge_rounds=rounds)
