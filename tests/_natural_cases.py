"""The cases of the population's natural-gradient step and their reference: torch
autograd of the same network built from the same flat parameters, in any dtype
(fp64 is the reference, fp32 the yardstick the tolerances come from).

A case is ``(H, inputs, outputs, head, S)``.  Heads: ``gauss`` (learned std),
``gauss_clamp`` (the log-std parameter above ``max_log_std``: the clamp is active),
``gauss_fixed`` (``learn_std=False``), ``cat`` and ``cat_double`` (the reference's
softmax-of-softmax head).  S: one row, both sides of a 64-row tile, several shares
with a ragged last tile (200), and more tiles than shares, so that a workgroup
walks more than one tile (1094 = 17 tiles + 6 rows against 16 shares).
"""
import numpy as np
import torch

_H = (32, 64)
_IN = (3, 17, 32)
_OUT = (1, 6, 8)
HEADS = ('gauss', 'gauss_clamp', 'gauss_fixed', 'cat', 'cat_double')
_S = (1, 63, 64, 65, 200, 1094)
# a sampled cross product: every value of every axis, every (H, inputs) pair, every head
# at every S class
CASES = [(_H[i % 2], _IN[(i // 2) % 3], _OUT[(i // 3) % 3], HEADS[i % 5],
          _S[(i // 5 + i) % 6]) for i in range(30)]

# Tolerances, relative to the largest magnitude of the reference quantity.  Each is twice
# the largest error of plain fp32 torch against fp64 torch over CASES, measured on the
# CPU by test_natural_cases_cpu.py (which holds fp32 torch to half of them) and rounded
# up to two digits.  Measured (fp32 vs fp64, max over the cases):
#   product 3.05e-7 (case 17), gradient 1.05e-6 (case 7),
#   loss 4.63e-7 (case 15; absolute: the losses are O(1))
TOL = dict(fvp=6.2e-7, grad=2.1e-6, loss=9.3e-7)
REG = 0.1


def r4(v):
    return (v + 3) & ~3


def layout(H, in_w, out_w):
    """Offsets of the flat parameter vector: slot 0 the log-std, then per layer
    ``W [out][round4(in)]`` and ``b [round4(out)]``.  Returns (w_off, b_off, n_flat)."""
    dims = (in_w, H, H, out_w)
    off, w_off, b_off = 4, [], []
    for l in range(3):
        w_off.append(off)
        off += dims[l + 1] * r4(dims[l])
        b_off.append(off)
        off += r4(dims[l + 1])
    return w_off, b_off, off


def make_desc(H, in_w, out_w):
    from garage_amd import _lib
    d = _lib.MlpDesc()
    d.n_layers = 3
    w_off, b_off, n_flat = layout(H, in_w, out_w)
    for l, v in enumerate((in_w, H, H, out_w)):
        d.dims[l] = v
    for l in range(3):
        d.w_off[l], d.b_off[l] = w_off[l], b_off[l]
    return d, n_flat


def make_case(case, seed):
    """fp64 CPU tensors of a case: flat parameters (padding zero), observations, actions,
    advantages, old log-likelihoods and a tangent vector (padding zero)."""
    H, in_w, out_w, head, S = case
    g = torch.Generator().manual_seed(seed)
    w_off, b_off, n_flat = layout(H, in_w, out_w)
    dims = (in_w, H, H, out_w)

    def flat(scale):
        v = torch.zeros(n_flat, dtype=torch.float64)
        for l in range(3):
            W = torch.randn(dims[l + 1], dims[l], generator=g, dtype=torch.float64)
            v[w_off[l]:w_off[l] + dims[l + 1] * r4(dims[l])].view(
                dims[l + 1], r4(dims[l]))[:, :dims[l]] = W * scale / np.sqrt(dims[l])
            v[b_off[l]:b_off[l] + dims[l + 1]] = 0.1 * scale * torch.randn(
                dims[l + 1], generator=g, dtype=torch.float64)
        return v

    params, vec = flat(1.0), flat(1.0)
    if head.startswith('gauss'):
        params[0], vec[0] = 0.3, 0.7
    X = torch.randn(S, in_w, generator=g, dtype=torch.float64)
    if head.startswith('cat'):
        actions = torch.randint(0, out_w, (S, 1), generator=g).double()
    else:
        actions = torch.randn(S, out_w, generator=g, dtype=torch.float64)
    adv = torch.randn(S, generator=g, dtype=torch.float64)
    with torch.no_grad():
        old_ll = log_likelihood(case, params, X, actions) + 0.1 * torch.randn(
            S, generator=g, dtype=torch.float64)
    return dict(params=params, vec=vec, X=X, actions=actions, adv=adv, old_ll=old_ll)


def std_options(head):
    """(has_min, min_log_std, has_max, max_log_std, learn_std) of a head."""
    return (0, 0.0, int(head == 'gauss_clamp'), 0.1, int(head != 'gauss_fixed'))


def forward(case, flat, X):
    H, in_w, out_w, _, _ = case
    w_off, b_off, _ = layout(H, in_w, out_w)
    dims = (in_w, H, H, out_w)
    h = X
    for l in range(3):
        W = flat[w_off[l]:w_off[l] + dims[l + 1] * r4(dims[l])].view(
            dims[l + 1], r4(dims[l]))[:, :dims[l]]
        h = h @ W.T + flat[b_off[l]:b_off[l] + dims[l + 1]]
        if l < 2:
            h = torch.tanh(h)
    return h


def _log_std(case, flat):
    s = flat[0]
    if case[3] == 'gauss_clamp':
        s = torch.clamp(s, max=0.1)
    return s


def _distribution(case, flat, X):
    head = case[3]
    out = forward(case, flat, X)
    if head.startswith('cat'):
        logits = torch.softmax(out, -1) if head == 'cat_double' else out
        return torch.distributions.Categorical(logits=logits)
    std = _log_std(case, flat).exp().expand_as(out)
    return torch.distributions.Independent(torch.distributions.Normal(out, std), 1)


def log_likelihood(case, flat, X, actions):
    dist = _distribution(case, flat, X)
    return dist.log_prob(actions[:, 0] if case[3].startswith('cat') else actions)


def surrogate(case, flat, t):
    """The unclipped surrogate loss (trpo.py:113-117), to be minimised."""
    ll = log_likelihood(case, flat, t['X'], t['actions'])
    return -((ll - t['old_ll']).exp() * t['adv']).mean()


def mean_kl(case, flat_old, flat_new, X):
    with torch.no_grad():
        old = _distribution(case, flat_old, X)
    return torch.distributions.kl_divergence(old, _distribution(case, flat_new, X)).mean()


def _no_std(case, g):
    """Slot 0 is no parameter of a categorical head or with ``learn_std=False``."""
    if case[3].startswith('cat') or case[3] == 'gauss_fixed':
        g = g.clone()
        g[0] = 0
    return g


def gradient(case, t, dtype=torch.float64):
    """(loss, gradient) of the surrogate at the case's parameters."""
    t = {k: v.to(dtype) for k, v in t.items()}
    flat = t['params'].clone().requires_grad_(True)
    loss = surrogate(case, flat, t)
    g, = torch.autograd.grad(loss, flat)
    return loss.detach(), _no_std(case, g)


def fvp(case, t, vec, dtype=torch.float64, reg=REG):
    """``d/dp (d/dp mean KL(old || new) . vec)`` at new == old by double backward, plus
    ``reg * vec``: what the reference's optimizer computes
    (conjugate_gradient_optimizer.py:18-66)."""
    params, X, vec = t['params'].to(dtype), t['X'].to(dtype), vec.to(dtype)
    flat = params.clone().requires_grad_(True)
    kl = mean_kl(case, params, flat, X)
    g, = torch.autograd.grad(kl, flat, create_graph=True)
    if not g.requires_grad:  # (a KL that is constant in its second derivative)
        return reg * vec
    hv, = torch.autograd.grad(g @ _no_std(case, vec), flat, allow_unused=True)
    hv = torch.zeros_like(vec) if hv is None else hv
    return _no_std(case, hv) + reg * vec


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
