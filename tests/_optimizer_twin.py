"""torch's single-tensor optimizer steps, restated in numpy fp32, and the case table
of the optimizer tests.

Written from ``torch/optim/sgd.py`` (``_single_tensor_sgd``), ``rmsprop.py``
(``_single_tensor_rmsprop``) and ``adam.py`` (``_single_tensor_adam``, the
non-capturable branch), not from the kernels.  The rules:

* every tensor operation is one fp32 rounding.  The composite ones follow the
  expression of torch's elementwise CPU kernels, left to right:
    ``add(t, alpha=a)``        ``x + a * t``
    ``addcmul(t1, t2, value)`` ``x + (value * t1) * t2``
    ``addcdiv(t1, t2, value)`` ``x + (value * t1) / t2``
* every scalar torch forms in Python is formed here in float64 and cast to fp32 once:
  ``1 - beta1``, ``1 - beta2``, ``1 - alpha``, ``1 - dampening``, ``1 - lr * wd``,
  ``-lr / bias_correction1``, ``bias_correction2 ** 0.5``, ``-lr``;
* ``lerp_`` (``exp_avg``, centred RMSprop's ``grad_avg``) is ONE fused multiply-add,
  ``w * (g - m) + m``, for the weights below 0.5 that the tables here use (torch's
  ``lerp`` switches to another formula from 0.5 on; ``lerp32`` refuses those).

``fma32`` is a correctly rounded fp32 fused multiply-add: ``float32(float64(a) *
float64(b) + float64(c))`` rounds twice and is wrong when the float64 sum lands on the
midpoint of two floats.

Used by ``test_optimizer_twin_cpu.py`` (is the twin itself within fp32's reach of
``torch.optim`` in float64?) and ``test_optimizer_steps_gpu.py`` (the optimizer entry
points of the C ABI, bit for bit against the twin).
"""
import zlib
from collections import OrderedDict
from fractions import Fraction

import numpy as np

F32 = np.float32
_FLT_MAX = float(np.finfo(np.float32).max)
# the smallest magnitude that rounds to infinity: FLT_MAX + half a unit of its last place
_OVERFLOW = Fraction(_FLT_MAX) + Fraction(2) ** 103


# ---- a correctly rounded fp32 fused multiply-add ------------------------------------

def fma32_shortcut(a, b, c):
    """``a * b + c`` through float64: the product is exact, the sum is rounded to
    float64 and then again to fp32."""
    with np.errstate(all='ignore'):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) +
                np.asarray(c, np.float64)).astype(np.float32)


def fma32_exact(a, b, c):
    """One element, by exact rational arithmetic: the nearest fp32 to ``a*b + c`` among
    the float64 shortcut's result and its two neighbours, ties to even."""
    a, b, c = float(F32(a)), float(F32(b)), float(F32(c))
    cand = fma32_shortcut(a, b, c)[()]
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return cand  # NaN / infinities: nothing to round
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x == 0:
        return cand  # an exact zero: the shortcut is exact too, sign included
    if abs(x) >= _OVERFLOW:
        return F32(np.inf) if x > 0 else F32(-np.inf)
    if not np.isfinite(cand):
        cand = F32(_FLT_MAX) if x > 0 else F32(-_FLT_MAX)
    best = None
    for k in (cand, np.nextafter(cand, F32(-np.inf)), np.nextafter(cand, F32(np.inf))):
        if not np.isfinite(k):
            continue
        key = (abs(Fraction(float(k)) - x), int(k.view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, k)
    return best[1]


def fma32(a, b, c):
    """Correctly rounded fp32 ``a * b + c``, elementwise with broadcasting.

    The float64 sum ``s`` is within half a float64 ulp of the exact value ``x``, so ``x``
    lies strictly between the float64 neighbours of ``s``.  Rounding to fp32 is
    monotonic: where both neighbours round to the same fp32, so does ``x``, and the
    shortcut is right.  Only the other elements (``s`` on or next to a midpoint of two
    floats) go through ``fma32_exact``."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32),
                                  np.asarray(c, np.float32))
    shape = a.shape
    a, b, c = np.atleast_1d(a, b, c)
    with np.errstate(all='ignore'):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = s.astype(np.float32)
        lo = np.nextafter(s, -np.inf).astype(np.float32)
        hi = np.nextafter(s, np.inf).astype(np.float32)
    doubt = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & (lo != hi)
    if doubt.any():
        out = out.copy()
        for idx in zip(*np.nonzero(doubt)):
            out[idx] = fma32_exact(a[idx], b[idx], c[idx])
    return out.reshape(shape)[()] if shape == () else out


def lerp32(m, g, w):
    """``m.lerp_(g, w)`` for ``w < 0.5``: ``fma(w, g - m, m)``."""
    assert abs(float(w)) < 0.5, 'torch.lerp takes another formula from 0.5 on'
    return fma32(F32(w), g - m, m)


# ---- torch's single-tensor steps -----------------------------------------------------
# Each function takes fp32 arrays, returns the new ones and leaves its inputs alone.

def _f(x):
    return F32(float(x))


def sgd_step(p, g, buf, lr=1e-3, momentum=0, dampening=0, weight_decay=0,
             nesterov=False):
    """``_single_tensor_sgd``.  ``buf`` is ``None`` before the first step, as in
    torch's state; returns ``(p, buf)``."""
    if weight_decay != 0:
        g = g + _f(weight_decay) * p                  # grad.add(param, alpha=wd)
    if momentum != 0:
        if buf is None:
            buf = g.copy()                            # torch.clone(grad).detach()
        else:
            buf = buf * _f(momentum)                  # buf.mul_(momentum)
            buf = buf + _f(1 - dampening) * g         #    .add_(grad, alpha=1-dampening)
        g = g + _f(momentum) * buf if nesterov else buf
    p = p + _f(-lr) * g                               # param.add_(grad, alpha=-lr)
    return p, buf


def rmsprop_step(p, g, square_avg, buf, grad_avg, lr=1e-2, alpha=0.99, eps=1e-8,
                 weight_decay=0, momentum=0, centered=False):
    """``_single_tensor_rmsprop``; returns ``(p, square_avg, buf, grad_avg)``."""
    if weight_decay != 0:
        g = g + _f(weight_decay) * p
    square_avg = square_avg * _f(alpha)               # square_avg.mul_(alpha)
    square_avg = square_avg + (_f(1 - alpha) * g) * g  #  .addcmul_(g, g, value=1-alpha)
    if centered:
        grad_avg = lerp32(grad_avg, g, _f(1 - alpha))  # grad_avg.lerp_(grad, 1-alpha)
        with np.errstate(invalid='ignore'):
            avg = np.sqrt(square_avg + (F32(-1) * grad_avg) * grad_avg)
    else:
        avg = np.sqrt(square_avg)
    avg = avg + _f(eps)                               # avg.add_(eps)
    if momentum > 0:
        buf = buf * _f(momentum)                      # buf.mul_(momentum)
        buf = buf + (F32(1) * g) / avg                #    .addcdiv_(grad, avg)
        p = p + _f(-lr) * buf                         # param.add_(buf, alpha=-lr)
    else:
        p = p + (_f(-lr) * g) / avg                   # param.addcdiv_(grad, avg, -lr)
    return p, square_avg, buf, grad_avg


def adam_step(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq, step, lr=1e-3,
              betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
              decoupled=False):
    """``_single_tensor_adam`` at step number ``step`` (1 for the first);
    ``decoupled`` is AdamW.  Returns ``(p, exp_avg, exp_avg_sq, max_exp_avg_sq)``."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    if weight_decay != 0:
        if decoupled:
            p = p * _f(1 - lr * weight_decay)         # param.mul_(1 - lr * wd)
        else:
            g = g + _f(weight_decay) * p
    exp_avg = lerp32(exp_avg, g, _f(1 - beta1))       # exp_avg.lerp_(grad, 1 - beta1)
    exp_avg_sq = exp_avg_sq * _f(beta2)               # exp_avg_sq.mul_(beta2)
    exp_avg_sq = exp_avg_sq + (_f(1 - beta2) * g) * g  # .addcmul_(g, g, value=1-beta2)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    if amsgrad:
        max_exp_avg_sq = np.maximum(max_exp_avg_sq, exp_avg_sq)
        root = np.sqrt(max_exp_avg_sq)
    else:
        root = np.sqrt(exp_avg_sq)
    denom = root / _f(bias_correction2_sqrt) + _f(eps)
    p = p + (_f(-step_size) * exp_avg) / denom        # addcdiv_(exp_avg, denom, -step_size)
    return p, exp_avg, exp_avg_sq, max_exp_avg_sq


def default_adam_step(p, g, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999),
                      eps=1e-8):
    """torch's default-shaped Adam (no weight decay, no amsgrad): the sequence
    ``ga_adam_update`` documents.  Returns ``(p, exp_avg, exp_avg_sq)``."""
    return adam_step(p, g, exp_avg, exp_avg_sq, None, step, lr=lr, betas=betas,
                     eps=eps)[:3]


# ---- the cases -----------------------------------------------------------------------
# tag -> (torch.optim class name, keyword arguments, step count before the first step).
# The first seven are ``OPTIMIZER_CASES`` of test_ppo_gpu.py / make_golden.py.  A
# non-zero step count starts from random non-zero state (``initial_state``).
CASES = OrderedDict([
    ('sgd_plain', ('SGD', dict(lr=5e-2), 0)),
    ('sgd_nesterov_wd', ('SGD', dict(lr=2e-2, momentum=0.9, nesterov=True,
                                     weight_decay=1e-3), 0)),
    ('sgd_momentum_dampening', ('SGD', dict(lr=2e-2, momentum=0.8, dampening=0.1), 0)),
    ('rmsprop', ('RMSprop', dict(lr=1e-3), 0)),
    ('rmsprop_centered_momentum', ('RMSprop', dict(lr=1e-3, alpha=0.9, momentum=0.5,
                                                   centered=True, weight_decay=1e-3),
                                   0)),
    ('adam_amsgrad_wd', ('Adam', dict(lr=2.5e-3, amsgrad=True, weight_decay=1e-2), 0)),
    ('adamw', ('AdamW', dict(lr=2.5e-3, weight_decay=5e-2), 0)),
    # float32(1) - float32(0.9) is not float32(1 - 0.9) (for 0.1 it happens to be)
    ('sgd_dampening_09', ('SGD', dict(lr=2e-2, momentum=0.8, dampening=0.9), 0)),
    ('rmsprop_default', ('RMSprop', dict(), 0)),
    ('rmsprop_centered', ('RMSprop', dict(lr=1e-3, centered=True), 0)),
    ('adam_amsgrad', ('Adam', dict(lr=2.5e-3, amsgrad=True), 0)),
    ('adamw_amsgrad', ('AdamW', dict(lr=2.5e-3, amsgrad=True), 0)),
    ('adamw_amsgrad_step1000', ('AdamW', dict(lr=2.5e-3, amsgrad=True), 1000)),
    # torch's default-shaped Adam: ga_adam_step_f32 and the fused update paths
    ('adam_default', ('Adam', dict(lr=2.5e-4), 0)),
])

STEPS = 6
BUFFERS = {'SGD': ('momentum_buffer', ),
           'RMSprop': ('square_avg', 'momentum_buffer', 'grad_avg'),
           'Adam': ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'),
           'AdamW': ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')}


def used_buffers(tag):
    """Names of the state buffers the case keeps, in the order of ``BUFFERS``."""
    name, kw, _ = CASES[tag]
    if name == 'SGD':
        keep = (kw.get('momentum', 0) != 0, )
    elif name == 'RMSprop':
        keep = (True, kw.get('momentum', 0) > 0, bool(kw.get('centered', False)))
    else:
        keep = (True, True, bool(kw.get('amsgrad', False)))
    return tuple(b for b, k in zip(BUFFERS[name], keep) if k)


def case_inputs(tag, n, steps=STEPS):
    """``(p0, grads[steps], state0)`` of a case: parameters ``0.3 * randn``, gradients
    ``randn``; ``state0`` maps each kept buffer to zeros (``None`` for SGD's momentum
    buffer, which torch creates at the first step) or, for a case that starts late, to
    random values with ``exp_avg_sq >= 0`` and ``max_exp_avg_sq >= exp_avg_sq``."""
    rng = np.random.RandomState(zlib.crc32(tag.encode()) & 0x7FFFFFFF)
    p0 = (0.3 * rng.randn(n)).astype(np.float32)
    grads = rng.randn(steps, n).astype(np.float32)
    name, _, step0 = CASES[tag]
    state = OrderedDict()
    for b in used_buffers(tag):
        if step0 == 0:
            state[b] = None if name == 'SGD' else np.zeros(n, np.float32)
        elif b in ('exp_avg_sq', 'square_avg'):
            state[b] = ((0.1 * rng.randn(n)) ** 2).astype(np.float32)
        elif b == 'max_exp_avg_sq':
            state[b] = state['exp_avg_sq'] + np.abs(0.01 * rng.randn(n)).astype(
                np.float32)
        else:
            state[b] = (0.1 * rng.randn(n)).astype(np.float32)
    return p0, grads, state


class Twin:
    """One case of the table, stepped in fp32.  ``p`` and ``state`` are replaced at
    every step, never written in place."""

    def __init__(self, tag, p0, state0):
        self.name, self.kw, self.step_count = CASES[tag]
        self.p = p0.copy()
        self.state = OrderedDict((k, None if v is None else v.copy())
                                 for k, v in state0.items())

    def step(self, g):
        self.step_count += 1
        s, kw = self.state, self.kw
        if self.name == 'SGD':
            self.p, buf = sgd_step(self.p, g, s.get('momentum_buffer'), **kw)
            if 'momentum_buffer' in s:
                s['momentum_buffer'] = buf
        elif self.name == 'RMSprop':
            out = rmsprop_step(self.p, g, s['square_avg'], s.get('momentum_buffer'),
                               s.get('grad_avg'), **kw)
            self.p = out[0]
            for k, v in zip(BUFFERS['RMSprop'], out[1:]):
                if k in s:
                    s[k] = v
        else:
            out = adam_step(self.p, g, s['exp_avg'], s['exp_avg_sq'],
                            s.get('max_exp_avg_sq'), self.step_count,
                            decoupled=self.name == 'AdamW',
                            **self._adam_kw())
            self.p = out[0]
            for k, v in zip(BUFFERS['Adam'], out[1:]):
                if k in s:
                    s[k] = v

    def _adam_kw(self):
        kw = dict(self.kw)
        if self.name == 'AdamW':
            kw.setdefault('weight_decay', 1e-2)  # torch.optim.AdamW's default
        return kw

    def buffers(self):
        """``{'p': ..., <state buffer>: ...}`` as they stand."""
        out = OrderedDict(p=self.p)
        out.update(self.state)
        return out


class TorchReference:
    """The same case through ``torch.optim`` (the single-tensor path) on the CPU, in
    ``dtype``; inputs are the fp32 values, widened."""

    def __init__(self, tag, p0, state0, dtype=None):
        import torch
        dtype = dtype or torch.float64
        name, kw, step0 = CASES[tag]
        self.dtype = dtype
        self.p = torch.from_numpy(p0.copy()).to(dtype).requires_grad_(True)
        self.opt = getattr(torch.optim, name)([self.p], foreach=False, **kw)
        self.names = tuple(state0)
        if step0:
            st = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in state0.items()}
            st['step'] = torch.tensor(float(step0))
            self.opt.state[self.p] = st

    def set_step_count(self, count):
        self.opt.state[self.p]['step'].fill_(float(count))

    def step(self, g):
        import torch
        self.p.grad = torch.from_numpy(g.copy()).to(self.dtype)
        self.opt.step()

    def buffers(self):
        out = OrderedDict(p=self.p.detach().numpy().copy())
        st = self.opt.state[self.p]
        for k in self.names:
            out[k] = st[k].numpy().copy()
        return out


def rel_err(a, b):
    """max|a - b| / max|b| in float64 (0 for two all-zero buffers)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    diff = np.abs(a - b).max()
    return 0.0 if diff == 0 else float(diff / scale)


def twin_and_fp64(tag, n, steps=STEPS):
    """Run a case through the twin and through float64 torch.  Returns
    ``(inputs, history, ref)``: ``history[k]`` = the twin's buffers after step ``k+1``,
    ``ref`` = float64 torch's after the last step."""
    p0, grads, state0 = case_inputs(tag, n, steps)
    twin = Twin(tag, p0, state0)
    ref = TorchReference(tag, p0, state0)
    history = []
    for g in grads:
        twin.step(g)
        ref.step(g)
        history.append(twin.buffers())
    return (p0, grads, state0), history, ref.buffers()
