"""The optimizer entry points of the C ABI, called directly: ``ga_optimizer_step_f32``,
``ga_adam_step_f32``, ``ga_reduce_slabs_f32`` and ``ga_reduce_adam_f32``.

The steps are held to ``tests/_optimizer_twin.py`` -- torch's single-tensor arithmetic
restated in numpy fp32, written from torch's source -- BIT FOR BIT: parameters and every
state buffer, after every step, with poisoned guard elements behind each buffer.  The
same runs are also held to ``torch.optim`` in float64, within 4x the twin's own error
against it (floor 2^-24): the twin's error varies by about 2x between seeds, a
complement weight formed from rounded constants costs 10 to 40x, and this second check
stays meaningful should the bitwise one ever be relaxed.  ``test_optimizer_twin_cpu.py``
shows the twin itself is within fp32's reach of float64 torch on every case.

The slab sums are exact on integer-valued slabs (any summation order gives the integer
sum, so a slab dropped or counted twice at a loop remainder shows), within the
any-order bound on random ones, and deterministic; ``ga_reduce_adam_f32`` must give
the bits of ``ga_reduce_slabs_f32`` followed by ``ga_adam_step_f32``."""
import ctypes as C
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _optimizer_twin as tw

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 4099)
NMAX = max(SIZES)
GUARD = 64
POISON = -7.0e9  # finite: a kernel that read it would not hide behind a NaN
GENERIC = [t for t in tw.CASES if t != 'adam_default']


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


def _lib():
    from garage_amd import _lib as L
    return L


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _guarded(values, n, dev, fill=POISON):
    """``values[:n]`` (or ``fill`` if ``None``) followed by GUARD poisoned elements."""
    t = torch.full((n + GUARD, ), fill, dtype=torch.float32, device=dev)
    if values is not None:
        t[:n] = torch.from_numpy(np.ascontiguousarray(values[:n])).to(dev)
    return t


def _host(t, n):
    """A host copy of ``t[:n]`` that later launches cannot change."""
    return t[:n].cpu().numpy().copy()


def _guard_intact(t, n, fill=POISON):
    return bool((t[n:] == fill).all())


def _hyper(tag):
    """``(kind, h[5], flags, (s1, s2, s3) buffer names or None)`` of a case as the header
    documents them, from torch's keyword names and defaults."""
    name, kw, _ = tw.CASES[tag]
    if name == 'SGD':
        h = [kw.get('lr', 1e-3), kw.get('momentum', 0), kw.get('dampening', 0),
             kw.get('weight_decay', 0), 0.0]
        kind, flags = 1, int(kw.get('nesterov', False))
    elif name == 'RMSprop':
        h = [kw.get('lr', 1e-2), kw.get('alpha', 0.99), kw.get('eps', 1e-8),
             kw.get('weight_decay', 0), kw.get('momentum', 0)]
        kind, flags = 2, int(kw.get('centered', False))
    else:
        betas = kw.get('betas', (0.9, 0.999))
        h = [kw.get('lr', 1e-3), betas[0], betas[1], kw.get('eps', 1e-8),
             kw.get('weight_decay', 1e-2 if name == 'AdamW' else 0)]
        kind = 3
        flags = int(kw.get('amsgrad', False)) | (2 if name == 'AdamW' else 0)
    used = tw.used_buffers(tag)
    slots = tuple(b if b in used else None for b in tw.BUFFERS[name])
    slots += (None, ) * (3 - len(slots))
    return kind, [float(v) for v in h], flags, slots


def test_hyper_parameters_are_what_the_wrapper_passes():
    from garage_amd.optimizers import _torch_optimizer_hyper
    for tag in GENERIC:
        name, kw, _ = tw.CASES[tag]
        kind, h, flags, slots = _hyper(tag)
        mine = _torch_optimizer_hyper(name, kw)
        assert mine['kind'] == 'generic' and mine['code'] == kind, tag
        assert [float(v) for v in mine['h']] == h and mine['flags'] == flags, tag
        assert tuple(bool(s) for s in slots) == tuple(mine['needs']), tag
    name, kw, _ = tw.CASES['adam_default']
    assert _torch_optimizer_hyper(name, kw)['kind'] == 'adam'


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """The twin's buffers after each step and float64 torch's after the last, at the
    largest size; the steps are elementwise, so a smaller size is a prefix."""
    (p0, grads, state0), history, ref = tw.twin_and_fp64(tag, NMAX)
    for arrs in history:
        for v in arrs.values():
            if v is not None:
                v.setflags(write=False)
    return p0, grads, state0, history, ref


def _run_generic(tag, n, dev, grads=None, p0=None):
    """Step a case through ``ga_optimizer_step_f32`` on ``n`` elements.  Returns
    ``(per-step {buffer: host array}, guards intact)``."""
    L = _lib()
    rp0, rgrads, state0, _, _ = _reference(tag)
    p0 = rp0 if p0 is None else p0
    grads = rgrads if grads is None else grads
    kind, h, flags, slots = _hyper(tag)
    step0 = tw.CASES[tag][2]
    p = _guarded(p0, n, dev)
    bufs = OrderedDict()
    for b in slots:
        if b is None:
            continue
        init = state0[b]
        bufs[b] = _guarded(init, n, dev)
        if init is None:  # SGD: torch clones the gradient at the first step
            bufs[b][:n] = float('nan')
    hh = (C.c_double * 5)(*h)
    out, intact = [], True
    for k, g in enumerate(grads):
        gd = _guarded(g, n, dev, fill=float('nan'))
        ptrs = [L.dptr(bufs[b]) if b is not None else None for b in slots]
        L.call('ga_optimizer_step_f32', kind, L.dptr(p), L.dptr(gd), ptrs[0], ptrs[1],
               ptrs[2], n, step0 + k + 1, hh, flags, L.stream_ptr())
        torch.cuda.synchronize()
        res = OrderedDict(p=_host(p, n))
        for b, t in bufs.items():
            res[b] = _host(t, n)
        out.append(res)
        intact = intact and _guard_intact(p, n) and all(
            _guard_intact(t, n) for t in bufs.values())
        assert np.array_equal(_bits(_host(gd, n)), _bits(g[:n]))
    return out, intact


def _mismatches(got, want, n):
    """Per buffer: how many elements differ in their bits, and by how much at most."""
    out = OrderedDict()
    for k, w in want.items():
        if w is None:
            continue
        bad = _bits(got[k]) != _bits(w[:n])
        if bad.any():
            out[k] = (int(bad.sum()), float(np.abs(got[k].astype(np.float64) -
                                                   w[:n]).max()))
    return out


@pytest.mark.parametrize('tag', GENERIC)
def test_optimizer_step_matches_the_twin_bit_for_bit(dev, tag):
    _, _, _, history, _ = _reference(tag)
    failures = []
    for n in SIZES:
        got, intact = _run_generic(tag, n, dev)
        assert intact, (tag, n, 'elements past n were written')
        for k in range(tw.STEPS):
            assert set(got[k]) == {'p'} | set(tw.used_buffers(tag))
            bad = _mismatches(got[k], history[k], n)
            if bad:
                failures.append((n, k + 1, bad))
    for f in failures[:12]:
        print('bit mismatch: %s n=%d step=%d %s' % ((tag, ) + f))
    assert not failures, (tag, len(failures), failures[0])


@pytest.mark.parametrize('tag', GENERIC)
def test_optimizer_step_stays_within_the_twins_error_of_float64_torch(dev, tag):
    _, _, _, history, ref = _reference(tag)
    for n in SIZES:
        got, _ = _run_generic(tag, n, dev)
        for k, r in ref.items():
            mine = tw.rel_err(got[-1][k], r[:n])
            twin = tw.rel_err(history[-1][k][:n], r[:n])
            bound = max(4 * twin, 2.0 ** -24)
            print('%-26s n=%-5d %-16s kernel %.2e twin %.2e bound %.2e' % (
                tag, n, k, mine, twin, bound))
            assert np.isfinite(got[-1][k]).all(), (tag, n, k)
            assert mine <= bound, (tag, n, k, mine, twin)


def test_late_start_state_is_what_it_should_be(dev):
    """The step-1000 case: the loaded state is non-zero, ``exp_avg_sq >= 0`` and
    ``max_exp_avg_sq >= exp_avg_sq``, and stays so on the device."""
    tag = 'adamw_amsgrad_step1000'
    _, _, state0, _, _ = _reference(tag)
    assert (state0['exp_avg_sq'] >= 0).all() and np.abs(state0['exp_avg']).min() > 0
    assert (state0['max_exp_avg_sq'] >= state0['exp_avg_sq']).all()
    got, _ = _run_generic(tag, 257, dev)
    for res in got:
        assert (res['exp_avg_sq'] >= 0).all()
        assert (res['max_exp_avg_sq'] >= res['exp_avg_sq']).all()


@pytest.mark.parametrize('tag', ['sgd_momentum_dampening', 'rmsprop',
                                 'rmsprop_centered', 'adam_amsgrad',
                                 'adam_generic_defaults'])
def test_zero_gradient_on_zero_state_changes_nothing(dev, tag):
    """``g = 0`` on ``v = 0``: the denominators are ``eps`` alone; the parameters keep
    their bits and no buffer turns NaN.  (Cases without weight decay.)"""
    if tag == 'adam_generic_defaults':  # kind 3 with nothing switched on
        tw_tag = 'adam_default'
    else:
        tw_tag = tag
    n = 257
    p0, _, _, _, _ = _reference(tw_tag)
    zeros = np.zeros((2, NMAX), np.float32)
    got, intact = _run_generic(tw_tag, n, dev, grads=zeros)
    assert intact
    for res in got:
        assert np.array_equal(_bits(res['p']), _bits(p0[:n]))
        for k, v in res.items():
            assert np.isfinite(v).all(), (tag, k)
            if k != 'p':
                assert not v.any(), (tag, k)


def test_default_adam_through_the_generic_entry_matches_the_twin(dev):
    """Kind 3 with no weight decay and no amsgrad is the default Adam again."""
    tag = 'adam_default'
    _, _, _, history, _ = _reference(tag)
    for n in (257, NMAX):
        got, intact = _run_generic(tag, n, dev)
        assert intact
        for k in range(tw.STEPS):
            assert not _mismatches(got[k], history[k], n), (n, k + 1)


# ---- ga_adam_step_f32 ---------------------------------------------------------------

def test_adam_step_matches_the_twin_bit_for_bit_and_float64_torch(dev):
    L = _lib()
    tag = 'adam_default'
    p0, grads, state0, history, ref = _reference(tag)
    _, kw, _ = tw.CASES[tag]
    lr = kw['lr']
    # one more step far along: the bias corrections at step 100000
    rng = np.random.RandomState(5)
    g_late = rng.randn(NMAX).astype(np.float32)
    last = history[-1]
    late = tw.default_adam_step(last['p'], g_late, last['exp_avg'], last['exp_avg_sq'],
                                100000, lr=lr)
    late = OrderedDict(zip(('p', 'exp_avg', 'exp_avg_sq'), late))
    ref64 = tw.TorchReference(tag, p0, state0)
    for g in grads:
        ref64.step(g)
    ref64.set_step_count(99999)
    ref64.step(g_late)
    ref_late = ref64.buffers()
    for n in SIZES:
        p = _guarded(p0, n, dev)
        m = _guarded(state0['exp_avg'], n, dev)
        v = _guarded(state0['exp_avg_sq'], n, dev)
        want = history + [late]
        for k, (g, step) in enumerate(list(zip(grads, range(1, 7))) +
                                      [(g_late, 100000)]):
            gd = _guarded(g, n, dev, fill=float('nan'))
            L.call('ga_adam_step_f32', L.dptr(p), L.dptr(gd), L.dptr(m), L.dptr(v), n,
                   step, lr, 0.9, 0.999, 1e-8, L.stream_ptr())
            torch.cuda.synchronize()
            got = OrderedDict(p=_host(p, n), exp_avg=_host(m, n),
                              exp_avg_sq=_host(v, n))
            assert not _mismatches(got, want[k], n), (n, step,
                                                      _mismatches(got, want[k], n))
            assert all(_guard_intact(t, n) for t in (p, m, v)), (n, step)
            if step in (6, 100000):
                r = ref if step == 6 else ref_late
                for key in got:
                    mine = tw.rel_err(got[key], r[key][:n])
                    twin = tw.rel_err(want[k][key][:n], r[key][:n])
                    assert mine <= max(4 * twin, 2.0 ** -24), (n, step, key, mine, twin)


# ---- ga_reduce_slabs_f32 / ga_reduce_adam_f32 ---------------------------------------

SPLITS = (1, 2, 3, 4, 5, 12, 13, 16, 17, 28, 29, 33)
REDUCE_N = (4, 252, 256, 260, 1028)


def _slabs(values, stride, dev):
    """``values[n_splits, n]`` laid out ``stride`` apart, the padding NaN."""
    s, n = values.shape
    host = np.full((s, stride), np.nan, np.float32)
    host[:, :n] = values
    return torch.from_numpy(host).to(dev).reshape(-1)


def _reduce(slabs, n_splits, stride, n, scale, dev):
    L = _lib()
    out = _guarded(None, n, dev)
    L.call('ga_reduce_slabs_f32', L.dptr(slabs), n_splits, stride, n, float(scale),
           L.dptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_intact(out, n), (n_splits, n, stride)
    return _host(out, n)


def _reduce_cases():
    for n in REDUCE_N:
        for stride in (n, n + 8):
            yield n, stride


@pytest.mark.parametrize('n_splits', SPLITS)
def test_reduce_slabs_is_exact_on_integers(dev, n_splits):
    rng = np.random.RandomState(100 + n_splits)
    for n, stride in _reduce_cases():
        vals = rng.randint(-1024, 1025, size=(n_splits, n)).astype(np.float32)
        want = vals.astype(np.int64).sum(axis=0)
        slabs = _slabs(vals, stride, dev)
        for scale in (1.0, 0.25, 8.0):
            got = _reduce(slabs, n_splits, stride, n, scale, dev)
            assert np.array_equal(got.astype(np.float64), want * scale), (n, stride,
                                                                          scale)


@pytest.mark.parametrize('n_splits', SPLITS)
def test_reduce_slabs_on_random_slabs_is_bounded_and_deterministic(dev, n_splits):
    """|sum - exact sum| <= (n_splits - 1) 2^-24 sum|x| holds for every order of adding
    n_splits floats, with no higher-order term (Rump, "Error estimation of floating-point
    summation and dot product", BIT 2012); the zeros the kernel adds are exact."""
    rng = np.random.RandomState(200 + n_splits)
    for n, stride in _reduce_cases():
        vals = rng.randn(n_splits, n).astype(np.float32)
        ref = vals.astype(np.float64).sum(axis=0)
        bound = (n_splits - 1) * 2.0 ** -24 * np.abs(vals.astype(np.float64)).sum(
            axis=0)
        slabs = _slabs(vals, stride, dev)
        got = _reduce(slabs, n_splits, stride, n, 1.0, dev)
        again = _reduce(slabs, n_splits, stride, n, 1.0, dev)
        assert np.array_equal(_bits(got), _bits(again)), (n, stride)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), (n, stride, float((err - bound).max()))
        if n_splits == 1:
            assert np.array_equal(_bits(got), _bits(vals[0]))


def _reduce_adam(vals, stride, n, step, zero_slot0, start, dev):
    """``ga_reduce_adam_f32`` from ``start`` = (p, m, v); returns grads, p, m, v."""
    L = _lib()
    slabs = _slabs(vals, stride, dev)
    p, m, v = (_guarded(x, n, dev) for x in start)
    g = _guarded(None, n, dev)
    L.call('ga_reduce_adam_f32', L.dptr(slabs), vals.shape[0], stride, L.dptr(p),
           L.dptr(g), L.dptr(m), L.dptr(v), n, step, 2.5e-4, 0.9, 0.999, 1e-8,
           int(zero_slot0), L.stream_ptr())
    torch.cuda.synchronize()
    assert all(_guard_intact(t, n) for t in (p, g, m, v)), (vals.shape, stride)
    return [_host(t, n) for t in (g, p, m, v)]


def _reduce_then_adam(vals, stride, n, step, zero_slot0, start, dev):
    """The two separate launches the fused one promises to reproduce."""
    L = _lib()
    slabs = _slabs(vals, stride, dev)
    p, m, v = (_guarded(x, n, dev) for x in start)
    g = _guarded(None, n, dev)
    L.call('ga_reduce_slabs_f32', L.dptr(slabs), vals.shape[0], stride, n, 1.0,
           L.dptr(g), L.stream_ptr())
    if zero_slot0:
        g[0:1].zero_()
    L.call('ga_adam_step_f32', L.dptr(p), L.dptr(g), L.dptr(m), L.dptr(v), n, step,
           2.5e-4, 0.9, 0.999, 1e-8, L.stream_ptr())
    torch.cuda.synchronize()
    return [_host(t, n) for t in (g, p, m, v)]


@pytest.mark.parametrize('n_splits', SPLITS)
def test_reduce_adam_is_reduce_slabs_then_adam_step(dev, n_splits):
    rng = np.random.RandomState(300 + n_splits)
    names = ('grads', 'params', 'exp_avg', 'exp_avg_sq')
    for n, stride in _reduce_cases():
        vals = rng.randn(n_splits, n).astype(np.float32)
        start = ((0.3 * rng.randn(n)).astype(np.float32),
                 (0.1 * rng.randn(n)).astype(np.float32),
                 ((0.1 * rng.randn(n)) ** 2).astype(np.float32))
        step = 3
        fused = _reduce_adam(vals, stride, n, step, 0, start, dev)
        apart = _reduce_then_adam(vals, stride, n, step, 0, start, dev)
        for name, a, b in zip(names, fused, apart):
            assert np.array_equal(_bits(a), _bits(b)), (name, n, stride)
        # and the step itself is the twin's, on the gradient the launch wrote
        want = tw.default_adam_step(start[0], fused[0], start[1], start[2], step,
                                    lr=2.5e-4)
        for name, a, b in zip(names[1:], fused[1:], want):
            assert np.array_equal(_bits(a), _bits(b)), (name, n, stride)
        # zero_slot0: element 0 steps on a zero gradient, nothing else changes
        flagged = _reduce_adam(vals, stride, n, step, 1, start, dev)
        apart0 = _reduce_then_adam(vals, stride, n, step, 1, start, dev)
        assert flagged[0][0] == 0.0 and not np.signbit(flagged[0][0])
        for name, a, b, plain in zip(names, flagged, apart0, fused):
            assert np.array_equal(_bits(a), _bits(b)), (name, n, stride)
            assert np.array_equal(_bits(a[1:]), _bits(plain[1:])), (name, n, stride)
        z = tw.default_adam_step(start[0][:1], np.zeros(1, np.float32), start[1][:1],
                                 start[2][:1], step, lr=2.5e-4)
        for name, a, b in zip(names[1:], flagged[1:], z):
            assert _bits(a[:1]) == _bits(b), name


# ---- refusals -----------------------------------------------------------------------

def test_refusals_leave_a_message_and_the_buffers_alone(dev):
    L = _lib()
    lib = L.load()
    s = L.stream_ptr()
    n = 8
    rng = np.random.RandomState(7)
    bufs = {k: torch.from_numpy(rng.randn(2 * n + 1).astype(np.float32)).to(dev)
            for k in ('p', 'g', 's1', 's2', 's3', 'slabs', 'out')}
    before = {k: t.clone() for k, t in bufs.items()}
    P = {k: L.dptr(t) for k, t in bufs.items()}
    off = {k: L.dptr(t[1:]) for k, t in bufs.items()}  # 4 bytes past a 16-B boundary
    sgd = (C.c_double * 5)(1e-2, 0.9, 0.0, 0.0, 0.0)
    sgd_plain = (C.c_double * 5)(1e-2, 0.0, 0.0, 0.0, 0.0)
    rms = (C.c_double * 5)(1e-2, 0.99, 1e-8, 0.0, 0.0)
    rms_mom = (C.c_double * 5)(1e-2, 0.99, 1e-8, 0.0, 0.5)
    adam = (C.c_double * 5)(1e-3, 0.9, 0.999, 1e-8, 0.0)

    def opt(kind, h, flags=0, p='p', g='g', s1='s1', s2='s2', s3='s3', n_=n, step=1):
        ptr = lambda k: P[k] if k else None  # noqa: E731
        return lib.ga_optimizer_step_f32(kind, ptr(p), ptr(g), ptr(s1), ptr(s2),
                                         ptr(s3), n_, step, h, flags, s)

    def adam_step(n_=n, step=1, **null):
        a = {k: (None if k in null else P[k]) for k in ('p', 'g', 's1', 's2')}
        return lib.ga_adam_step_f32(a['p'], a['g'], a['s1'], a['s2'], n_, step, 1e-3,
                                    0.9, 0.999, 1e-8, s)

    def slabs(ptrs=P, n_splits=2, stride=n, n_=n, slabs_='slabs', out='out'):
        return lib.ga_reduce_slabs_f32(ptrs[slabs_] if slabs_ else None, n_splits,
                                       stride, n_, 1.0, ptrs[out] if out else None, s)

    def radam(n_splits=2, stride=n, n_=n, step=1, **ptrs):
        a = dict(slabs=P['slabs'], p=P['p'], g=P['g'], s1=P['s1'], s2=P['s2'])
        a.update(ptrs)
        return lib.ga_reduce_adam_f32(a['slabs'], n_splits, stride, a['p'], a['g'],
                                      a['s1'], a['s2'], n_, step, 1e-3, 0.9, 0.999,
                                      1e-8, 0, s)

    refused = [
        ('ga_optimizer_step_f32', [
            lambda: opt(0, adam), lambda: opt(4, adam), lambda: opt(-1, adam),
            lambda: opt(3, adam, n_=0), lambda: opt(1, sgd, n_=-4),
            lambda: opt(3, adam, step=0), lambda: opt(1, sgd, step=0),
            lambda: opt(2, rms, step=-1),
            lambda: opt(3, adam, p=None), lambda: opt(3, adam, g=None),
            lambda: lib.ga_optimizer_step_f32(3, P['p'], P['g'], P['s1'], P['s2'],
                                              None, n, 1, None, 0, s),
            lambda: opt(1, sgd, s1=None),                    # SGD with momentum
            lambda: opt(2, rms, s1=None),                    # RMSprop: square_avg
            lambda: opt(2, rms_mom, s2=None),                #   momentum buffer
            lambda: opt(2, rms, flags=1, s3=None),           #   centred: grad_avg
            lambda: opt(3, adam, s1=None), lambda: opt(3, adam, s2=None),
            lambda: opt(3, adam, flags=1, s3=None),          # amsgrad
            lambda: opt(3, adam, flags=3, s3=None)]),
        ('ga_adam_step_f32', [
            lambda: adam_step(n_=0), lambda: adam_step(n_=-1),
            lambda: adam_step(step=0), lambda: adam_step(p=1), lambda: adam_step(g=1),
            lambda: adam_step(s1=1), lambda: adam_step(s2=1)]),
        ('ga_reduce_slabs_f32', [
            lambda: slabs(n_=0), lambda: slabs(n_splits=0), lambda: slabs(n_=6),
            lambda: slabs(stride=n + 2), lambda: slabs(n_=6, stride=6),
            lambda: slabs(slabs_=None), lambda: slabs(out=None),
            lambda: slabs(ptrs=dict(P, slabs=off['slabs'])),
            lambda: slabs(ptrs=dict(P, out=off['out']))]),
        ('ga_reduce_adam_f32', [
            lambda: radam(n_=0), lambda: radam(n_splits=0), lambda: radam(step=0),
            lambda: radam(n_=6), lambda: radam(stride=n + 2),
            lambda: radam(slabs=None), lambda: radam(p=None), lambda: radam(g=None),
            lambda: radam(s1=None), lambda: radam(s2=None),
            lambda: radam(slabs=off['slabs']), lambda: radam(p=off['p']),
            lambda: radam(g=off['g']), lambda: radam(s1=off['s1']),
            lambda: radam(s2=off['s2'])]),
    ]
    for entry, calls in refused:
        for i, fn in enumerate(calls):
            rc = fn()
            assert rc != 0, (entry, i)
            assert entry.encode() in lib.ga_last_error(), (entry, i,
                                                           lib.ga_last_error())
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    # what is allowed: unused state pointers are NULL
    assert opt(1, sgd_plain, s1=None, s2=None, s3=None) == 0
    assert opt(2, rms, s2=None, s3=None) == 0
    assert opt(3, adam, s3=None) == 0
    torch.cuda.synchronize()
