"""Precondition of ``test_optimizer_steps_gpu.py``: the fp32 twin of torch's
single-tensor optimizer steps (``_optimizer_twin.py``) rounds its fused multiply-add
correctly and, on every case of the table, stays within fp32's reach of ``torch.optim``
run in float64.  The figures it prints are the yardstick the GPU test's fp64 bound is
set from.  (No GPU, no library.)

No bit equality with torch's fp32 CPU result is asked: torch's vectorised CPU kernels
fuse ``add(alpha=)`` and ``addcmul`` into one multiply-add, so they are not
one-rounding-per-operation and differ from the twin in the last bit on most cases."""
import numpy as np
import pytest

import _optimizer_twin as tw

F32 = np.float32

# A buffer takes at most 5 roundings of half a unit in the last place per step (centred
# RMSprop's parameters: weight decay 2, addcdiv 3; every other buffer fewer), each
# relative to an element no larger than the buffer's maximum, and what it reads from
# the other buffers enters scaled by lr or by a weight below 1.  Over 6 steps that is
# 6 * 5 * 2^-24 = 1.8e-6 if every rounding went the same way; 2^-19 = 1.9e-6.  The
# measured figures are 4 to 20 times smaller; forming one complement
# weight from rounded constants, 1.f - 0.999f, costs 1.3e-5 and fails this.
TWIN_BOUND = 2.0 ** -19


def test_fma32_rounds_once_where_the_float64_shortcut_rounds_twice():
    a = F32(2.0 ** -4 + 2.0 ** -27)
    b = F32(1 - 2.0 ** -23)
    c = F32(2.0 ** 20 + 2.0 ** -3)
    # a * b + c = 2^20 + 2^-3 + 2^-4 - 2^-50: just below the midpoint of two floats
    assert float(a) == 2.0 ** -4 + 2.0 ** -27 and float(c) == 2.0 ** 20 + 2.0 ** -3
    assert float(tw.fma32(a, b, c)) == 2.0 ** 20 + 2.0 ** -3
    assert float(tw.fma32_exact(a, b, c)) == 2.0 ** 20 + 2.0 ** -3
    assert float(tw.fma32_shortcut(a, b, c)) == 2.0 ** 20 + 2.0 ** -2
    # the mirror image, just above a midpoint, and an exact tie (to even)
    assert float(tw.fma32(-a, b, -c)) == -(2.0 ** 20 + 2.0 ** -3)
    assert float(tw.fma32(F32(2.0 ** -4), F32(1), c)) == 2.0 ** 20 + 2.0 ** -2
    assert float(tw.fma32(F32(2.0 ** -4), F32(1), F32(2.0 ** 20))) == 2.0 ** 20
    # in an array, only the doubtful element is changed
    got = tw.fma32(np.array([a, F32(3)]), np.array([b, F32(5)]), np.array([c, F32(7)]))
    assert got.dtype == np.float32 and got.tolist() == [2.0 ** 20 + 2.0 ** -3, 22.0]


def test_fma32_edges():
    big = F32(np.finfo(np.float32).max)
    tiny = F32(2.0 ** -149)
    assert np.isposinf(tw.fma32(big, F32(2), F32(0)))
    assert np.isneginf(tw.fma32(big, F32(-2), F32(0)))
    assert tw.fma32(big, F32(1), F32(2.0 ** 102)) == big        # below the overflow tie
    assert np.isposinf(tw.fma32(big, F32(1), F32(2.0 ** 103)))  # on it: to even = inf
    assert np.isnan(tw.fma32(F32(np.nan), F32(1), F32(1)))
    assert np.isnan(tw.fma32(F32(np.inf), F32(0), F32(1)))
    assert float(tw.fma32(tiny, F32(0.5), F32(0))) == 0.0       # tie to even: zero
    assert float(tw.fma32(tiny, F32(0.75), F32(0))) == 2.0 ** -149
    assert float(tw.fma32(tiny, F32(0.5), tiny)) == 2.0 ** -148  # 1.5 -> even
    z = tw.fma32(F32(-0.0), F32(1), F32(-0.0))
    assert z == 0 and np.signbit(z)
    z = tw.fma32(F32(1), F32(1), F32(-1))
    assert z == 0 and not np.signbit(z)


def test_fma32_equals_the_shortcut_and_the_exact_sum_on_random_triples():
    rng = np.random.RandomState(0)
    a, b, c = rng.randn(3, 3000).astype(np.float32)
    got = tw.fma32(a, b, c)
    assert np.array_equal(got, tw.fma32_shortcut(a, b, c))
    exact = np.array([tw.fma32_exact(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), exact.view(np.uint32))
    # cancellation (the lerp shape: w * (g - m) + m with m near -w * (g - m))
    c2 = (-(a.astype(np.float64) * b)).astype(np.float32)
    got = tw.fma32(a, b, c2)
    exact = np.array([tw.fma32_exact(x, y, z) for x, y, z in zip(a, b, c2)])
    assert np.array_equal(got.view(np.uint32), exact.view(np.uint32))


def test_scalars_are_formed_in_double_and_rounded_once():
    """What separates the twin from fp32-formed complements."""
    for x in (0.999, 0.99, 0.9):
        assert tw._f(1 - x) == F32(1 - x)
        assert tw._f(1 - x) != F32(1) - F32(x)
    assert tw._f(1 - 0.1) == F32(1) - F32(0.1)  # this one happens to agree
    with pytest.raises(AssertionError):
        tw.lerp32(np.zeros(2, F32), np.ones(2, F32), F32(0.5))


def test_table_covers_what_it_claims():
    kinds = {(tw.CASES[t][0], tw.used_buffers(t)) for t in tw.CASES}
    assert ('SGD', ()) in kinds and ('SGD', ('momentum_buffer', )) in kinds
    assert ('RMSprop', ('square_avg', )) in kinds
    assert ('RMSprop', ('square_avg', 'grad_avg')) in kinds
    assert ('RMSprop', ('square_avg', 'momentum_buffer', 'grad_avg')) in kinds
    for name in ('Adam', 'AdamW'):
        assert (name, ('exp_avg', 'exp_avg_sq')) in kinds
        assert (name, ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')) in kinds
    assert any(s for _, _, s in tw.CASES.values())
    _, _, st = tw.case_inputs('adamw_amsgrad_step1000', 257)
    assert (st['exp_avg_sq'] >= 0).all() and (st['exp_avg_sq'] > 0).any()
    assert (st['max_exp_avg_sq'] >= st['exp_avg_sq']).all()
    assert np.abs(st['exp_avg']).max() > 0


@pytest.mark.parametrize('tag', list(tw.CASES))
def test_twin_stays_close_to_float64_torch(tag):
    """Parameters and every state buffer after 6 steps on 4099 elements, max|a - b| /
    max|b| per buffer against ``torch.optim`` in float64 on the same (widened) inputs."""
    _, history, ref = tw.twin_and_fp64(tag, 4099)
    assert set(ref) == {'p'} | set(tw.used_buffers(tag))
    errs = {k: tw.rel_err(history[-1][k], ref[k]) for k in ref}
    print('twin vs float64 torch: %-28s %s' % (
        tag, '  '.join('%s %.2e' % kv for kv in errs.items())))
    for k, e in errs.items():
        assert history[-1][k].dtype == np.float32 and np.isfinite(ref[k]).all()
        assert e <= TWIN_BOUND, (tag, k, e)


def test_fp32_formed_complements_would_not_pass(monkeypatch):
    """The bound above tells the two ways of forming ``1 - beta2`` apart: the same twin
    with its scalars formed from constants already rounded misses it on exp_avg_sq."""
    real = tw._f

    def fp32_formed(x):
        for c in (0.999, 0.99):
            if x == 1 - c:
                return F32(1) - F32(c)
        return real(x)

    monkeypatch.setattr(tw, '_f', fp32_formed)
    _, history, ref = tw.twin_and_fp64('adamw_amsgrad', 4099)
    assert tw.rel_err(history[-1]['exp_avg_sq'], ref['exp_avg_sq']) > 4 * TWIN_BOUND
