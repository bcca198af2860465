"""Every dispatch of ``ga_gae_scan_f32`` against one literal fp64 reference, under a
one-ulp bar, and the small reductions that share its buffers (GPU box).

The reference below is the padded recurrence itself, NOT the closed form of the
padded tail that the kernels (and ``oracle.returns.gae_ragged_closed_form_f64``)
use: for an episode of ``L`` steps the whole row of ``P = max_episode_length``
cells is built (rewards 0 and baselines ``v0`` in the padding, the constant bonus
in every cell) and ``A_t = (r_t + bonus_t) + g32 V_{t+1} - V_t + c32 A_{t+1}`` is
run backwards over all ``P`` cells in numpy float64.

Tolerance: both kernels run both recurrences in fp64 registers and round once on
store, so the bar is the rounding of that single cast,
``|got - ref| <= spacing(float32(|ref|)) + 1e-9 * max|ref| of the row``
(the second term covers the fp64 association order: lane-wise composition, the
suffix scan and the closed-form tail against the plain backward loop).

Which kernel runs is decided on the host (``ga_gae_scan_f32``); the library only
counts scan launches as one kind, so ``_host_dispatch`` restates those rules and
every case asserts that its inputs select the kernel it is meant for:

  rows<1>         mode 1, no bonus array, max_len <= 256, 16-B aligned bases
  rows<2>         the same after ga_set_gae_rows_steps_per_lane(8), max_len > 4
  general<true>   fast path off / bonus array / max_len > 256 / mode 0, with 16-B
                  aligned bases and (row stride % 4 == 0 or packed offsets)
  general<false>  the same with a row stride that is no multiple of 4, or bases
                  4 bytes off alignment
"""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GA_PROF_GAE_SCAN = 6  # csrc/prof.h: every gae_scan kernel counts as this kind

# (discount, gae_lambda, v0, bonus_const): every value of the four lists
#   (g, lam) in {(0.99, 0.95), (1, 1), (0.99, 0), (1, 0.9999999), (0.5, 1)},
#   v0 in {0, 0.37, -2.5}, bonus_const in {0, 0.11}
# appears; (1, 1) -- the geo = m - 1 arm of the padded tail -- comes with v0 != 0
# and bonus_const != 0.
COMBOS = [
    (0.99, 0.95, 0.37, 0.11),
    (1.0, 1.0, -2.5, 0.11),
    (0.99, 0.0, 0.0, 0.0),
    (1.0, 0.9999999, 0.37, 0.0),
    (0.5, 1.0, -2.5, 0.11),
]
GAMMA_LAMBDA_ONE = 1  # index of (1, 1, ...) in COMBOS

# dispatch name -> (fixed fast path, steps per lane)
SETTERS = {
    'rows<1>': (1, 4),
    'rows<2>': (1, 8),
    'general<true>': (0, 4),
    'general<false>': (0, 4),
}


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


_state = {'fast': 1, 'steps': 4}


@contextlib.contextmanager
def _scan_setters(fast, steps):
    """Set both dispatch switches of the scan; always back to (1, 4) afterwards."""
    from garage_amd import _lib
    lib = _lib.load()
    try:
        lib.ga_set_gae_fixed_fast_path(fast)
        lib.ga_set_gae_rows_steps_per_lane(steps)
        _state.update(fast=fast, steps=steps)
        yield
    finally:
        lib.ga_set_gae_rows_steps_per_lane(4)
        lib.ga_set_gae_fixed_fast_path(1)
        _state.update(fast=1, steps=4)


def _host_dispatch(arrays, tail, packed, ld, max_len, has_bonus):
    """The kernel ``ga_gae_scan_f32`` picks for these arguments (its host rules)."""
    mode = 0 if tail is not None else 1
    aligned = all(t.data_ptr() % 16 == 0 for t in arrays)
    if _state['fast'] and mode == 1 and not has_bonus and max_len <= 256 and \
            aligned:
        return 'rows<2>' if _state['steps'] == 8 and max_len > 4 else 'rows<1>'
    vec = (packed or ld % 4 == 0) and aligned and (
        tail is None or tail.data_ptr() % 8 == 0)
    return 'general<true>' if vec else 'general<false>'


# ---------------------------------------------------------------------------
# the reference (1a) and the bound (1b)
def _reference(rew, val, bon, lens, P, discount, gae_lambda, v0, bonus_const):
    """Literal padded semantics in float64.  ``rew`` / ``val`` / ``bon`` (or None):
    the packed fp32 steps of episodes of ``lens`` steps.  Returns the advantages
    and returns of the valid steps, packed, and for every step the largest
    |advantage| / |return| of its row."""
    n = len(lens)
    g32 = float(np.float32(discount))
    c32 = float(np.float32(discount * gae_lambda))  # double product, rounded once
    v0 = float(np.float32(v0))
    bc = float(np.float32(bonus_const))
    assert lens.min() >= 1 and lens.max() <= P
    valid = np.arange(P)[None, :] < lens[:, None]  # row-major = packed order
    R = np.zeros((n, P), np.float64)
    V = np.full((n, P + 1), v0, np.float64)
    V[:, P] = 0.0
    B = np.full((n, P), bc, np.float64)
    R[valid] = rew
    V[:, :P][valid] = val
    if bon is not None:
        B[valid] += bon
    A = np.zeros((n, P + 1), np.float64)
    G = np.zeros((n, P + 1), np.float64)
    for t in range(P - 1, -1, -1):
        A[:, t] = (R[:, t] + B[:, t]) + g32 * V[:, t + 1] - V[:, t] + \
            c32 * A[:, t + 1]
        # rewards are 0 beyond L, so G is exactly 0 there: the recursion over the
        # L valid steps
        G[:, t] = R[:, t] + float(discount) * G[:, t + 1]
    amax = np.where(valid, np.abs(A[:, :P]), 0.0).max(1)
    gmax = np.where(valid, np.abs(G[:, :P]), 0.0).max(1)
    return (A[:, :P][valid], G[:, :P][valid], np.repeat(amax, lens),
            np.repeat(gmax, lens))


class _Problem:
    pass


@functools.lru_cache(maxsize=None)
def _problem(lens, P, combo, use_bonus, seed):
    """Episodes of the given lengths with their reference, computed once and
    shared (read-only) by every dispatch that runs them."""
    rng = np.random.RandomState(seed)
    S = int(sum(lens))
    p = _Problem()
    p.lens = np.asarray(lens, np.int64)
    p.off = np.concatenate([[0], np.cumsum(p.lens)]).astype(np.int64)
    p.rew = rng.randn(S).astype(np.float32)
    p.val = rng.randn(S).astype(np.float32)
    p.bon = (0.3 * rng.rand(S)).astype(np.float32) if use_bonus else None
    g, lam, v0, bc = COMBOS[combo]
    p.adv, p.ret, p.amax, p.gmax = _reference(p.rew, p.val, p.bon, p.lens, P, g,
                                              lam, v0, bc)
    for a in (p.rew, p.val, p.adv, p.ret, p.amax, p.gmax, p.off):
        a.setflags(write=False)
    return p


def _assert_one_ulp(got, ref, rowmax, what):
    """``|got - ref| <= spacing(float32(|ref|)) + 1e-9 * max|ref| of the row``."""
    assert got.dtype == np.float32
    bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + \
        1e-9 * rowmax
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)  # a NaN is bad too
    if bad.any():
        k = int(np.argmax(np.where(bad, err / bound, 0.0)))
        raise AssertionError(
            '{}: {} of {} steps outside one fp32 ulp; worst at packed step {}: '
            'got {!r}, reference {!r}, error {:.3e}, bound {:.3e}'.format(
                what, int(bad.sum()), bad.size, k, float(got[k]), float(ref[k]),
                float(err[k]), float(bound[k])))


def _launches():
    from garage_amd import _lib
    return _lib.load().ga_launch_count(GA_PROF_GAE_SCAN)


# ---------------------------------------------------------------------------
# layouts
def _run_packed(dev, prob, P, combo, max_len, misalign, want, what):
    """Packed 1-D arrays with ``offsets``.  Every buffer has a tail (NaN behind the
    inputs, a sentinel behind the outputs); with ``misalign`` the arrays are
    ``[1:]`` views, 4 bytes off the 16-B alignment of the allocation."""
    from garage_amd.engine import gae_scan
    S, lead, slack = int(prob.off[-1]), int(misalign), 8

    def upload(x, fill):
        host = np.full(lead + S + slack, fill, np.float32)
        if x is not None:
            host[lead:lead + S] = x
        buf = torch.from_numpy(host).to(dev)
        return buf, buf[lead:lead + S]

    _, rew = upload(prob.rew, np.nan)
    _, val = upload(prob.val, np.nan)
    bon = None if prob.bon is None else upload(prob.bon, np.nan)[1]
    adv_buf, adv = upload(None, SENTINEL)
    ret_buf, ret = upload(None, SENTINEL)
    arrays = [t for t in (rew, val, bon, adv, ret) if t is not None]
    ran = _host_dispatch(arrays, None, True, 0, max_len, bon is not None)
    assert ran == want, (what, ran)
    g, lam, v0, bc = COMBOS[combo]
    before = _launches()
    gae_scan(rew, val, discount=g, gae_lambda=lam, max_episode_length=P,
             offsets=torch.from_numpy(prob.off).to(dev), max_len=max_len, v0=v0,
             bonus=bon, bonus_const=bc, adv=adv, ret=ret)
    assert _launches() == before + 1
    for name, buf, ref, rowmax in (('adv', adv_buf, prob.adv, prob.amax),
                                   ('ret', ret_buf, prob.ret, prob.gmax)):
        host = buf.cpu().numpy()
        assert (host[:lead] == SENTINEL).all() and \
            (host[lead + S:] == SENTINEL).all(), (what, name, 'wrote outside')
        _assert_one_ulp(host[lead:lead + S], ref, rowmax,
                        '{} {} {}'.format(what, ran, name))


def _run_rows(dev, prob, N, T, ld, pos, P, combo, want, what, tail=None):
    """``(N, T)`` views of ``(N, ld)`` buffers; ``pos`` = position of every packed
    step of ``prob`` in the flattened buffer.  Slack columns hold NaN (inputs) or a
    sentinel (outputs); steps of the view outside ``pos`` (mode 0: unfinished
    episodes) hold ordinary data and are not compared."""
    from garage_amd.engine import gae_scan
    rng = np.random.RandomState(N * 1000 + T)

    def upload(x, fill, dtype=np.float32):
        host = np.full((N, ld), fill, dtype)
        if x is not None:
            host[:, :T] = rng.randn(N, T)
            host.reshape(-1)[pos] = x
        buf = torch.from_numpy(host).to(dev)
        return buf, buf[:, :T]

    _, rew = upload(prob.rew, np.nan)
    _, val = upload(prob.val, np.nan)
    bon = None if prob.bon is None else upload(prob.bon, np.nan)[1]
    adv_buf, adv = upload(None, SENTINEL)
    ret_buf, ret = upload(None, SENTINEL)
    tail_dev = None if tail is None else torch.from_numpy(tail).to(dev)
    arrays = [t for t in (rew, val, bon, adv, ret) if t is not None]
    ld_host = ld if N > 1 else T  # the engine passes T for a single row
    ran = _host_dispatch(arrays, tail_dev, False, ld_host, T, bon is not None)
    assert ran in want, (what, ran)
    g, lam, v0, bc = COMBOS[combo]
    before = _launches()
    gae_scan(rew, val, discount=g, gae_lambda=lam, max_episode_length=P,
             tail=tail_dev, v0=v0, bonus=bon, bonus_const=bc, adv=adv, ret=ret)
    assert _launches() == before + 1
    for name, buf, ref, rowmax in (('adv', adv_buf, prob.adv, prob.amax),
                                   ('ret', ret_buf, prob.ret, prob.gmax)):
        host = buf.cpu().numpy()
        assert (host[:, T:] == SENTINEL).all(), (what, name, 'wrote the slack')
        _assert_one_ulp(host.reshape(-1)[pos], ref, rowmax,
                        '{} {} {}'.format(what, ran, name))
    return ran


def _row_positions(N, T, ld):
    return (np.arange(N)[:, None] * ld + np.arange(T)[None, :]).reshape(-1)


# ---------------------------------------------------------------------------
# packed batches of short episodes: both fast paths, both general instantiations
SHORT_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256]


def _short_lens():
    """The 13 lengths, shuffled, five times over: 65 rows -- lanes with no, a
    partial and a full quad, row ends on lane boundaries, the 8-step lane that
    holds exactly 4 valid steps, row starts at every residue modulo 4."""
    rng = np.random.RandomState(13)
    lens = np.concatenate([rng.permutation(SHORT_LENS) for _ in range(5)])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert set(starts % 4) == {0, 1, 2, 3}
    return tuple(int(v) for v in lens)


# P - L of {0, 1} (256: L = 256, 255), {1, 2} (257), large (all; 1000: up to 999)
SHORT_P = [256, 257, 1000]


@pytest.mark.parametrize('combo', range(len(COMBOS)))
@pytest.mark.parametrize('dispatch', list(SETTERS))
def test_packed_short_episodes(dev, dispatch, combo):
    lens = _short_lens()
    with _scan_setters(*SETTERS[dispatch]):
        for P in SHORT_P:
            _run_packed(dev, _problem(lens, P, combo, False, 100 + P), P, combo,
                        256, dispatch == 'general<false>', dispatch,
                        ('packed', P, COMBOS[combo]))


@pytest.mark.parametrize('combo', range(len(COMBOS)))
@pytest.mark.parametrize('dispatch', ['general<true>', 'general<false>'])
def test_packed_short_episodes_with_bonus_array(dev, dispatch, combo):
    """A per-step bonus selects the general kernels by itself: the switches stay
    at their defaults."""
    lens = _short_lens()
    for P in SHORT_P:
        _run_packed(dev, _problem(lens, P, combo, True, 200 + P), P, combo, 256,
                    dispatch == 'general<false>', dispatch,
                    ('packed+bonus', P, COMBOS[combo]))


@pytest.mark.parametrize('steps', [4, 8])
def test_packed_misaligned_views_leave_the_fast_paths(dev, steps):
    """The constant-decay kernels choose their 16-B accesses from step indices
    alone: arrays that start 4 bytes off alignment go to the scalar-access general
    kernel although both switches ask for a fast path."""
    lens = _short_lens()
    with _scan_setters(1, steps):
        for combo in (0, GAMMA_LAMBDA_ONE):
            _run_packed(dev, _problem(lens, 257, combo, False, 357), 257, combo,
                        256, True, 'general<false>',
                        ('misaligned', steps, COMBOS[combo]))


# rows of more than 256 steps: the chunked walk of the general kernels.  Starts
# 0, 512, 812 are 4-float aligned (16-B accesses in general<true>), 1069 and 1582
# are not.
LONG_LENS = (512, 300, 257, 513, 1)


@pytest.mark.parametrize('combo', range(len(COMBOS)))
@pytest.mark.parametrize('dispatch', ['general<true>', 'general<false>'])
def test_packed_long_episodes_chunked_walk(dev, dispatch, combo):
    for P in (513, 1000):
        for use_bonus in (False, True):
            _run_packed(dev, _problem(LONG_LENS, P, combo, use_bonus, 300 + P), P,
                        combo, 513, dispatch == 'general<false>', dispatch,
                        ('long', P, use_bonus, COMBOS[combo]))


# ---------------------------------------------------------------------------
# padded (N, T) batches
PADDED_VARIANTS = {
    # name -> (setters, bonus array, kernels the host rules may pick)
    'rows<1>': ((1, 4), False, ('rows<1>', )),
    # (rows of at most 4 steps stay on rows<1>: one quad per lane is all there is)
    'rows<2>': ((1, 8), False, ('rows<1>', 'rows<2>')),
    'general': ((0, 4), False, ('general<true>', 'general<false>')),
    'general+bonus': ((1, 4), True, ('general<true>', 'general<false>')),
}


# 20, 33 and 100 fill in the lanes-per-row values between those of 9 and 256 (4
# steps per lane: 1, 1, 2, 4, 8, 16, 32, 64 lanes; 8 steps: -, -, 1, 2, 4, 8, 16,
# 32): the suffix scan of the 8-step path first multiplies by a host-built power
# of the decay with 4 lanes per row, i.e. from 17 steps on.
@pytest.mark.parametrize('T', [1, 4, 5, 9, 20, 33, 100, 256])
@pytest.mark.parametrize('variant', list(PADDED_VARIANTS))
def test_padded_rows(dev, variant, T):
    """``ld == T``; 65 rows leave a ragged last wave for every lanes-per-row
    value.  The 12 (N, P - L) pairs cycle through the parameter lines, (1, 1)
    falling on P - L = 1, 2 and 500."""
    setters, use_bonus, want = PADDED_VARIANTS[variant]
    ran = set()
    with _scan_setters(*setters):
        k = 0
        for N in (1, 3, 65):
            for m in (0, 1, 2, 500):
                combo = k % len(COMBOS)
                k += 1
                prob = _problem((T, ) * N, T + m, combo, use_bonus, 400 + k)
                ran.add(_run_rows(dev, prob, N, T, T, _row_positions(N, T, T),
                                  T + m, combo, want,
                                  ('padded', N, T, m, COMBOS[combo])))
    if variant == 'rows<2>':
        assert ran == {'rows<2>' if T > 4 else 'rows<1>'}
    if variant.startswith('general'):
        assert ran == {'general<true>' if T % 4 == 0 else 'general<false>'}


@pytest.mark.parametrize('slack', [3, 4])
@pytest.mark.parametrize('variant', list(PADDED_VARIANTS))
def test_padded_rows_with_a_wider_stride(dev, variant, slack):
    """``buf[:, :9]`` of ``(N, 12)`` and ``(N, 13)`` buffers, all four (five)
    arrays sharing the stride; the slack columns of the outputs stay untouched."""
    setters, use_bonus, want = PADDED_VARIANTS[variant]
    T, ld = 9, 9 + slack
    with _scan_setters(*setters):
        k = 0
        for N in (3, 65):
            for m in (0, 1, 2, 500):
                combo = (k + 1) % len(COMBOS)
                k += 1
                prob = _problem((T, ) * N, T + m, combo, use_bonus, 500 + k)
                ran = _run_rows(dev, prob, N, T, ld, _row_positions(N, T, ld),
                                T + m, combo, want,
                                ('strided', N, ld, m, COMBOS[combo]))
                if variant.startswith('general'):
                    assert ran == ('general<true>' if ld % 4 == 0 else
                                   'general<false>')
                elif variant == 'rows<2>':
                    assert ran == 'rows<2>'


@pytest.mark.parametrize('T,ld', [(7, 7), (5, 7), (9, 9), (301, 301),
                                  (256, 301)])
def test_padded_rows_scalar_general_kernel(dev, T, ld):
    """Row strides that are no multiple of 4 (301: an equal-length batch of
    ``max_episode_length = 301`` viewed as ``(N, longest)``) must take
    ``gae_scan_kernel<false>``."""
    k = 0
    for use_bonus in (False, True):
        # without a bonus array, rows of at most 256 steps need the switch
        with _scan_setters(0 if T <= 256 and not use_bonus else 1, 4):
            for m in (0, 1, 2, 500):
                for combo in (k % len(COMBOS), GAMMA_LAMBDA_ONE):
                    prob = _problem((T, ) * 5, T + m, combo, use_bonus, 600 + k)
                    _run_rows(dev, prob, 5, T, ld, _row_positions(5, T, ld),
                              T + m, combo, ('general<false>', ),
                              ('scalar', T, ld, m, use_bonus, COMBOS[combo]))
                k += 1


# ---------------------------------------------------------------------------
# mode 0: several episodes per env row, marked by tail flags
def _tail_plan(T, P):
    """Rows of episode lengths (sum <= T; what is left are unfinished steps)."""

    def ending_at(ends):
        out, t = [], 0
        for e in sorted(set(e for e in ends if 0 < e <= T)):
            while t < e:
                out.append(min(P, e - t))
                t += out[-1]
        return out

    rng = np.random.RandomState(T * 7 + P)
    rows = [
        [1] * T,  # length 1 throughout; the last one ends on the row's last step
        ending_at(range(4, T + 1, 4)),  # an end on every 4-step lane boundary
        ending_at([256, 512, T]),  # on the 256-step chunk boundaries, then on T
        # (where P allows) an episode over steps 3..4: across a lane boundary;
        # one that starts at step 255: across a lane and a chunk boundary
        ending_at([3, 5, 255, 255 + min(P, 5)]),
        ending_at([T - 2]),  # two unfinished steps behind the last episode
    ]
    for _ in range(6):
        row, t = [], 0
        while True:
            L = int(rng.randint(1, P + 1))
            if t + L > T:
                break
            row.append(L)
            t += L
        rows.append(row)
    eps = [(i, s, L) for i, row in enumerate(rows)
           for s, L in zip(np.concatenate([[0], np.cumsum(row)[:-1]]), row)]
    # the plan holds what it is meant to hold

    def crosses(q):
        return [(s, L) for _, s, L in eps if s // q != (s + L - 1) // q]

    assert any(L == 1 for _, _, L in eps)
    assert any(s + L == T for _, s, L in eps)
    assert any(sum(row) < T for row in rows)
    assert T < 4 or any((s + L) % 4 == 0 for _, s, L in eps)
    assert T < 256 or any(s + L == 256 for _, s, L in eps)
    assert P < 2 or crosses(4)
    assert P < 2 or T <= 256 or crosses(256)
    return len(rows), eps


@pytest.mark.parametrize('P', [1, 5, 100])
@pytest.mark.parametrize('T', [7, 36, 260, 515])
def test_rollout_buffer_tail_flags(dev, T, P):
    """Asserted on finished episodes only.  ``T`` of 36 and 260 take
    ``gae_scan_kernel<true>``, 7 and 515 (stride no multiple of 4) ``<false>``."""
    n, eps = _tail_plan(T, P)
    lens = tuple(int(L) for _, _, L in eps)
    pos = np.concatenate([i * T + s + np.arange(L) for i, s, L in eps])
    tail = np.zeros((n, T), np.uint16)
    for i, s, L in eps:
        tail[i, s + L - 1] = L
    want = ('general<true>' if T % 4 == 0 else 'general<false>', )
    for combo in range(len(COMBOS)):
        for use_bonus in (False, True):
            prob = _problem(lens, P, combo, use_bonus, 700 + combo)
            _run_rows(dev, prob, n, T, T, pos, P, combo, want,
                      ('tails', T, P, use_bonus, COMBOS[combo]), tail=tail)


# ---------------------------------------------------------------------------
# engine.gae_scan with strided views
def test_gae_scan_allocates_outputs_with_the_input_stride(dev):
    """Without ``adv`` / ``ret`` the outputs of a ``buf[:, :T]`` call get the
    inputs' row stride (the library takes one stride for every array)."""
    from garage_amd.engine import gae_scan
    N, T, combo = 65, 9, 0
    g, lam, v0, bc = COMBOS[combo]
    for ld, fast in ((12, 1), (13, 1), (13, 0)):
        prob = _problem((T, ) * N, T + 2, combo, False, 800 + ld)
        host = np.full((2, N, ld), np.nan, np.float32)
        host[0, :, :T] = prob.rew.reshape(N, T)
        host[1, :, :T] = prob.val.reshape(N, T)
        buf = torch.from_numpy(host).to(dev)
        with _scan_setters(fast, 4):
            adv, ret = gae_scan(buf[0, :, :T], buf[1, :, :T], discount=g,
                                gae_lambda=lam, max_episode_length=T + 2, v0=v0,
                                bonus_const=bc)
        for name, out, ref, rowmax in (('adv', adv, prob.adv, prob.amax),
                                       ('ret', ret, prob.ret, prob.gmax)):
            assert out.shape == (N, T) and out.stride() == (ld, 1), (name, ld)
            _assert_one_ulp(out.cpu().numpy().reshape(-1), ref, rowmax,
                            'default outputs ld={} {}'.format(ld, name))
    # contiguous and packed inputs keep getting contiguous outputs
    r = torch.zeros(4, 8, device=dev)
    adv, ret = gae_scan(r, r, discount=0.9, gae_lambda=0.9, max_episode_length=8)
    assert adv.is_contiguous() and ret.is_contiguous()


def test_gae_scan_refuses_mismatched_strides_before_any_launch(dev):
    from garage_amd.engine import gae_scan
    N, T = 6, 9
    wide = lambda: torch.zeros(N, T + 4, device=dev)[:, :T]
    tight = lambda: torch.zeros(N, T, device=dev)
    transposed = lambda: torch.zeros(T, N, device=dev).t()
    kw = dict(discount=0.99, gae_lambda=0.95, max_episode_length=T)
    before = _launches()
    cases = [
        dict(rewards=wide(), values=tight()),
        dict(rewards=wide(), values=wide(), adv=tight()),
        dict(rewards=wide(), values=wide(), ret=tight()),
        dict(rewards=wide(), values=wide(), adv=wide(), ret=tight()),
        dict(rewards=wide(), values=wide(), bonus=tight()),
        dict(rewards=tight(), values=tight(), adv=wide()),
        dict(rewards=tight(), values=tight(),
             tail=torch.zeros(N, T + 3, dtype=torch.int16, device=dev)[:, :T]),
        # rows that are not unit-stride
        dict(rewards=transposed(), values=transposed()),
        dict(rewards=tight(), values=tight(), ret=transposed()),
        dict(rewards=tight(), values=tight(), bonus=transposed()),
    ]
    for case in cases:
        r, v = case.pop('rewards'), case.pop('values')
        with pytest.raises(ValueError):
            gae_scan(r, v, **kw, **case)
    # packed arrays: a strided 1-D view
    flat = torch.zeros(40, device=dev)
    off = torch.tensor([0, 7, 20], device=dev)
    with pytest.raises(ValueError):
        gae_scan(flat[:20], flat[:20], offsets=off, max_len=13,
                 adv=flat[::2], **kw)
    assert _launches() == before


# ---------------------------------------------------------------------------
# the reductions that share those buffers
def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('center,positive', [(True, False), (False, True),
                                             (True, True)])
@pytest.mark.parametrize('n', [2, 255, 256, 257, 131072, 131073, 300001])
def test_center_advantages_sizes(dev, n, center, positive):
    """``ga_stats_f32`` / ``ga_adv_center_f32`` / ``ga_sub_scalar_f32`` from one
    thread to the grid-stride loop (more than 512 blocks x 256 threads = 131072
    elements).  Reference: float64 mean, unbiased variance and minimum, then
    ``(x - float32(mean)) / (float32(var) + 1e-8)`` in fp32 as the kernel (and
    the reference implementation) does it.  The statistics are exact to fp64 and
    the subtract and divide are correctly rounded: 2 fp32 ulp of the result."""
    from garage_amd.engine import center_advantages
    rng = np.random.RandomState(n)
    x = (rng.randn(n) * 3 + 1).astype(np.float32)
    want = x.copy()
    if center:
        x64 = x.astype(np.float64)
        mean = math.fsum(x64) / n
        var = math.fsum((x64 - mean)**2) / (n - 1)
        want = (want - np.float32(mean)) / (np.float32(var) + np.float32(1e-8))
        assert want.dtype == np.float32
    if positive:
        want = want - want.min()
    got = center_advantages(torch.from_numpy(x.copy()).to(dev), center=center,
                            positive=positive).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= 2 * _ulp32(want)).all(), (n, float(err.max()))


@pytest.mark.parametrize('n_eps', [1, 255, 256, 257])
def test_episode_sums(dev, n_eps):
    """``ga_episode_sums_f32`` (one thread per episode, sequential fp64 sum)
    against ``math.fsum``: ``1e-12 * sum|x|``."""
    from garage_amd._lib import call, dptr, stream_ptr
    rng = np.random.RandomState(n_eps)
    lens = rng.randint(1, 120, size=n_eps)
    lens[::7] = 1
    lens[-1] = 300
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = (rng.randn(int(off[-1])) * 10).astype(np.float32)
    sums = torch.full((n_eps + 1, ), SENTINEL, dtype=torch.float64, device=dev)
    xd, od = torch.from_numpy(x).to(dev), torch.from_numpy(off).to(dev)
    call('ga_episode_sums_f32', dptr(xd), dptr(od), n_eps, dptr(sums),
         stream_ptr())
    got = sums.cpu().numpy()
    assert got[n_eps] == SENTINEL
    for e in range(n_eps):
        seg = x[off[e]:off[e + 1]].astype(np.float64)
        assert abs(got[e] - math.fsum(seg)) <= 1e-12 * np.abs(seg).sum(), e


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 70001])
def test_dot(dev, n):
    """``ga_dot_f32`` (one block of 1024 threads striding over n, fp64
    accumulation) against the exact sum of the (exact) fp64 products."""
    from garage_amd._lib import call, dptr, stream_ptr
    rng = np.random.RandomState(n)
    a = rng.randn(n).astype(np.float32)
    b = rng.randn(n).astype(np.float32)
    out = torch.full((2, ), SENTINEL, dtype=torch.float64, device=dev)
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    call('ga_dot_f32', dptr(ad), dptr(bd), n, dptr(out), stream_ptr())
    got = out.cpu().numpy()
    prod = a.astype(np.float64) * b.astype(np.float64)
    assert got[1] == SENTINEL
    assert abs(got[0] - math.fsum(prod)) <= 1e-12 * np.abs(prod).sum()


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 70001])
def test_axpby(dev, n):
    """``ga_axpby_f32`` (one element per thread): ``y = alpha x + beta y`` with the
    coefficients rounded to fp32 first.  The kernel may or may not contract to an
    fma, so the bar is one fp32 ulp of ``|alpha x| + |beta y|``, not of the
    result; nothing behind ``y[n - 1]`` is written."""
    from garage_amd._lib import call, dptr, stream_ptr
    rng = np.random.RandomState(n)
    x = rng.randn(n).astype(np.float32)
    y = rng.randn(n).astype(np.float32)
    alpha, beta = 0.7, -1.3  # neither is an fp32 number
    yd = torch.full((n + 3, ), SENTINEL, device=dev)
    yd[:n] = torch.from_numpy(y).to(dev)
    xd = torch.from_numpy(x).to(dev)
    call('ga_axpby_f32', alpha, dptr(xd), beta, dptr(yd), n, stream_ptr())
    got = yd.cpu().numpy()
    ax = float(np.float32(alpha)) * x.astype(np.float64)
    by = float(np.float32(beta)) * y.astype(np.float64)
    want = (ax + by).astype(np.float32)
    assert (got[n:] == SENTINEL).all()
    err = np.abs(got[:n].astype(np.float64) - want.astype(np.float64))
    assert (err <= _ulp32(np.abs(ax) + np.abs(by))).all(), float(err.max())
