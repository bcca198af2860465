"""The cases of ``ga_advantages_members_f32`` and a plain fp64 reference.

A case is one launch: members of differing shape, one padding length ``P``.  A member is
``(layout, shape, v0, bonus_const)``: ``('matrix', (N, L, ld))`` equal-length episodes as
an ``(N, L)`` view of ``(N, ld)`` buffers, or ``('ragged', lengths)`` packed episodes with
offsets; ``v0`` ``None`` is the null pointer (0.0).  Sample counts: 1, 255 / 256 / 257
(the steps of ``ga_red_blocks``), 1030 (five virtual blocks: a quarter plays two) and
32768 (the cap); rows of 4, 7 and 256 steps (``L < P`` and ``L == P``), odd ragged lengths
(unaligned starts), rows of 257 and 600 steps (the general kernel, across chunks), rows
``ld > L`` apart.

Tolerances.  Raw advantages and returns: the one-ulp bar of ``test_gae_scan_edges_gpu.py``.
Normalised advantages: with ``u = 2**-23`` and ``scale = (max|a| + |mean|) / (var + 1e-8)``
(``max|a|`` without centring) the bound is ``u * scale * (8 centred, else 1; + 3 with
positive_adv)``: per element the numerator carries one ulp of the raw advantage, half an
ulp each of the fp32 mean and of the difference (1.5 u), the denominator four roundings of
2**-24 (the fp32 inputs of the variance, its cast, the added epsilon: 2 u), the quotient
half an ulp (0.5 u) -- 4 u -- and the subtracted minimum, itself such a value, one more;
doubled, so that an fp32 restatement of the lone arithmetic (``restate_f32``) stays within
half of it.  Worst ratio of that restatement over these cases: 0.31
(``test_advantage_cases_cpu.py`` asserts <= 0.5).
"""
import numpy as np

U = 2.0 ** -23
DISCOUNT, GAE_LAMBDA = 0.99, 0.95
SEVENS = (7, ) * 35 + (5, 3, 1, 1)

# name -> (P, members)
CASES = {
    'one-sample': (8, [('matrix', (1, 1, 1), 0.37, 0.11)]),
    'block-steps': (7, [('ragged', SEVENS, 0.37, 0.0),              # S = 255
                        ('matrix', (64, 4, 4), None, 0.11),          # S = 256
                        ('ragged', (7, ) * 36 + (5, ), -2.5, 0.11)]),  # S = 257
    'mixed-kernels': (600, [('ragged', (257, ), 0.37, 0.0),
                            ('ragged', (600, 3), None, 0.11),
                            ('matrix', (4, 256, 256), -2.5, 0.0),
                            ('ragged', (7, ) * 147 + (1, ), 0.37, 0.11),  # S = 1030
                            ('matrix', (5, 7, 12), 0.37, 0.11)]),
    'cap': (256, [('matrix', (128, 256, 256), 0.37, 0.0)]),           # S = 32768
}
OPTIONS = [(c, p) for c in (False, True) for p in (False, True)]  # (centre, positive)


def lengths(member):
    layout, shape = member[:2]
    return np.full(shape[0], shape[1], np.int64) if layout == 'matrix' else \
        np.asarray(shape, np.int64)


def inputs(name, m):
    """Packed fp32 rewards and values of member ``m`` of case ``name``."""
    rng = np.random.RandomState(100 * sorted(CASES).index(name) + m)
    S = int(lengths(CASES[name][1][m]).sum())
    return rng.randn(S).astype(np.float32), rng.randn(S).astype(np.float32)


def reference(rew, val, lens, P, v0, bonus, center, positive):
    """Padded-tail returns and GAE run backwards over all ``P`` cells in
    fp64, then unbiased variance, ``(a - mean) / (var + 1e-8)`` and the minimum shift.
    Returns raw advantages, returns, final advantages, the row maxima of the first two
    (for the one-ulp bar) and the normalisation's ``scale``."""
    g32, c32 = float(np.float32(DISCOUNT)), float(np.float32(DISCOUNT * GAE_LAMBDA))
    v0 = 0.0 if v0 is None else float(np.float32(v0))
    n = len(lens)
    valid = np.arange(P)[None, :] < lens[:, None]
    R, V = np.zeros((n, P)), np.full((n, P + 1), v0)
    V[:, P] = 0.0
    R[valid], V[:, :P][valid] = rew, val
    A, G = np.zeros((n, P + 1)), np.zeros((n, P + 1))
    for t in range(P - 1, -1, -1):
        A[:, t] = (R[:, t] + float(np.float32(bonus))) + g32 * V[:, t + 1] - V[:, t] + \
            c32 * A[:, t + 1]
        G[:, t] = R[:, t] + DISCOUNT * G[:, t + 1]
    raw, ret = A[:, :P][valid], G[:, :P][valid]
    amax = np.repeat(np.where(valid, np.abs(A[:, :P]), 0.0).max(1), lens)
    gmax = np.repeat(np.where(valid, np.abs(G[:, :P]), 0.0).max(1), lens)
    adv, scale = normalise(raw, center, positive, np.float64)
    return raw, ret, adv, amax, gmax, scale


def normalise(a, center, positive, dtype):
    """The normalisation with fp64 moments; the elementwise part in ``dtype``."""
    scale = np.abs(a).max()
    x = a.astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        if center:
            mean = a.astype(np.float64).sum() / len(a)
            var = ((a.astype(np.float64) - mean) ** 2).sum() / (len(a) - 1.0)
            scale = (scale + abs(mean)) / (var + 1e-8)
            x = (x - dtype(mean)) / (dtype(var) + dtype(1e-8))
        if positive:
            x = x - x.min() if not np.isnan(x).all() else x
    return x, scale


def restate_f32(raw, center, positive):
    """The lone arithmetic in numpy fp32 on the fp32-rounded raw advantages."""
    return normalise(raw.astype(np.float32), center, positive, np.float32)[0]


def bound(scale, center, positive):
    return U * scale * ((8.0 if center else 1.0) + (3.0 if positive else 0.0))
