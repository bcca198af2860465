"""The case table of the linear feature baseline's tests, their inputs, and an fp64
numpy twin of ``garage.np.baselines.LinearFeatureBaseline``.

Shared by ``tests/golden/make_golden_linear_baseline.py`` (which feeds the same
inputs to the REAL class and stores what it answers),
``test_linear_baseline_cpu.py`` (twin against golden, conditioning of the cases),
``test_linear_baseline_gpu.py`` and ``test_linear_baseline_algos_gpu.py`` (device
against twin).  numpy only.

A case is ``(name, obs_dim, episode lengths, ld_extra)``; ``ld_extra`` > 0 gives
the device observations a row stride that much larger than ``round4(obs_dim)``,
with NaN in the padding columns (a kernel that reads them cannot pass).

The Gram kernel takes slabs of 2048 rows (``LB_SLAB_ROWS``): three cases sit at
2047 / 2048 / 2049 rows, and ``long_episode`` spans three slabs with ONE episode.

``spread``: how far the twin's own predictions move when the rows are permuted
before the fit (max over three permutations, absolute; measured on the build
machine and recorded here -- ``test_linear_baseline_cpu.py`` recomputes them and
holds every case to 1e-8).  The predictions' magnitudes are about 100.
A single episode of 4500 steps with returns that grow with its length moved by
1.3e-8 and was replaced by returns whose ramp is bounded.
"""
import numpy as np

SLAB = 2048

CASES = [
    # name, obs_dim, episode lengths, ld_extra               spread    max |v|
    ('smallest', 1, [1], 0),                               # 0         9.9e1
    ('single_steps', 1, [1, 1, 2], 0),                     # 8.5e-14   1.3e2
    ('stride4', 3, [5, 1, 40, 17], 8),                     # 8.8e-12   9.8e1
    ('equal_then_ragged', 17, 8 * [40] + [13, 1, 27], 0),  # 1.8e-10   1.1e2
    ('exact_tiles', 30, [90, 61, 120], 0),                 # 1.9e-11   1.3e2
    ('tile_edge', 31, [64, 65, 63, 1, 200], 0),            # 2.6e-11   1.3e2
    ('many_chunks', 4, [1000, 3], 0),                      # 1.9e-11   1.0e2
    ('long_episode', 4, [4500, 3], 0),                     # 9.4e-10   1.1e2
    ('limit', 128, 12 * [100] + [37], 0),                  # 2.0e-11   1.5e2
    ('slab_minus', 2, [700, 647, 700], 0),                 # 4.1e-12   1.0e2
    ('slab_exact', 2, [700, 648, 700], 0),                 # 7.6e-12   9.8e1
    ('slab_plus', 2, [700, 649, 700], 0),                  # 7.4e-12   1.0e2
]
# the spread column, for the tests that derive a bound from it
SPREAD = {
    'smallest': 0.0, 'single_steps': 8.5e-14, 'stride4': 8.8e-12,
    'equal_then_ragged': 1.8e-10, 'exact_tiles': 1.9e-11, 'tile_edge': 2.6e-11,
    'many_chunks': 1.9e-11, 'long_episode': 9.4e-10, 'limit': 2.0e-11,
    'slab_minus': 4.1e-12, 'slab_exact': 7.6e-12, 'slab_plus': 7.4e-12,
}
CASE_NAMES = [c[0] for c in CASES]
REG_COEFF = 1e-5


def case(name):
    return CASES[CASE_NAMES.index(name)]


def round4(n):
    return (n + 3) // 4 * 4


def make_inputs(name):
    """``(obs fp32 [S, obs_dim], returns fp32 [S], lengths)`` of a case: observations
    uniform in [-3, 3], 2 % of the entries times 5 (so the clip acts), a few exactly
    +-10; returns ~ N(0, 30) plus a ramp that falls from 100 to 0 over the episode."""
    _, obs_dim, lengths, _ = case(name)
    rng = np.random.RandomState(1000 + CASE_NAMES.index(name))
    S = int(sum(lengths))
    obs = rng.uniform(-3.0, 3.0, size=(S, obs_dim))
    obs[rng.uniform(size=obs.shape) < 0.02] *= 5.0
    flat = obs.reshape(-1)
    n_ten = min(4, flat.size // 2)
    where = rng.choice(flat.size, size=n_ten, replace=False)
    flat[where] = np.where(np.arange(n_ten) % 2 == 0, 10.0, -10.0)
    ramp = np.concatenate([100.0 * np.arange(n, 0, -1) / n for n in lengths])
    returns = 30.0 * rng.standard_normal(S) + ramp
    return obs.astype(np.float32), returns.astype(np.float32), list(lengths)


def paths_of(obs, returns, lengths, dtype=np.float64):
    """The reference's ``paths``: one dict per episode."""
    paths, at = [], 0
    for n in lengths:
        paths.append({'observations': obs[at:at + n].astype(dtype),
                      'returns': returns[at:at + n].astype(dtype)})
        at += n
    return paths


def golden_feature_rows(S, F, budget=8000):
    """The rows whose features the golden file stores: all of them while S * F fits
    the budget, else every k-th and the last three."""
    k = max(1, -(-S * F // budget))
    return np.unique(np.concatenate([np.arange(0, S, k),
                                     np.arange(max(0, S - 3), S)]))


# ---- the twin: the reference's arithmetic, restated in numpy fp64 ------------------
def features(obs, lengths):
    """``[S, 2 * obs_dim + 4]`` float64 feature rows of a batch."""
    x = np.clip(np.asarray(obs, dtype=np.float64), -10, 10)
    al = np.concatenate([np.arange(n) for n in lengths]).reshape(-1, 1) / 100.0
    return np.concatenate([x, x**2, al, al**2, al**3, np.ones_like(al)], axis=1)


def solve(gram, rhs, reg_coeff=REG_COEFF):
    """The ridge solve, regularisation times 10 while the result holds a NaN."""
    coeffs = None
    for _ in range(5):
        coeffs = np.linalg.lstsq(gram + reg_coeff * np.identity(gram.shape[0]),
                                 rhs, rcond=-1)[0]
        if not np.any(np.isnan(coeffs)):
            break
        reg_coeff *= 10
    return coeffs


def fit(phi, returns, reg_coeff=REG_COEFF):
    r = np.asarray(returns, dtype=np.float64)
    return solve(phi.T.dot(phi), phi.T.dot(r), reg_coeff)


def permutation_spread(phi, returns, n_perms=3, seed=5, eval_phi=None):
    """max |Phi' c(perm) - Phi' c| over ``n_perms`` row orders of the fit on
    ``phi``; ``Phi'`` is ``eval_phi`` (another batch's features) or ``phi``."""
    at = phi if eval_phi is None else eval_phi
    base = at.dot(fit(phi, returns))
    rng = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(n_perms):
        p = rng.permutation(phi.shape[0])
        moved = at.dot(fit(phi[p], np.asarray(returns)[p]))
        worst = max(worst, float(np.max(np.abs(moved - base))))
    return worst


def gae(rewards, values, lengths, discount, gae_lambda):
    """``(advantages, returns)`` in fp64 with a zero appended to every episode's
    baselines, as garage's numpy path does for a LinearFeatureBaseline.  The
    advantages' two constants are rounded to fp32 first, as ``ga_gae_scan_f32``
    takes them (the torch reference computes advantages in fp32); the returns use
    the float64 discount (``discount_cumsum``)."""
    adv = np.zeros(len(rewards))
    ret = np.zeros(len(rewards))
    gamma_ret = discount
    discount, c = float(np.float32(discount)), float(
        np.float32(discount * gae_lambda))
    at = 0
    for n in lengths:
        r = np.asarray(rewards[at:at + n], dtype=np.float64)
        v = np.append(np.asarray(values[at:at + n], dtype=np.float64), 0.0)
        a = g = 0.0
        for t in range(n - 1, -1, -1):
            delta = r[t] + discount * v[t + 1] - v[t]
            a = delta + c * a
            g = r[t] + gamma_ret * g
            adv[at + t], ret[at + t] = a, g
        at += n
    return adv, ret
