"""Host twin of a population's joint pack index (``ga_member_pack_index``) and of
the progress check it starts from (``ga_member_progress``).  Numpy only.

Written from the statements of ``include/garage_amd.h``: a member's episodes are the
non-zero cells of its rows of ``tail`` in the columns below ``c_m``, read off the
TRANSPOSED block in row-major order -- which is (end column, env index) -- where the
device gives a thread to every column and counts ranks from ``col_base``; offsets are
cumulative sums where the device scans; a row's cell comes from ``np.repeat`` over
the episodes where the device bisects the offsets.

``tail`` is ``[n, Tcap]``: an episode's length at its last cell, else 0; member ``m``
owns the rows ``[m g, (m + 1) g)``.
"""
import numpy as np


def round16(x):
    return -(-np.asarray(x, dtype=np.int64) // 16) * 16


def member_progress(tail, n_members, n_cols, num_samples):
    """``(progress [M, 3], col_base [M, Tcap])`` as the header states them:
    ``c_m`` (0: the target is not reached within ``n_cols``), the episodes that
    ended below ``c_m`` (below ``n_cols`` while ``c_m == 0``), the steps of all
    episodes completed below ``n_cols``; per column the member's episodes that ended
    before it."""
    tail = np.asarray(tail).astype(np.int64)
    n, tcap = tail.shape
    g = n // n_members
    progress = np.zeros((n_members, 3), dtype=np.int32)
    col_base = np.zeros((n_members, tcap), dtype=np.int32)
    for m in range(n_members):
        block = tail[m * g:(m + 1) * g, :n_cols]
        steps, ended = block.sum(axis=0), (block != 0).sum(axis=0)
        done = np.cumsum(steps)
        reached = np.nonzero(done >= num_samples)[0]
        c = int(reached[0]) + 1 if reached.size else 0
        progress[m] = (c, ended[:c].sum() if c else ended.sum(), done[-1])
        col_base[m, :n_cols] = np.cumsum(ended) - ended
    return progress, col_base


def pack_index(tail, n_members, progress, max_samples=None):
    """Everything ``ga_member_pack_index`` writes, plus ``episode_start``
    (``[M + 1]``: the episodes of the members before ``m``).  ``max_samples``
    defaults to the bound the header gives: the sum of ``g c_m`` rounded up to 16."""
    tail = np.asarray(tail).astype(np.int64)
    n, tcap = tail.shape
    g = n // n_members
    c = np.asarray(progress)[:, 0].astype(np.int64)
    if max_samples is None:
        max_samples = int(round16(g * c).sum())
    env, end, length, off, samples = [], [], [], [], []
    for m in range(n_members):
        block = tail[m * g:(m + 1) * g, :c[m]]
        t, i = np.nonzero(block.T)  # row-major over (column, env)
        L = block[i, t]
        env.append(i + m * g)
        end.append(t)
        length.append(L)
        off.append(np.concatenate([[0], np.cumsum(L)]))
        samples.append(int(L.sum()))
    samples = np.asarray(samples, dtype=np.int64)
    member_off = np.concatenate([[0], np.cumsum(round16(samples))])
    src = np.full(max_samples, -1, dtype=np.int64)
    for m in range(n_members):
        L = length[m]
        first = env[m] * tcap + end[m] - (L - 1)
        within = np.arange(samples[m]) - np.repeat(off[m][:-1], L)
        lo = member_off[m]
        src[lo:lo + samples[m]] = np.repeat(first, L) + within
    counts = np.asarray([len(e) for e in env], dtype=np.int64)
    return dict(
        ep_env=np.concatenate(env), ep_end=np.concatenate(end),
        ep_len=np.concatenate(length), ep_off=np.concatenate(off),
        member_samples=samples, member_off=member_off, src=src,
        episode_start=np.concatenate([[0], np.cumsum(counts)]))


def random_tail(rng, n, tcap, max_len, min_len=1):
    """A ``tail`` buffer as a rollout leaves it: every env runs episodes of
    ``min_len..max_len`` steps back to back; the one in flight at ``tcap`` leaves no
    mark."""
    tail = np.zeros((n, tcap), dtype=np.uint16)
    for i in range(n):
        t = 0
        while True:
            L = int(rng.integers(min_len, max_len + 1))
            t += L
            if t > tcap:
                break
            tail[i, t - 1] = L
    return tail


def cases():
    """``{name: (tail, n_members, n_cols, num_samples)}``: the shapes both test files
    run -- one env per member, one member, members that reach the target in different
    columns, episodes of one step only, an episode as long as the buffer, a member
    that never reaches the target (``c_m == 0``), more than 256 columns (the index
    walks the columns 256 at a time) and more episodes in a member than a bisection
    of a few steps covers."""
    rng = np.random.default_rng(11)
    out = {}
    out['g=1'] = (random_tail(rng, 5, 24, 6), 5, 24, 9)
    out['M=1'] = (random_tail(rng, 7, 20, 5), 1, 20, 40)
    # short episodes in member 0, long ones in member 2: c_m differs
    tail = np.concatenate([random_tail(rng, 16, 40, 3),
                           random_tail(rng, 16, 40, 9, 4),
                           random_tail(rng, 16, 40, 17, 12)])
    out['different-c'] = (tail, 3, 40, 100)
    out['length-1'] = (random_tail(rng, 12, 16, 1), 3, 16, 30)
    tail = random_tail(rng, 6, 12, 4)
    tail[1] = 0
    tail[1, 11] = 12  # env 1 runs one episode over the whole buffer
    tail[4] = 0
    tail[4, 11] = 12
    out['length-Tcap'] = (tail, 2, 12, 30)
    tail = random_tail(rng, 12, 16, 4)
    tail[4:8] = 0  # member 1 completes nothing
    out['c=0'] = (tail, 3, 16, 20)
    out['300-columns'] = (random_tail(rng, 4, 300, 40, 20), 2, 300, 500)
    out['many-episodes'] = (random_tail(rng, 64, 48, 2), 2, 48, 1400)
    return out
