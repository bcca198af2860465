"""Host twin of the stretch between the rollout step and the packed batch: the
per-step record, the episode order, the flat cells of the packed samples and the
keyed id permutation.  Numpy only -- no torch, no GPU.

Written from the statements of ``include/garage_amd.h``, DESIGN.md and the comments
above the kernels, in whole-array numpy: the episode order is a SORT by (column, env)
where the device ranks with ballots and a running base, a step's record is a handful
of masked assignments where the device runs one thread per env, the permutation walks
its cycles with a masked loop over the still-out-of-range entries where the device
loops per element.  ``test_episode_pack_ref_cpu.py`` holds it to a brute-force double
loop and to the batches the real samplers produced (``tests/golden``).

Layouts (env-major, as the rollout buffers): ``rew`` / ``st`` / ``tail`` are
``[n, Tcap]``, ``lastobs`` is ``[n, Tcap, ldo]``; ``tail[i, t]`` is the length of the
episode of env ``i`` whose last step is column ``t``, else 0.
"""
import numpy as np

FIRST, MID, TERMINAL, TIMEOUT = 0, 1, 2, 3


# ---- one step's record ------------------------------------------------------------
def record_step(state, reward, step_type, next_obs, col, max_episode_length,
                terminal_only):
    """One vectorised step into column ``col``.

    ``state``: dict of ``rew``, ``st``, ``tail``, ``lastobs``, ``done``, ``ep_t``
    (not modified).  ``next_obs`` is ``[n, obs_dim]``: the entries a terminal
    observation has; ``lastobs`` rows may be wider, their padding is not written.
    Returns ``(new state, episodes that ended in the column, their total length)``.

    An env's episode grows by the step; it ends when it has reached
    ``max_episode_length`` or its step is a last one -- TERMINAL or TIMEOUT for the
    VecWorker, TERMINAL alone for the FragmentWorker (``terminal_only``).  Reward and
    step type are recorded for every env; the length and the terminal observation
    only where the episode ended, where the env is also marked for reset and its
    step count starts over.
    """
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    step_type = np.asarray(step_type)
    length = state['ep_t'].astype(np.int64) + 1
    last = (step_type == TERMINAL) if terminal_only else np.isin(
        step_type, (TERMINAL, TIMEOUT))
    ended = (length >= int(max_episode_length)) | last
    out['rew'][:, col] = reward
    out['st'][:, col] = step_type
    out['tail'][:, col] = np.where(ended, length, 0)
    obs_dim = np.asarray(next_obs).shape[1]
    out['lastobs'][ended, col, :obs_dim] = np.asarray(next_obs)[ended]
    out['done'][:] = ended
    out['ep_t'][:] = np.where(ended, 0, length)
    return out, int(ended.sum()), int(length[ended].sum())


# ---- episode order ----------------------------------------------------------------
def pack_order(tail):
    """``(ep_env, ep_end, ep_len)`` of the episodes that end inside ``tail``
    (``[n, columns]``), sorted by (column, env): the batch order of
    ``EpisodeBatch.concatenate`` over the worker's completion order."""
    tail = np.asarray(tail)
    env, end = np.nonzero(tail)
    order = np.lexsort((env, end))  # last key is the primary one
    env, end = env[order], end[order]
    return (env.astype(np.int64), end.astype(np.int64),
            tail[env, end].astype(np.int64))


def column_counts(tail):
    """Episodes that end in each column, and ``ep_base``: the episodes before it."""
    counts = (np.asarray(tail) != 0).sum(axis=0).astype(np.int64)
    return counts, np.cumsum(counts) - counts


def src_index(ep_env, ep_end, ep_len, Tcap):
    """``(off, cells)``: episode ``e`` owns the packed samples ``[off[e], off[e+1])``;
    sample ``j`` of it lies in the cell ``env * Tcap + column`` of the column ``j``
    steps after the episode's (or fragment's) first, its last being ``ep_end``."""
    ep_env, ep_end, ep_len = (np.asarray(a, dtype=np.int64)
                              for a in (ep_env, ep_end, ep_len))
    off = np.concatenate([[0], np.cumsum(ep_len)]).astype(np.int64)
    first_col = ep_end - (ep_len - 1)
    within = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], ep_len)
    cells = np.repeat(ep_env * int(Tcap) + first_col, ep_len) + within
    return off, cells


def packed_batch(bufs, n_steps, Tcap, first_step=0):
    """The batch a worker packs from the columns ``[first_step, n_steps)`` of its
    buffers ``bufs`` (``obs``, ``lastobs``, ``rew``, ``st``, ``tail``)."""
    env, end, length = pack_order(bufs['tail'][:, first_step:n_steps])
    end = end + first_step
    off, cells = src_index(env, end, length, Tcap)
    flat = lambda a: a.reshape((-1, ) + a.shape[2:])
    return dict(ep_env=env, ep_end=end, lengths=length, off=off, cells=cells,
                obs=flat(bufs['obs'])[cells], rew=flat(bufs['rew'])[cells],
                st=flat(bufs['st'])[cells],
                last_obs=flat(bufs['lastobs'])[env * int(Tcap) + end])


# ---- keyed permutation of [0, n) ----------------------------------------------------
_M32 = 0xFFFFFFFF


def _mix(x, k):
    """The round function: xor the round key in, then three multiply / xor-shift
    steps (uint32 arrays wrap)."""
    x = x ^ np.uint32(k)
    x = x * np.uint32(0x9E3779B1)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x85EBCA77)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE3D)
    x = x ^ (x >> np.uint32(16))
    return x


def half_bits_of(n):
    """The smallest ``h >= 1`` with ``4^h >= n``."""
    h = 1
    while 4**h < n:
        h += 1
    return h


def feistel_permutation(n, key, rounds=4):
    """``out[i]`` = the balanced Feistel network over ``2 h`` bits applied to ``i``
    until the value falls below ``n`` (cycle walking).  ``key`` is 64 bits: ``k0`` its
    low word, ``k1`` its high one; round ``r`` is keyed with
    ``k0 + 0x9E3779B9 r + (k1 ^ r)`` mod 2^32."""
    n, key = int(n), int(key)
    k0, k1 = key & _M32, (key >> 32) & _M32
    h = np.uint32(half_bits_of(n))
    mask = np.uint32((1 << int(h)) - 1)
    keys = [(k0 + 0x9E3779B9 * r + (k1 ^ r)) & _M32 for r in range(rounds)]

    def network(x):
        left, right = x >> h, x & mask
        for k in keys:
            left, right = right, left ^ (_mix(right, k) & mask)
        return (left << h) | right

    x = network(np.arange(n, dtype=np.uint32))
    while True:
        outside = np.nonzero(x >= np.uint32(n))[0]
        if outside.size == 0:
            return x.astype(np.int64)
        x[outside] = network(x[outside])
