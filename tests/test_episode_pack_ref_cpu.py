"""``tests/_episode_pack_ref.py`` held to things it was not written from: a brute-force
double loop over (column, env), the batches the real ``VecWorker`` produced
(``tests/golden/sampler.npz``, ``point_sampler.npz``) and the defining properties of a
keyed permutation.  Also the two refusals of oversized or too-narrow buffers, which
need no GPU: the checks come before any launch.

Seeded mutations of the twin (``test_seeded_mutations_are_noticed``) show that each
comparison the GPU file makes would notice the mistake it is there for."""
import ctypes as C

import numpy as np
import pytest

import _episode_pack_ref as ref

PERM_SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1025, 4097, 65537)
KEY_A, KEY_B = 0x0123456789ABCDEF, 0xFEDCBA9876543210


# ---- brute force -------------------------------------------------------------------
def _brute_order(tail):
    env, end, length = [], [], []
    for t in range(tail.shape[1]):
        for i in range(tail.shape[0]):
            if tail[i, t]:
                env.append(i)
                end.append(t)
                length.append(int(tail[i, t]))
    return env, end, length


def _brute_cells(env, end, length, Tcap):
    off, cells = [0], []
    for e in range(len(env)):
        for j in range(length[e]):
            cells.append(env[e] * Tcap + end[e] - length[e] + 1 + j)
        off.append(len(cells))
    return off, cells


def _random_tail(rng, n, cols, density):
    """Episode ends at random cells, every length consistent with the columns behind
    it (an episode of env i starts after the env's previous one ended)."""
    tail = np.zeros((n, cols), dtype=np.uint16)
    for i in range(n):
        start = 0
        for t in range(cols):
            if rng.rand() < density:
                # (an episode may have begun before column 0: any length >= its part)
                tail[i, t] = t - start + 1 + (rng.randint(0, 4) if start == 0 else 0)
                start = t + 1
    return tail


@pytest.mark.parametrize('n,cols,density', [(1, 1, 1.0), (1, 9, 0.4), (7, 5, 0.0),
                                            (13, 11, 0.3), (300, 6, 0.5),
                                            (40, 17, 1.0)])
def test_order_and_cells_equal_the_double_loop(n, cols, density):
    rng = np.random.RandomState(n * 100 + cols)
    tail = _random_tail(rng, n, cols, density)
    env, end, length = ref.pack_order(tail)
    b_env, b_end, b_len = _brute_order(tail)
    assert env.tolist() == b_env and end.tolist() == b_end
    assert length.tolist() == b_len
    counts, base = ref.column_counts(tail)
    assert counts.tolist() == [b_end.count(t) for t in range(cols)]
    assert base.tolist() == [sum(e < t for e in b_end) for t in range(cols)]
    # the cells of whole episodes only (a length may reach back before column 0)
    keep = [e for e in range(len(b_env)) if b_len[e] <= b_end[e] + 1]
    sub = [[x[e] for e in keep] for x in (b_env, b_end, b_len)]
    Tcap = cols + 3
    off, cells = ref.src_index(sub[0], sub[1], sub[2], Tcap)
    b_off, b_cells = _brute_cells(sub[0], sub[1], sub[2], Tcap)
    assert off.tolist() == b_off and cells.tolist() == b_cells


def test_fragment_cells_equal_the_double_loop():
    """A fragment is shorter than the episode it belongs to: ``ep_len`` counts back
    from ``ep_end`` whatever the tail said."""
    env, end, length = [3, 0, 3, 2], [4, 9, 9, 0], [2, 10, 5, 1]
    off, cells = ref.src_index(env, end, length, 10)
    b_off, b_cells = _brute_cells(env, end, length, 10)
    assert off.tolist() == b_off and cells.tolist() == b_cells
    assert cells[0] == 33 and cells[2] == 0 and cells[-1] == 20


# ---- the real samplers' batches ----------------------------------------------------
def _tail_of(env_lengths, cols):
    """Tail matrix of envs that each run the given episodes back to back from column
    0 (an episode that would not end inside ``cols`` leaves no mark)."""
    n = len(env_lengths)
    tail = np.zeros((n, cols), dtype=np.uint16)
    for i, lens in enumerate(env_lengths):
        t = 0
        for L in lens:
            if t + L > cols:
                break
            tail[i, t + L - 1] = L
            t += L
    return tail


def _first_column_with(tail, num_samples):
    done = np.cumsum(tail.astype(np.int64).sum(axis=0))
    return int(np.argmax(done >= num_samples)) + 1


def test_counting_env_batches_of_the_real_vecworker(golden):
    """``sampler.npz``: the tail matrix follows from the fixture's ``cycles`` alone
    (episode ``e`` of env ``i`` lasts ``cycles[i][e % 3]`` steps, reward = step index,
    observation = (env, episode, t)); the twin's order must be the real worker's.
    Usable: ``vec_`` / ``vec2_`` lengths, rewards and the (env, episode, t) of the last
    observations.  Not usable: ``def_`` (one worker per env: worker order, nothing is
    packed by completion step) and ``frag*`` (fragment order is host logic)."""
    g = golden('sampler')
    P, n = [int(v) for v in g['cfg']]
    cyc = g['cycles']
    episode0 = np.zeros(n, dtype=np.int64)
    for prefix, num in (('vec_', 30), ('vec2_', 17)):
        cols = num + P
        env_lengths = [[min(int(cyc[i][(episode0[i] + k) % cyc.shape[1]]), P)
                        for k in range(cols)] for i in range(n)]
        tail = _tail_of(env_lengths, cols)
        n_steps = _first_column_with(tail, num)
        tail = tail[:, :n_steps]
        env, end, length = ref.pack_order(tail)
        assert length.tolist() == g[prefix + 'lengths'].tolist()
        last = g[prefix + 'last_observations']
        assert env.tolist() == last[:, 0].astype(int).tolist()
        assert length.tolist() == last[:, 2].astype(int).tolist()
        # which episode of its env each one is
        nth = [int((env[:e] == env[e]).sum()) for e in range(len(env))]
        assert (episode0[env] + nth).tolist() == last[:, 1].astype(int).tolist()
        # rewards through the cells: cell (i, t) holds the step index in its episode
        rew = np.full((n, n_steps), -1.0)
        for i in range(n):
            t = 0
            for L in env_lengths[i]:
                if t + L > n_steps:
                    break
                rew[i, t:t + L] = np.arange(L)
                t += L
        off, cells = ref.src_index(env, end, length, n_steps)
        assert np.array_equal(rew.reshape(-1)[cells], g[prefix + 'rewards'])
        assert off[-1] == len(g[prefix + 'rewards'])
        # the next call: envs with an episode in flight start a new one
        finished = np.asarray([(env == i).sum() for i in range(n)])
        steps = np.asarray([length[env == i].sum() for i in range(n)])
        episode0 = episode0 + finished + (steps < n_steps)


def test_point_env_batches_of_the_real_vecworker(golden):
    """``point_sampler.npz``: every episode names its env through its goal, and both
    calls start every env at column 0, so the fixture's own lengths give the tail
    matrix; the order the twin sorts it into must be the fixture's.  Usable: ``a_`` /
    ``b_`` lengths, goals and rewards."""
    g = golden('point_sampler')
    P, n = [int(v) for v in g['cfg']]
    goals = g['goals']
    for prefix in ('a_', 'b_'):
        lengths = g[prefix + 'lengths'].astype(np.int64)
        ep_env = np.asarray([int(np.nonzero((goals == row).all(axis=1))[0][0])
                             for row in g[prefix + 'goal']])
        assert len(set(map(tuple, goals))) == n  # goals name the envs
        cols = int(max(lengths[ep_env == i].sum() for i in range(n)))
        tail = _tail_of([lengths[ep_env == i] for i in range(n)], cols)
        # rewards of env i in time order = those of its episodes, in batch order
        off_fix = np.concatenate([[0], np.cumsum(lengths)])
        rew = np.full((n, cols), np.nan)
        for i in range(n):
            mine = np.concatenate([g[prefix + 'rewards'][off_fix[e]:off_fix[e + 1]]
                                   for e in np.nonzero(ep_env == i)[0]])
            rew[i, :len(mine)] = mine
        env, end, length = ref.pack_order(tail)
        assert env.tolist() == ep_env.tolist()
        assert length.tolist() == lengths.tolist()
        off, cells = ref.src_index(env, end, length, cols)
        assert off.tolist() == off_fix.tolist()
        assert np.array_equal(rew.reshape(-1)[cells], g[prefix + 'rewards'])


# ---- the record of a step ----------------------------------------------------------
def _blank_state(n, Tcap, ldo, ep_t):
    return dict(rew=np.full((n, Tcap), -5.0, np.float32),
                st=np.full((n, Tcap), 9, np.uint8),
                tail=np.full((n, Tcap), 7, np.uint16),
                lastobs=np.full((n, Tcap, ldo), -3.0, np.float32),
                done=np.full(n, 5, np.uint8), ep_t=np.asarray(ep_t, np.int32))


@pytest.mark.parametrize('terminal_only', [0, 1])
def test_record_step_is_the_workers_loop(terminal_only):
    """Against the per-env loop of the worker (``vec_worker.py:185-201``,
    ``fragment_worker.py:104-116``), written as a loop."""
    P, Tcap, col = 4, 3, 1
    cases = [(ep_t, st) for ep_t in (0, 1, 2, 3) for st in (0, 1, 2, 3)]
    n = len(cases)
    state = _blank_state(n, Tcap, 4, [c[0] for c in cases])
    reward = np.arange(n, dtype=np.float32)
    step_type = np.asarray([c[1] for c in cases], np.uint8)
    next_obs = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    new, eps, samples = ref.record_step(state, reward, step_type, next_obs, col, P,
                                        terminal_only)
    want_eps = want_samples = 0
    for i, (ep_t, st) in enumerate(cases):
        length = ep_t + 1
        last = st == 2 if terminal_only else st in (2, 3)
        ended = length >= P or last
        assert new['rew'][i, col] == reward[i] and new['st'][i, col] == st
        assert new['tail'][i, col] == (length if ended else 0)
        assert new['done'][i] == ended
        assert new['ep_t'][i] == (0 if ended else length)
        want = list(next_obs[i]) + [-3.0] if ended else [-3.0] * 4
        assert new['lastobs'][i, col].tolist() == want
        want_eps += ended
        want_samples += length if ended else 0
    assert (eps, samples) == (want_eps, want_samples)
    for k in ('rew', 'st', 'tail', 'lastobs'):  # the other columns
        assert np.array_equal(np.delete(new[k], col, axis=1),
                              np.delete(state[k], col, axis=1)), k
    assert state['done'][0] == 5 and state['tail'][0, col] == 7  # input untouched


def test_record_step_reaches_the_longest_episode():
    state = _blank_state(2, 2, 1, [65534, 65533])
    new, eps, samples = ref.record_step(state, [0, 0], [1, 1], np.zeros((2, 1)), 0,
                                        65535, 0)
    assert new['tail'][:, 0].tolist() == [65535, 0] and (eps, samples) == (1, 65535)
    assert new['ep_t'].tolist() == [0, 65534]


# ---- the permutation ----------------------------------------------------------------
@pytest.mark.parametrize('n', PERM_SIZES)
def test_feistel_permutation_is_a_keyed_bijection(n):
    a = ref.feistel_permutation(n, KEY_A)
    assert np.array_equal(np.sort(a), np.arange(n))
    assert np.array_equal(a, ref.feistel_permutation(n, KEY_A))
    if n >= 64:
        assert not np.array_equal(a, np.arange(n))
        assert not np.array_equal(a, ref.feistel_permutation(n, KEY_B))
        # both key words matter
        assert not np.array_equal(a, ref.feistel_permutation(n, KEY_A ^ 1))
        assert not np.array_equal(a, ref.feistel_permutation(n, KEY_A ^ (1 << 32)))


def test_feistel_permutation_against_a_scalar_walk():
    """Python integers, one id at a time: the array arithmetic wraps where it should."""
    n, key = 1000, KEY_B
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    h = ref.half_bits_of(n)
    assert h == 5 and ref.half_bits_of(1024) == 5 and ref.half_bits_of(1025) == 6
    assert [ref.half_bits_of(v) for v in (1, 4, 5, 16, 17)] == [1, 1, 2, 2, 3]
    mask, M = (1 << h) - 1, 0xFFFFFFFF

    def mix(x, k):
        x ^= k
        for mul, sh in ((0x9E3779B1, 15), (0x85EBCA77, 13), (0xC2B2AE3D, 16)):
            x = (x * mul) & M
            x ^= x >> sh
        return x

    out = []
    for i in range(n):
        x = i
        while True:
            left, right = x >> h, x & mask
            for r in range(4):
                rk = (k0 + 0x9E3779B9 * r + (k1 ^ r)) & M
                left, right = right, left ^ (mix(right, rk) & mask)
            x = (left << h) | right
            if x < n:
                break
        out.append(x)
    assert ref.feistel_permutation(n, key).tolist() == out


def test_feistel_permutation_is_fast_enough_for_a_million_ids():
    n = 2**20 + 1
    a = ref.feistel_permutation(n, KEY_A)
    assert a.min() == 0 and a.max() == n - 1 and np.unique(a).size == n


# ---- a comparison with the twin notices a wrong twin ---------------------------------
def _mutant_order(tail, descending=False):
    env, end, length = ref.pack_order(tail)
    if descending:  # the envs of a column ranked from the top
        order = np.lexsort((-env, end))
        return env[order], end[order], length[order]
    return env, end, length


def test_seeded_mutations_are_noticed():
    """What the GPU file compares would differ under each mistake it is there for, at
    the shapes it uses (the mutations are of the twin; the kernels are not touched)."""
    rng = np.random.RandomState(3)
    n, cols = 600, 12
    tail = np.zeros((n, cols), np.uint16)
    tail[rng.rand(n, cols) < 0.3] = 5
    tail[:256, 4] = 0   # a column whose enders are all >= 256
    env, end, length = ref.pack_order(tail)
    # pack: descending rank within a column
    m_env = _mutant_order(tail, descending=True)[0]
    assert not np.array_equal(m_env, env)
    # pack: the carried base dropped -- the second pass of a column ranks from the
    # column's base again, so two episodes share a slot and one slot stays poison
    counts, base = ref.column_counts(tail)
    slot = np.empty(len(env), np.int64)
    for e in range(len(env)):
        in_pass = (end == end[e]) & (env // 256 == env[e] // 256) & (env < env[e])
        slot[e] = base[end[e]] + in_pass.sum()
    assert len(set(slot.tolist())) < len(env)
    # src index: end - len instead of end - len + 1
    off, cells = ref.src_index([2, 0], [9, 3], [4, 4], 10)
    assert not np.array_equal(cells, ref.src_index([2, 0], [8, 2], [4, 4], 10)[1])
    # record: TIMEOUT ending a fragment worker's episode; `>` for `>=` at the limit
    st = _blank_state(3, 2, 1, [0, 2, 1])
    args = ([0, 0, 0], [3, 1, 1], np.zeros((3, 1)), 0)
    a = ref.record_step(st, *args, 3, 1)
    assert a[0]['tail'][:, 0].tolist() == [0, 3, 0]
    assert ref.record_step(st, *args, 3, 0)[0]['tail'][:, 0].tolist() == [1, 3, 0]
    assert ref.record_step(st, *args, 4, 1)[0]['tail'][:, 0].tolist() == [0, 0, 0]
    # gathers: a source row one off, or the stride of the wrong side
    src = rng.randn(37, 12).astype(np.float32)
    idx = np.asarray([36, 0, 0, 36, 35])
    assert not np.array_equal(src[idx, :8], src[np.maximum(idx - 1, 0), :8])
    assert not np.array_equal(src[idx, :8],
                              src.reshape(-1)[idx[:, None] * 8 + np.arange(8)])
    # permutation: three rounds, the key's high word dropped
    for size in (257, 1025):
        a = ref.feistel_permutation(size, KEY_A)
        assert not np.array_equal(a, ref.feistel_permutation(size, KEY_A, rounds=3))
        assert not np.array_equal(
            a, ref.feistel_permutation(size, KEY_A & 0xFFFFFFFF))


# ---- the refusals (checked before any launch: no GPU) --------------------------------
def test_buffers_with_too_many_cells_are_refused():
    from garage_amd.sampler import check_cells_int32
    check_cells_int32(8192, 262140)          # 2^31 - 32768 cells
    check_cells_int32(1, 2**31 - 1)
    for n, tcap in ((8193, 262140), (1, 2**31), (65536, 32768), (2**20, 2048)):
        with pytest.raises(ValueError, match='rollout buffers too large'):
            check_cells_int32(n, tcap)


def test_alloc_buffers_checks_the_cells_before_it_allocates():
    """``_alloc_buffers`` (and ``_grown`` through it) with a worker that never saw a
    GPU: the refusal comes before the first tensor."""
    from garage_amd.sampler import GpuVecWorker
    w = GpuVecWorker.__new__(GpuVecWorker)
    w._n_envs, w._max_episode_length, w.env = 2**16, 1000, None
    with pytest.raises(ValueError, match='rollout buffers too large'):
        w._alloc_buffers(2**31)  # ceil(2^31 / 2^16) + 999 columns: 2^31 cells and more


def _host_args():
    buf = C.create_string_buffer(4096)
    return buf, C.addressof(buf)


def test_pack_src_index_refuses_what_int32_cannot_address():
    from garage_amd import _lib
    buf, addr = _host_args()
    for tcap in (0, -1, 2**31, 2**40):
        with pytest.raises(_lib.GarageAmdError, match='rollout buffers too large'):
            _lib.call('ga_pack_src_index', addr, addr, addr, addr, 1, tcap, addr, None)
    for n_eps in (0, 2**31):
        with pytest.raises(_lib.GarageAmdError, match='bad n_eps'):
            _lib.call('ga_pack_src_index', addr, addr, addr, addr, n_eps, 8, addr, None)


def test_record_step_refuses_rows_narrower_than_the_observation():
    from garage_amd import _lib
    buf, addr = _host_args()

    def record(**kw):
        rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5, reward=addr,
                              step_type=addr, next_obs=addr, ldo=4, obs_dim=3,
                              ep_t=addr, rew_buf=addr, st_buf=addr, tail_buf=addr,
                              lastobs_buf=addr, done=addr, step_eps=addr,
                              step_samples=addr)
        for k, v in kw.items():
            setattr(rec, k, v)
        _lib.call('ga_record_step', C.byref(rec), None)

    for kw in (dict(ldo=2), dict(ldo=0), dict(obs_dim=5), dict(obs_dim=-1)):
        with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
            record(**kw)
