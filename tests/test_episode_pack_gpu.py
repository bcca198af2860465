"""The stretch between the rollout step and the packed batch, entry by entry:
``ga_record_step``, ``ga_pack_episodes``, ``ga_pack_src_index``, the three gathers and
``ga_permutation_i32``, each called directly and held to ``tests/_episode_pack_ref.py``
EXACTLY -- everything here is integer or bit-copy work.

Every buffer an entry may write lies between two guard regions of poison bytes that
must survive the call; whole buffers are compared, so the cells, columns and padding an
entry must leave alone are part of every comparison.  Float payloads (NaN payloads and
-0.0 among them) are compared through their int32 views.
``test_episode_pack_ref_cpu.py`` holds the twin itself to a brute-force loop and to the
real samplers' batches."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _episode_pack_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 256        # bytes before and after every buffer (keeps 16-B alignment)
POISON = 0xA5      # every byte of a guard, and of what an entry has yet to write
PERM_SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1025, 4097, 65537,
              2**20 + 1)
KEYS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)


@pytest.fixture(scope='module')
def dev():
    from garage_amd.engine import require_gpu
    return require_gpu()


def _L():
    from garage_amd import _lib
    return _lib


def _stream():
    return _L().stream_ptr()


class Guarded:
    """A device buffer holding ``host`` (any dtype, any shape) between two guards."""

    def __init__(self, host, dev):
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, self.nbytes = host.shape, host.dtype, host.nbytes
        raw = np.full(2 * GUARD + self.nbytes, POISON, dtype=np.uint8)
        raw[GUARD:GUARD + self.nbytes] = host.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(raw).to(dev)
        assert self.t.data_ptr() % 16 == 0

    @classmethod
    def poisoned(cls, shape, dtype, dev):
        count = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return cls(np.full(count, POISON, np.uint8).view(dtype).reshape(shape), dev)

    def ptr(self, byte_offset=0):
        return C.c_void_p(self.t.data_ptr() + GUARD + byte_offset)

    def host(self):
        """The payload; the guards must be as they were."""
        raw = self.t.cpu().numpy()
        assert (raw[:GUARD] == POISON).all(), 'wrote before the buffer'
        assert (raw[GUARD + self.nbytes:] == POISON).all(), 'wrote past the buffer'
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape)


def _same(got, want, what=''):
    """Bit equality: same dtype, same shape, same bytes (floats through int32)."""
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert bad.size == 0, '{}: {} of {} differ, first at {}: {} != {}'.format(
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]],
        want.reshape(-1)[bad[0]])


def _poison_like(shape, dtype):
    count = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(count, POISON, np.uint8).view(dtype).reshape(shape).copy()


def _floats(rng, shape):
    """Random fp32 with the payloads a bit copy must keep: NaNs of two payloads,
    -0.0, infinities, a denormal."""
    x = rng.randn(*shape).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    special = np.asarray([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0xFF800000,
                          0x00000001, 0x7F812345], dtype=np.uint32)
    where = rng.randint(0, flat.size, size=max(1, flat.size // 9))
    flat[where] = special[rng.randint(0, special.size, size=where.size)]
    return x


# ---- ga_record_step ------------------------------------------------------------------
STATE_KEYS = ('rew', 'st', 'tail', 'lastobs', 'done', 'ep_t')


class Recorder:
    """Rollout buffers on the device and in the twin, stepped together."""

    def __init__(self, rng, n, Tcap, obs_dim, ldo, dev, zero_counts=False):
        self.n, self.Tcap, self.obs_dim, self.ldo, self.dev = n, Tcap, obs_dim, ldo, dev
        self.state = dict(rew=_floats(rng, (n, Tcap)),
                          st=rng.randint(0, 256, size=(n, Tcap)).astype(np.uint8),
                          tail=rng.randint(0, 65536, size=(n, Tcap)).astype(np.uint16),
                          lastobs=_poison_like((n, Tcap, ldo), np.float32),
                          done=rng.randint(0, 2, size=n).astype(np.uint8),
                          ep_t=np.zeros(n, np.int32))
        self.step_eps = rng.randint(1, 1000, size=Tcap).astype(np.int32)
        self.step_samples = rng.randint(1, 100000, size=Tcap).astype(np.int32)
        if zero_counts:
            self.step_eps[:], self.step_samples[:] = 0, 0
        self.d = {k: Guarded(v, dev) for k, v in self.state.items()}
        self.d_eps = Guarded(self.step_eps, dev)
        self.d_samples = Guarded(self.step_samples, dev)

    def set_ep_t(self, ep_t):
        self.state['ep_t'] = np.asarray(ep_t, np.int32)
        self.d['ep_t'] = Guarded(self.state['ep_t'], self.dev)

    def args(self, reward, step_type, next_obs, col, P, terminal_only):
        r = _L().RecordArgs()
        r.n, r.col, r.Tcap, r.max_episode_length = self.n, col, self.Tcap, P
        r.reward, r.step_type = reward.ptr().value, step_type.ptr().value
        r.next_obs, r.ldo, r.obs_dim = next_obs.ptr().value, self.ldo, self.obs_dim
        r.ep_t = self.d['ep_t'].ptr().value
        r.rew_buf, r.st_buf = self.d['rew'].ptr().value, self.d['st'].ptr().value
        r.tail_buf = self.d['tail'].ptr().value
        r.lastobs_buf = self.d['lastobs'].ptr().value
        r.done = self.d['done'].ptr().value
        r.step_eps, r.step_samples = self.d_eps.ptr().value, self.d_samples.ptr().value
        r.terminal_only = terminal_only
        return r

    def step(self, reward, step_type, next_obs, col, P, terminal_only):
        """One ``ga_record_step`` and one twin step; everything must agree.
        ``next_obs``: ``[n, ldo]``, the padding columns are poison the entry must not
        copy."""
        ins = [Guarded(np.asarray(reward, np.float32), self.dev),
               Guarded(np.asarray(step_type, np.uint8), self.dev),
               Guarded(np.asarray(next_obs, np.float32), self.dev)]
        r = self.args(*ins, col, P, terminal_only)
        _L().call('ga_record_step', C.byref(r), _stream())
        torch.cuda.synchronize()
        self.state, eps, samples = ref.record_step(
            self.state, reward, step_type, next_obs[:, :self.obs_dim], col, P,
            terminal_only)
        self.step_eps[col] += eps
        self.step_samples[col] += samples
        self.check('col {} P {} terminal_only {}'.format(col, P, terminal_only))
        for g, want in zip(ins, (reward, step_type, next_obs)):
            _same(g.host(), np.asarray(want, g.dtype), 'an input changed')
        return eps, samples

    def check(self, what):
        for k in STATE_KEYS:
            _same(self.d[k].host(), self.state[k], '{} ({})'.format(k, what))
        _same(self.d_eps.host(), self.step_eps, 'step_eps ({})'.format(what))
        _same(self.d_samples.host(), self.step_samples, 'step_samples ({})'.format(what))


def _next_obs(rng, n, obs_dim, ldo):
    """``[n, ldo]``; the padding columns hold bytes of their own, which are not the
    poison of ``lastobs``: a copy of the whole row would show."""
    x = np.full(n * ldo * 4, 0x3C, np.uint8).view(np.float32).reshape(n, ldo).copy()
    x[:, :obs_dim] = _floats(rng, (n, obs_dim))
    return x


def _wave_step(rng, n, P, terminal_only, shift):
    """Step types and step counts by wave of 64 envs, in turn: nothing ends in the
    wave; only lane 63 ends; every lane ends.  Enders end by TERMINAL, by TIMEOUT
    (where that is a last step) or by reaching P with any step type."""
    st = np.zeros(n, np.uint8)
    ep_t = np.zeros(n, np.int32)
    quiet = [0, 1, 3] if terminal_only else [0, 1]
    for i in range(n):
        kind = (i // 64 + shift) % 3
        ends = kind == 2 or (kind == 1 and i % 64 == 63)
        if not ends:
            st[i], ep_t[i] = rng.choice(quiet), rng.randint(0, P - 1)
        else:
            how = rng.randint(0, 3)
            if how == 0:
                st[i], ep_t[i] = 2, rng.randint(0, P)
            elif how == 1 and not terminal_only:
                st[i], ep_t[i] = 3, rng.randint(0, P)
            else:
                st[i], ep_t[i] = rng.randint(0, 4), P - 1
    return st, ep_t


@pytest.mark.parametrize('terminal_only', [0, 1])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 513])
def test_record_step(n, terminal_only, dev):
    rng = np.random.RandomState(1000 * terminal_only + n)
    Tcap, obs_dim, ldo = 5, 3, 8
    rec = Recorder(rng, n, Tcap, obs_dim, ldo, dev)
    seen = set()
    # whole waves without an ender / one ender in lane 63 / every lane ending
    for shift, col in ((0, 0), (1, Tcap - 1), (2, 2)):
        P = 100
        st, ep_t = _wave_step(rng, n, P, terminal_only, shift)
        rec.set_ep_t(ep_t)
        rec.step(_floats(rng, (n, )), st, _next_obs(rng, n, obs_dim, ldo), col, P,
                 terminal_only)
        waves = [rec.state['done'][w:w + 64] for w in range(0, n, 64)]
        seen |= {'none' if not w.any() else 'all' if w.all() else
                 'lane63' if w.sum() == 1 and len(w) == 64 and w[63] else 'mixed'
                 for w in waves}
    assert {'none', 'all'} <= seen and ('lane63' in seen) == (n >= 64)
    assert 'mixed' not in seen
    # at the limit, one short of it, MID at the limit; every step type
    P = 7
    rec.set_ep_t(rng.choice([P - 1, P - 2, 0, 3], size=n))
    st = rng.randint(0, 4, size=n).astype(np.uint8)
    st[:min(n, 3)] = 1
    rec.state['ep_t'][:min(n, 3)] = [P - 1, P - 2, 0][:min(n, 3)]
    rec.set_ep_t(rec.state['ep_t'])
    rec.step(_floats(rng, (n, )), st, _next_obs(rng, n, obs_dim, ldo), 1, P,
             terminal_only)
    assert rec.state['tail'][0, 1] == P and (n < 2 or rec.state['tail'][1, 1] == 0)
    # max_episode_length = 1: every step ends an episode of length 1
    rec.set_ep_t(np.zeros(n, np.int32))
    eps, samples = rec.step(_floats(rng, (n, )), rng.randint(0, 4, size=n),
                            _next_obs(rng, n, obs_dim, ldo), 3, 1, terminal_only)
    assert (eps, samples) == (n, n)
    # the longest episode there is: 65534 steps behind it, limit 65535
    rec.set_ep_t(np.resize([65534, 65533, 65534, 0], n))
    rec.step(_floats(rng, (n, )), np.ones(n, np.uint8),
             _next_obs(rng, n, obs_dim, ldo), Tcap - 1, 65535, terminal_only)
    assert rec.state['tail'][0, Tcap - 1] == 65535
    assert (rec.d['tail'].host()[::4, Tcap - 1] == 65535).all()


@pytest.mark.parametrize('terminal_only', [0, 1])
def test_record_step_carries_an_episode_over_columns(terminal_only, dev):
    """Consecutive columns: the step count and the reset mark of one call are what
    the next one starts from."""
    rng = np.random.RandomState(77 + terminal_only)
    n, Tcap, obs_dim, ldo, P = 257, 4, 5, 8, 3
    rec = Recorder(rng, n, Tcap, obs_dim, ldo, dev)
    total = 0
    for col in range(Tcap):
        st = rng.choice([0, 1, 1, 1, 2, 3], size=n).astype(np.uint8)
        eps, _ = rec.step(_floats(rng, (n, )), st, _next_obs(rng, n, obs_dim, ldo),
                          col, P, terminal_only)
        total += eps
    tail = rec.state['tail']
    assert total > n and tail.max() == P and (tail == 2).any() and (tail == 1).any()


def test_record_step_refusals(dev):
    L = _L()
    rng = np.random.RandomState(5)
    n, Tcap, obs_dim, ldo = 4, 3, 3, 4
    rec = Recorder(rng, n, Tcap, obs_dim, ldo, dev)
    ins = [Guarded(np.zeros(n, np.float32), dev), Guarded(np.zeros(n, np.uint8), dev),
           Guarded(np.zeros((n, ldo), np.float32), dev)]

    def refused(match, **kw):
        r = rec.args(*ins, 0, 5, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        with pytest.raises(L.GarageAmdError, match=match):
            L.call('ga_record_step', C.byref(r), _stream())

    for field in ('reward', 'step_type', 'next_obs', 'ep_t', 'rew_buf', 'st_buf',
                  'tail_buf', 'lastobs_buf', 'done', 'step_eps', 'step_samples'):
        refused('null pointer', **{field: None})
    with pytest.raises(L.GarageAmdError, match='null pointer'):
        L.call('ga_record_step', None, _stream())
    refused('out of range', col=Tcap)
    refused('out of range', col=-1)
    refused('max_episode_length', max_episode_length=0)
    refused('max_episode_length', max_episode_length=65536)
    refused('leading dimensions', ldo=obs_dim - 1)
    torch.cuda.synchronize()
    rec.check('after the refusals')  # nothing was launched


# ---- ga_pack_episodes ----------------------------------------------------------------
def _column_enders(rng, n, kind):
    i = np.arange(n)
    last_pass = ((n - 1) // 256) * 256
    return [np.zeros(n, bool), np.ones(n, bool), i >= 256, i % 256 >= 192,
            i >= last_pass, rng.rand(n) < 0.3][kind]


def _tail_matrix(rng, n, Tcap, shift):
    """Column t: no ender / every env / only envs >= 256 / only the fourth wave of a
    pass / only the last partial pass / a random third, in turn from ``shift``."""
    tail = np.zeros((n, Tcap), np.uint16)
    for t in range(Tcap):
        ends = _column_enders(rng, n, (t + shift) % 6)
        tail[ends, t] = rng.randint(1, 65536, size=int(ends.sum()))
    return tail


def _pack(tail_dev, tail_byte_offset, n, Tcap, cols, base, n_eps, dev):
    outs = [Guarded.poisoned((n_eps, ), np.int32, dev) for _ in range(3)]
    base_dev = Guarded(np.asarray(base, np.int32), dev)
    _L().call('ga_pack_episodes', tail_dev.ptr(tail_byte_offset), n, Tcap, cols,
              base_dev.ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), _stream())
    torch.cuda.synchronize()
    _same(base_dev.host(), np.asarray(base, np.int32), 'ep_base changed')
    return [o.host() for o in outs]


@pytest.mark.parametrize('n_steps', [1, 7, 12])
@pytest.mark.parametrize('n', [1, 64, 255, 256, 257, 600, 1025])
def test_pack_episodes(n, n_steps, dev):
    Tcap = 12
    rng = np.random.RandomState(n * 13 + n_steps)
    for shift in range(6):
        tail = _tail_matrix(rng, n, Tcap, shift)
        env, end, length = ref.pack_order(tail[:, :n_steps])
        counts, base = ref.column_counts(tail[:, :n_steps])
        assert len(env) == counts.sum()
        tail_dev = Guarded(tail, dev)
        got = _pack(tail_dev, 0, n, Tcap, n_steps, base, len(env), dev)
        for g, w, name in zip(got, (env, end, length), ('ep_env', 'ep_end', 'ep_len')):
            _same(g, w.astype(np.int32), '{} (shift {})'.format(name, shift))
        _same(tail_dev.host(), tail, 'tail changed')


def test_pack_episodes_from_a_first_step(dev):
    """The sampler's ``first_step`` form: the tail and the column bases offset by a
    column, ``ep_end`` shifted afterwards (``GpuVecWorker._pack``)."""
    n, Tcap, first, n_steps = 600, 12, 5, 11
    rng = np.random.RandomState(9)
    tail = _tail_matrix(rng, n, Tcap, 1)
    step_eps = (tail[:, :n_steps] != 0).sum(axis=0)
    step_eps[:first] = 0
    base = np.concatenate([[0], np.cumsum(step_eps)[:-1]])
    env, end, length = ref.pack_order(tail[:, first:n_steps])
    assert len(env) == step_eps.sum() and (env >= 256).any() and (env < 256).any()
    got = _pack(Guarded(tail, dev), 2 * first, n, Tcap, n_steps - first, base[first:],
                len(env), dev)
    _same(got[0], env.astype(np.int32), 'ep_env')
    _same(got[1] + np.int32(first), (end + first).astype(np.int32), 'ep_end')
    _same(got[2], length.astype(np.int32), 'ep_len')


def test_pack_episodes_refusals(dev):
    L = _L()
    g = Guarded(np.zeros(64, np.int32), dev)
    p = g.ptr()
    bad = [(p, 4, 12, 13, p, p, p, p), (p, 0, 12, 3, p, p, p, p),
           (p, 4, 12, 0, p, p, p, p)]
    for k in (0, 4, 5, 6, 7):
        a = [p, 4, 12, 3, p, p, p, p]
        a[k] = None
        bad.append(tuple(a))
    for a in bad:
        with pytest.raises(L.GarageAmdError, match='bad sizes|null pointer'):
            L.call('ga_pack_episodes', *a, _stream())
    torch.cuda.synchronize()
    assert (g.host() == 0).all()


# ---- ga_pack_src_index ---------------------------------------------------------------
def _src_index(env, end, length, Tcap, dev):
    off, cells = ref.src_index(env, end, length, Tcap)
    assert 0 <= cells.min() and cells.max() < 2**31
    ins = [Guarded(np.asarray(a, np.int32), dev) for a in (env, end, length)]
    off_dev = Guarded(off, dev)
    src = Guarded.poisoned((int(off[-1]), ), np.int32, dev)
    _L().call('ga_pack_src_index', ins[0].ptr(), ins[1].ptr(), ins[2].ptr(),
              off_dev.ptr(), len(env), Tcap, src.ptr(), _stream())
    torch.cuda.synchronize()
    for g, w in zip(ins, (env, end, length)):
        _same(g.host(), np.asarray(w, np.int32), 'an input changed')
    return src.host(), cells.astype(np.int32)


def test_pack_src_index(dev):
    """Episodes of 1, 255, 256, 257 and 1000 steps (the 256-stride loop and its
    remainder), one from column 0, one up to Tcap - 1, two of one env, fragments
    (shorter than their episode), a far env."""
    Tcap = 1300
    eps = [(0, 0, 1), (5, Tcap - 1, 1), (1, 254, 255), (2, 255, 256), (3, 600, 257),
           (4, Tcap - 1, 1000), (7, 99, 100), (7, 399, 300), (6, 900, 300),
           (1, 1000, 3), (1_000_000, 700, 257), (9, 256, 257), (8, 511, 512)]
    env, end, length = (np.asarray(c) for c in zip(*eps))
    assert ((end - length + 1) == 0).any() and (end == Tcap - 1).any()
    got, want = _src_index(env, end, length, Tcap, dev)
    _same(got, want, 'src')
    # in the order a pack leaves them, at an odd Tcap
    rng = np.random.RandomState(4)
    tail = np.zeros((300, 37), np.uint16)
    for i in range(300):
        t = 0
        while True:
            L = int(rng.randint(1, 12))
            if t + L > 37:
                break
            tail[i, t + L - 1] = L
            t += L
    env, end, length = ref.pack_order(tail)
    got, want = _src_index(env, end, length, 37, dev)
    _same(got, want, 'src of a packed order')


def test_pack_src_index_refusals(dev):
    L = _L()
    g = Guarded(np.zeros(64, np.int64), dev)
    p = g.ptr()
    for a, match in (((p, p, p, p, 0, 8, p), 'bad n_eps'),
                     ((p, p, p, p, 2**31, 8, p), 'bad n_eps'),
                     ((p, p, p, p, 1, 0, p), 'too large'),
                     ((p, p, p, p, 1, 2**31, p), 'too large'),
                     ((None, p, p, p, 1, 8, p), 'null pointer'),
                     ((p, p, p, p, 1, 8, None), 'null pointer')):
        with pytest.raises(L.GarageAmdError, match=match):
            L.call('ga_pack_src_index', *a, _stream())
    torch.cuda.synchronize()
    assert (g.host() == 0).all()


# ---- the gathers ---------------------------------------------------------------------
def _indices(rng, count, n_src):
    """Repeated and descending, with 0 and the last row (both from 2 indices on)."""
    head = [n_src - 1, 0, 0, n_src - 1]
    down = list(range(n_src - 1, -1, -1))
    some = list(rng.randint(0, n_src, size=count))
    return np.asarray((head + down + some)[:count], np.int32)


@pytest.mark.parametrize('rows', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('width', [4, 8, 12, 36])
def test_gather_rows(width, rows, dev):
    rng = np.random.RandomState(width * 7 + rows)
    n_src, ld_src, ld_dst = 37, width + 4, width + 8
    assert (rows * width // 4) % 256  # the last block is a partial one
    src = _floats(rng, (n_src, ld_src))
    idx = _indices(rng, rows, n_src)
    want = _poison_like((rows, ld_dst), np.float32)
    want[:, :width] = src[idx, :width]
    d_src, d_idx = Guarded(src, dev), Guarded(idx, dev)
    dst = Guarded.poisoned((rows, ld_dst), np.float32, dev)
    _L().call('ga_gather_rows_f32', d_src.ptr(), ld_src, d_idx.ptr(), rows, width,
              dst.ptr(), ld_dst, _stream())
    torch.cuda.synchronize()
    _same(dst.host(), want, 'dst')
    _same(d_src.host(), src, 'src changed')
    _same(d_idx.host(), idx, 'idx changed')


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_gather_scalars(n, dev):
    rng = np.random.RandomState(n)
    n_src = 301
    idx = _indices(rng, n, n_src)
    for name, src in (('ga_gather_f32', _floats(rng, (n_src, ))),
                      ('ga_gather_u8',
                       rng.randint(0, 256, size=n_src).astype(np.uint8))):
        d_src, d_idx = Guarded(src, dev), Guarded(idx, dev)
        dst = Guarded.poisoned((n, ), src.dtype, dev)
        _L().call(name, d_src.ptr(), d_idx.ptr(), n, dst.ptr(), _stream())
        torch.cuda.synchronize()
        _same(dst.host(), src[idx], name)
        _same(d_src.host(), src, 'src changed')


def test_gather_refusals(dev):
    L = _L()
    g = Guarded(np.zeros(4096, np.float32), dev)
    p, p4 = g.ptr(), g.ptr(4)
    # (src, ld_src, idx, rows, width, dst, ld_dst)
    for a in ((p, 8, p, 4, 6, p, 8), (p, 10, p, 4, 8, p, 8), (p, 8, p, 4, 8, p, 10),
              (p, 4, p, 4, 8, p, 8), (p, 8, p, 4, 8, p, 4), (p, 8, p, 0, 8, p, 8),
              (p, 8, p, 4, 0, p, 8)):
        with pytest.raises(L.GarageAmdError, match='multiples of 4'):
            L.call('ga_gather_rows_f32', *a, _stream())
    for a in ((p4, 8, p, 4, 8, p, 8), (p, 8, p, 4, 8, p4, 8)):
        with pytest.raises(L.GarageAmdError, match='16-B alignment'):
            L.call('ga_gather_rows_f32', *a, _stream())
    for a in ((None, 8, p, 4, 8, p, 8), (p, 8, None, 4, 8, p, 8),
              (p, 8, p, 4, 8, None, 8)):
        with pytest.raises(L.GarageAmdError, match='null pointer'):
            L.call('ga_gather_rows_f32', *a, _stream())
    for name in ('ga_gather_f32', 'ga_gather_u8'):
        for a in ((p, p, 0, p), (None, p, 4, p), (p, None, 4, p), (p, p, 4, None)):
            with pytest.raises(L.GarageAmdError, match='bad arguments'):
                L.call(name, *a, _stream())
    torch.cuda.synchronize()
    assert (g.host().view(np.int32) == 0).all()


# ---- one chain through all of it -----------------------------------------------------
def _scripted_step_types(rng, n, cols, P):
    """Envs running episodes of scripted lengths back to back: FIRST, MID ...,
    TERMINAL at the scripted end; at P an even env reports TIMEOUT and an odd one
    plain MID (the record must end it by its length)."""
    st = np.zeros((n, cols), np.uint8)
    for i in range(n):
        t, L = 0, int(rng.choice([1, 2, 3, 5, 8]))
        for c in range(cols):
            t += 1
            if t >= P:
                st[i, c] = 3 if i % 2 == 0 else 1
            elif t >= L:
                st[i, c] = 2
            else:
                st[i, c] = 0 if t == 1 else 1
            if t >= min(L, P):
                t, L = 0, int(rng.choice([1, 2, 3, 5, 8]))
    return st


def test_record_pack_gather_chain(dev):
    """Scripted step types through ``ga_record_step`` column by column, then packed
    and gathered exactly as ``GpuVecWorker._pack`` does."""
    L = _L()
    rng = np.random.RandomState(21)
    n, Tcap, obs_dim, ldo, P = 300, 8, 5, 8, 4
    st = _scripted_step_types(rng, n, Tcap, P)
    rec = Recorder(rng, n, Tcap, obs_dim, ldo, dev, zero_counts=True)
    rec.state['tail'][:] = 0  # as _alloc_buffers hands them out
    rec.d['tail'] = Guarded(rec.state['tail'], dev)
    obs = _floats(rng, (n, Tcap, ldo))
    d_obs = Guarded(obs, dev)
    for col in range(Tcap):
        rec.step(_floats(rng, (n, )), st[:, col], _next_obs(rng, n, obs_dim, ldo), col,
                 P, 0)
    bufs = dict(rec.state, obs=obs)
    want = ref.packed_batch(bufs, Tcap, Tcap)
    counts, _ = ref.column_counts(rec.state['tail'])
    per_col_low = [(want['ep_env'][want['ep_end'] == c] < 256).sum()
                   for c in range(Tcap)]
    assert min(per_col_low) >= 2 and min(counts - per_col_low) >= 2
    assert set(want['lengths'].tolist()) == {1, 2, 3, 4}
    # -- GpuVecWorker._pack, on the device buffers --
    step_eps = rec.d_eps.host().astype(np.int64)
    _same(step_eps, counts, 'step_eps against the order\'s column counts')
    ep_base = np.concatenate([[0], np.cumsum(step_eps)[:-1]])
    n_eps = int(step_eps.sum())
    ep = [Guarded.poisoned((n_eps, ), np.int32, dev) for _ in range(3)]
    base_dev = Guarded(ep_base.astype(np.int32), dev)
    s = _stream()
    L.call('ga_pack_episodes', rec.d['tail'].ptr(), n, Tcap, Tcap, base_dev.ptr(),
           ep[0].ptr(), ep[1].ptr(), ep[2].ptr(), s)
    torch.cuda.synchronize()
    ep_env, ep_end, ep_len = (e.host() for e in ep)
    lengths = ep_len.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lengths)])
    S = int(off[-1])
    off_dev = Guarded(off, dev)
    src = Guarded.poisoned((S, ), np.int32, dev)
    L.call('ga_pack_src_index', ep[0].ptr(), ep[1].ptr(), ep[2].ptr(), off_dev.ptr(),
           n_eps, Tcap, src.ptr(), s)
    cell = Guarded((ep_env.astype(np.int64) * Tcap + ep_end).astype(np.int32), dev)

    def rows(buf, idx, count):
        out = Guarded.poisoned((count, ldo), np.float32, dev)
        L.call('ga_gather_rows_f32', buf.ptr(), ldo, idx.ptr(), count, ldo, out.ptr(),
               ldo, s)
        return out

    g_obs = rows(d_obs, src, S)
    g_last = rows(rec.d['lastobs'], cell, n_eps)
    g_rew = Guarded.poisoned((S, ), np.float32, dev)
    L.call('ga_gather_f32', rec.d['rew'].ptr(), src.ptr(), S, g_rew.ptr(), s)
    g_st = Guarded.poisoned((S, ), np.uint8, dev)
    L.call('ga_gather_u8', rec.d['st'].ptr(), src.ptr(), S, g_st.ptr(), s)
    torch.cuda.synchronize()
    _same(ep_env, want['ep_env'].astype(np.int32), 'ep_env')
    _same(ep_end, want['ep_end'].astype(np.int32), 'ep_end')
    _same(lengths, want['lengths'], 'lengths')
    _same(off, want['off'], 'offsets')
    _same(src.host(), want['cells'].astype(np.int32), 'src')
    _same(g_obs.host(), want['obs'], 'obs')
    _same(g_last.host(), want['last_obs'], 'last_obs')
    _same(g_rew.host(), want['rew'], 'rew')
    _same(g_st.host(), want['st'], 'st')
    rec.check('after the pack')  # packing reads only


# ---- ga_permutation_i32 --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_permutation(n, key):
    out = ref.feistel_permutation(n, key).astype(np.int32)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize('n', PERM_SIZES)
def test_permutation(n, dev):
    for key in KEYS:
        out = Guarded.poisoned((n, ), np.int32, dev)
        _L().call('ga_permutation_i32', n, key, out.ptr(), _stream())
        torch.cuda.synchronize()
        got = out.host()
        _same(got, _reference_permutation(n, key), 'key {:#x}'.format(key))
        assert np.array_equal(np.sort(got), np.arange(n))


def test_permutation_refusals(dev):
    L = _L()
    g = Guarded(np.zeros(64, np.int32), dev)
    for a in ((0, 1, g.ptr()), (2**30, 1, g.ptr()), (-1, 1, g.ptr()), (8, 1, None)):
        with pytest.raises(L.GarageAmdError, match='bad arguments'):
            L.call('ga_permutation_i32', *a, _stream())
    torch.cuda.synchronize()
    assert (g.host() == 0).all()


def test_optimizer_minibatches_partition_the_ids(dev):
    """``OptimizerWrapper(permutation='device')``: the minibatches of a pass are a
    partition of ``range(n)``, passes differ, the seed decides."""
    from garage_amd.envs import SyntheticVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import GaussianMLPPolicy
    n, mb, passes = 1000, 64, 3
    assert n % mb
    pol = GaussianMLPPolicy(SyntheticVecEnv(2, 3, 2, 4, seed=1).spec,
                            hidden_sizes=(8, ))

    def all_passes(seed):
        opt = OptimizerWrapper((torch.optim.Adam, dict(lr=1e-3)), pol,
                               max_optimization_epochs=passes, minibatch_size=mb,
                               permutation='device', seed=seed)
        parts = [p.cpu().numpy() for p in opt.minibatch_indices(n)]
        per_pass = -(-n // mb)
        assert len(parts) == passes * per_pass
        out = []
        for k in range(passes):
            mine = parts[k * per_pass:(k + 1) * per_pass]
            assert [len(p) for p in mine] == [mb] * (per_pass - 1) + [n % mb]
            ids = np.concatenate(mine)
            assert ids.dtype == np.int32
            assert np.array_equal(np.sort(ids), np.arange(n))
            out.append(ids)
        return out

    a, b, c = all_passes(5), all_passes(5), all_passes(6)
    for k in range(passes):
        assert np.array_equal(a[k], b[k])
        assert not np.array_equal(a[k], c[k])
        assert not np.array_equal(a[k], np.arange(n))
    for k in range(1, passes):
        assert not np.array_equal(a[k], a[k - 1])
