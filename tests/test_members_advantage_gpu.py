"""``ga_advantages_members_f32``: every member's returns, advantages and normalisation
in one launch against the lone entry points (bit for bit) and the fp64 reference of
``_advantage_cases.py``, inside sentinels; and its refusals (GPU box)."""
import functools

import numpy as np
import pytest
import torch

import _advantage_cases as cases

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
LEAD = 8  # floats in front of every output (keeps its 16-byte alignment)


@functools.lru_cache(maxsize=None)
def _reference(name, m, center, positive):
    P, members = cases.CASES[name]
    rew, val = cases.inputs(name, m)
    mem = members[m]
    return cases.reference(rew, val, cases.lengths(mem), P, mem[2], mem[3], center,
                           positive)


class _Member:
    """Device inputs of one member and two sets of sentinel-filled outputs (joint,
    lone) in the member's layout."""

    def __init__(self, dev, name, m, shift):
        self.layout, self.shape, v0, self.bonus = cases.CASES[name][1][m]
        rew, val = cases.inputs(name, m)
        self.lens = cases.lengths(cases.CASES[name][1][m])
        self.S = int(self.lens.sum())
        self.v0 = None if v0 is None else torch.tensor([v0], dtype=torch.float32,
                                                       device=dev)
        self.off = None
        if self.layout == 'matrix':
            N, L, ld = self.shape
            self.n = N * ld

            def place(x):
                host = np.zeros((N, ld), np.float32)
                host[:, :L] = x.reshape(N, L)
                return torch.from_numpy(host.reshape(-1)).to(dev)
        else:
            self.n = self.S
            self.off = torch.from_numpy(
                np.concatenate([[0], np.cumsum(self.lens)])).to(dev)

            def place(x):
                return torch.from_numpy(x).to(dev)
        self.rew, self.val = place(rew), place(val)
        # (shift: a member whose outputs sit 4 bytes off alignment takes the general
        # kernel's scalar path in both calls)
        lead = LEAD + shift
        self.outs = [{k: torch.full((lead + self.n + LEAD, ), SENTINEL, device=dev)
                      for k in ('adv', 'ret')} for _ in range(2)]
        self.stats = [torch.zeros(4, dtype=torch.float64, device=dev) for _ in range(2)]
        self.lead = lead

    def view(self, which, k):
        return self.outs[which][k][self.lead:self.lead + self.n]

    def packed(self, flat):
        """The valid steps of a buffer in this member's layout, packed."""
        if self.layout == 'matrix':
            N, L, ld = self.shape
            return flat.view(N, ld)[:, :L].contiguous().view(-1)
        return flat

    def untouched(self, which, k):
        buf = self.outs[which][k]
        ok = bool((buf[:self.lead] == SENTINEL).all()) and \
            bool((buf[self.lead + self.n:] == SENTINEL).all())
        if self.layout == 'matrix' and self.shape[2] > self.shape[1]:
            N, L, ld = self.shape
            ok = ok and bool((self.view(which, k).view(N, ld)[:, L:] == SENTINEL).all())
        return ok

    def lone(self, P, center, positive):
        """``VPG._before_train``'s calls on this member alone."""
        from garage_amd.engine import center_advantages, gae_scan
        v0 = 0.0 if self.v0 is None else float(self.v0.item())
        adv, ret = self.view(1, 'adv'), self.view(1, 'ret')
        kw = dict(discount=cases.DISCOUNT, gae_lambda=cases.GAE_LAMBDA,
                  max_episode_length=P, v0=v0, bonus_const=self.bonus)
        if self.layout == 'matrix':
            N, L, ld = self.shape
            rows = [t.view(N, ld)[:, :L] for t in (self.rew, self.val, adv, ret)]
            gae_scan(rows[0], rows[1], adv=rows[2], ret=rows[3], **kw)
        else:
            gae_scan(self.rew, self.val, offsets=self.off, max_len=int(self.lens.max()),
                     adv=adv, ret=ret, **kw)
        flat = self.packed(adv)  # (a copy where the rows lie ld > L apart)
        center_advantages(flat, center=center, positive=positive, stats=self.stats[1])
        return flat, self.packed(ret)


def _call(members, P, center, positive):
    from garage_amd import _lib
    arr = (_lib.MemberAdvantage * len(members))()
    for u, mem in zip(arr, members):
        u.rewards, u.values = mem.rew.data_ptr(), mem.val.data_ptr()
        if mem.layout == 'matrix':
            u.n_rows, u.T, u.ld = mem.shape
            u.max_len = mem.shape[1]
        else:
            u.offsets = mem.off.data_ptr()
            u.n_rows, u.T, u.ld, u.max_len = len(mem.lens), mem.S, 0, int(mem.lens.max())
        u.v0 = None if mem.v0 is None else mem.v0.data_ptr()
        u.bonus_const = mem.bonus
        u.adv, u.ret = mem.view(0, 'adv').data_ptr(), mem.view(0, 'ret').data_ptr()
        u.stats = mem.stats[0].data_ptr()
    return arr


def _one_ulp(got, ref, rowmax):
    """The bar of ``test_gae_scan_edges_gpu.py``."""
    bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-9 * rowmax
    return np.abs(got.astype(np.float64) - ref) <= bound


@pytest.mark.parametrize('center,positive', cases.OPTIONS)
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_every_member_gets_the_bits_of_its_lone_launches(name, center, positive):
    from garage_amd._lib import call, stream_ptr
    from garage_amd.engine import require_gpu
    dev = require_gpu()
    P, table = cases.CASES[name]
    members = [_Member(dev, name, m, shift=int(name == 'block-steps' and m == 2))
               for m in range(len(table))]
    arr = _call(members, P, center, positive)
    call('ga_advantages_members_f32', arr, len(members), P, cases.DISCOUNT,
         cases.GAE_LAMBDA, int(center), int(positive), stream_ptr())
    for m, mem in enumerate(members):
        where = (name, m, center, positive)
        lone_adv, lone_ret = mem.lone(P, center, positive)
        adv = mem.packed(mem.view(0, 'adv'))
        ret = mem.packed(mem.view(0, 'ret'))
        # (a) bit for bit the lone entry points', NaN included
        assert torch.equal(adv.view(torch.int32), lone_adv.view(torch.int32)), where
        assert torch.equal(ret.view(torch.int32), lone_ret.view(torch.int32)), where
        assert torch.equal(mem.stats[0].view(torch.int64),
                           mem.stats[1].view(torch.int64)), where
        # (c) nothing written outside
        assert all(mem.untouched(0, k) for k in ('adv', 'ret')), where
        # (b) within tolerance of the fp64 reference
        raw, ref_ret, ref_adv, amax, gmax, scale = _reference(name, m, center, positive)
        got, got_ret = adv.cpu().numpy(), ret.cpu().numpy()
        assert _one_ulp(got_ret, ref_ret, gmax).all(), where
        if not (center or positive):
            assert _one_ulp(got, raw, amax).all(), where
        else:
            assert (np.isnan(got) == np.isnan(ref_adv)).all(), where
            err = np.abs(got - ref_adv)[~np.isnan(ref_adv)]
            print(where, 'worst error / bound',
                  float(err.max() / cases.bound(scale, center, positive))
                  if err.size else 'nan batch')
            assert (err <= cases.bound(scale, center, positive)).all(), where


REFUSALS = [
    (dict(rewards=None), 'null pointer'),
    (dict(stats=None), 'null pointer'),
    (dict(n_rows=0), 'S < 1'),
    (dict(n_rows=4097, T=8, ld=8), 'MA_MAX_STEPS'),
    (dict(ld=3), 'ld (3) < T (4)'),
    (dict(count=0), 'n_members must be 1 .. 1024'),
    (dict(count=1025), 'n_members must be 1 .. 1024'),
]


@pytest.mark.parametrize('change,message', REFUSALS)
def test_a_refused_argument_is_named(change, message):
    """... before any launch: the outputs keep their sentinels."""
    from garage_amd import _lib
    from garage_amd.engine import require_gpu
    dev = require_gpu()
    mem = _Member(dev, 'block-steps', 1, 0)
    change = dict(change)
    count = change.pop('count', 1)
    arr = (_lib.MemberAdvantage * max(1, count))()
    arr[0] = _call([mem], 7, True, False)[0]
    for k, v in change.items():
        setattr(arr[0], k, v)
    with pytest.raises(_lib.GarageAmdError) as err:
        _lib.call('ga_advantages_members_f32', arr, count, 7, 0.99, 0.95, 1, 0,
                  _lib.stream_ptr())
    assert message in str(err.value)
    torch.cuda.synchronize()
    assert bool((mem.outs[0]['adv'] == SENTINEL).all())
