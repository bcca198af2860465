"""A population's joint pack, as far as it goes without a GPU: the numpy twin of
``ga_member_pack_index`` (``_member_pack_ref.py``) against the single-member twin
(``_episode_pack_ref.py``) applied to each member's rows, the layout rules of the
header, every refusal of ``ga_member_pack_index`` / ``ga_member_pack_gather`` through
ctypes with host pointers (each check precedes the first launch), the ctypes mirror of
``ga_pack_plane``, the host code under a sanitizer and ``DevicePopulationBatch``."""
import ctypes as C
import os
import pickle
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from garage_amd import _lib
from garage_amd._dtypes import DevicePopulationBatch

from _episode_pack_ref import pack_order, src_index
from _member_pack_ref import cases, member_progress, pack_index, round16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()


# -- the twin against the single-member twin ---------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_twin_equals_the_single_member_twin_per_member(name):
    tail, M, n_cols, num_samples = CASES[name]
    n, tcap = tail.shape
    g = n // M
    progress, col_base = member_progress(tail, M, n_cols, num_samples)
    got = pack_index(tail, M, progress)
    start = got['episode_start']
    for m in range(M):
        c = int(progress[m, 0])
        env, end, length = pack_order(tail[m * g:(m + 1) * g, :c])
        off, cells = src_index(env + m * g, end, length, tcap)
        e0, e1 = start[m], start[m + 1]
        assert e1 - e0 == len(env) == (progress[m, 1] if c else 0)
        assert np.array_equal(got['ep_env'][e0:e1], env + m * g)
        assert np.array_equal(got['ep_end'][e0:e1], end)
        assert np.array_equal(got['ep_len'][e0:e1], length)
        # the member's own entries of ep_off: relative, from 0 to S_m
        assert np.array_equal(got['ep_off'][e0 + m:e1 + m + 1], off)
        assert got['member_samples'][m] == off[-1]
        lo = got['member_off'][m]
        assert np.array_equal(got['src'][lo:lo + off[-1]], cells)
        # col_base is what ranks the member's episodes of a column
        for e in range(len(env)):
            first = e0 + col_base[m, end[e]]
            assert first <= e0 + e < first + g
    if name == 'c=0':
        assert progress[1, 0] == 0 and start[2] == start[1]
        assert got['member_samples'][1] == 0
    if name == 'different-c':
        assert len(set(progress[:, 0])) == 3
    if name == 'length-Tcap':
        assert (got['ep_len'] == tcap).sum() == 2
    if name == 'length-1':
        assert (got['ep_len'] == 1).all()


@pytest.mark.parametrize('name', list(CASES))
def test_member_slices_are_aligned_disjoint_and_padded_with_minus_one(name):
    tail, M, n_cols, num_samples = CASES[name]
    g = tail.shape[0] // M
    progress, _ = member_progress(tail, M, n_cols, num_samples)
    got = pack_index(tail, M, progress)
    off, S, src = got['member_off'], got['member_samples'], got['src']
    assert off[0] == 0 and (off % 16 == 0).all()
    assert np.array_equal(off[1:], off[:-1] + round16(S))  # back to back
    assert (S <= g * progress[:, 0]).all()  # the bound the arrays are sized by
    assert len(src) == round16(g * progress[:, 0].astype(np.int64)).sum()
    sample = np.zeros(len(src), dtype=bool)
    for m in range(M):
        assert not sample[off[m]:off[m] + S[m]].any()
        sample[off[m]:off[m] + S[m]] = True
    assert np.array_equal(src == -1, ~sample)
    # every cell is packed once
    assert len(np.unique(src[sample])) == sample.sum()


# -- the C ABI's refusals ------------------------------------------------------------
N, TCAP, COLS, MEMBERS = 64, 8, 6, 2
INDEX_PTRS = ('tail', 'progress', 'col_base', 'ep_env', 'ep_end', 'ep_len',
              'ep_off', 'member_samples', 'member_off', 'src')


def _index(n=N, tcap=TCAP, cols=COLS, members=MEMBERS, max_eps=4, max_samples=16,
           **ptrs):
    buf = (C.c_double * 16)()
    a = {k: C.addressof(buf) for k in INDEX_PTRS}
    a.update(ptrs)
    _lib.call('ga_member_pack_index', a['tail'], n, tcap, cols, members,
              a['progress'], a['col_base'], max_eps, max_samples, a['ep_env'],
              a['ep_end'], a['ep_len'], a['ep_off'], a['member_samples'],
              a['member_off'], a['src'], None)


def _gather(planes='default', n_planes=None, src='buf', n_rows=16, ep_env='buf',
            ep_end='buf', n_eps=4, tcap=TCAP, **plane):
    buf = (C.c_double * 16)()
    addr = C.addressof(buf)
    assert addr % 16 == 0
    fields = dict(src=addr, dst=addr, ld_src=4, ld_dst=4, elem_size=4, width=4,
                  per_episode=0)
    # (the plane's own pointers are given as plane_src / plane_dst)
    fields.update({k.replace('plane_', ''): v for k, v in plane.items()})
    table = (_lib.PackPlane * 17)(*[_lib.PackPlane(**fields)] * 17)
    pick = lambda v: addr if v == 'buf' else v
    _lib.call('ga_member_pack_gather', table if planes == 'default' else planes,
              1 if n_planes is None else n_planes, pick(src), n_rows,
              pick(ep_env), pick(ep_end), n_eps, tcap, None)


def test_every_refusal_of_the_index_precedes_the_launch():
    err = _lib.GarageAmdError
    for name in INDEX_PTRS:
        with pytest.raises(err, match='ga_member_pack_index: null pointer'):
            _index(**{name: None})
    for bad in (0, -2, 1025):
        with pytest.raises(err, match=r'n_members must be in 1\.\.1024'):
            _index(members=bad, n=2050 if bad > 0 else N)
    with pytest.raises(err, match='64 envs do not split into 3 members'):
        _index(members=3)
    for bad in (0, -1, TCAP + 1):
        with pytest.raises(err, match=r'n_cols must be in 1\.\.Tcap'):
            _index(cols=bad)
    with pytest.raises(err, match='rollout buffers too large'):
        _index(n=1 << 20, tcap=1 << 11, cols=4)
    for bad in (0, -3):
        with pytest.raises(err, match='max_eps must be at least 1'):
            _index(max_eps=bad)
    for bad in (0, -1, 1 << 31):
        with pytest.raises(err, match=r'max_samples must be in 1\.\.2\^31 - 1'):
            _index(max_samples=bad)
    assert b'ga_member_pack_index' in _lib.load().ga_last_error()


def test_every_refusal_of_the_gather_precedes_the_launch():
    err = _lib.GarageAmdError
    who = 'ga_member_pack_gather'
    with pytest.raises(err, match=who + ': null pointer'):
        _gather(planes=None)
    with pytest.raises(err, match=who + ': null pointer'):
        _gather(src=None)
    for name in ('plane_src', 'plane_dst'):
        with pytest.raises(err, match='null pointer in plane 0'):
            _gather(**{name: None})
    for name in ('ep_env', 'ep_end'):
        with pytest.raises(err, match=r'null pointer \(plane 0 is per episode\)'):
            _gather(per_episode=1, **{name: None})
    with pytest.raises(err, match='plane 0 is per episode and n_eps is 0'):
        _gather(per_episode=1, n_eps=0)
    for bad in (0, -1, 17):
        with pytest.raises(err, match=r'n_planes must be in 1\.\.16'):
            _gather(n_planes=bad)
    for bad in (0, -1, 1 << 31):
        with pytest.raises(err, match='n_rows must be in'):
            _gather(n_rows=bad)
    with pytest.raises(err, match='bad n_eps'):
        _gather(n_eps=-1)
    for bad in (0, 1 << 31):
        with pytest.raises(err, match='Tcap must be in'):
            _gather(tcap=bad)
    for bad in (0, 2, 8):
        with pytest.raises(err, match='elem_size must be 1 or 4'):
            _gather(elem_size=bad)
    with pytest.raises(err, match='rows of 0 elements'):
        _gather(width=0)
    with pytest.raises(err, match='rows of 8 elements with strides 4 / 8'):
        _gather(width=8, ld_dst=8)
    with pytest.raises(err, match='rows of 8 elements with strides 8 / 4'):
        _gather(width=8, ld_src=8)
    # 4-byte rows of width >= 4 are quads on both sides
    buf = (C.c_double * 16)()
    addr = C.addressof(buf)
    for bad in (dict(width=6, ld_src=8, ld_dst=8), dict(ld_src=6), dict(ld_dst=5),
                dict(plane_src=addr + 4), dict(plane_dst=addr + 8)):
        with pytest.raises(err, match='copied as 16-byte quads'):
            _gather(**bad)
    # the last plane of several is checked like the first
    table = (_lib.PackPlane * 3)(*[_lib.PackPlane(
        src=addr, dst=addr, ld_src=4, ld_dst=4, elem_size=4, width=4)] * 3)
    table[2].elem_size = 3
    with pytest.raises(err, match='plane 2: elem_size must be 1 or 4'):
        _gather(planes=table, n_planes=3)
    assert who.encode() in _lib.load().ga_last_error()


def test_header_states_the_entries_and_the_abi_stays_5():
    text = open(os.path.join(ROOT, 'include', 'garage_amd.h')).read()
    for name in ('ga_member_pack_index', 'ga_member_pack_gather'):
        assert 'GA_API int %s(' % name in text
        assert name in _lib.SIGNATURES
    start = text.index('a population\'s episodes packed in one pass')
    assert 'vec_worker.py:206-219' in text[start:]
    assert 'Refused before any launch' in text[start:]
    assert '#define GA_PACK_MAX_PLANES %d' % _lib.PACK_MAX_PLANES in text
    assert _lib.load().ga_abi_version() == 5


def test_pack_plane_mirror_matches_the_header():
    py = _lib.PackPlane
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%zu\\n", sizeof(ga_pack_plane));']
    want = [str(C.sizeof(py))]
    for field, ftype in py._fields_:
        lines.append('printf("{0} %zu %zu\\n", offsetof(ga_pack_plane, {0}), '
                     'sizeof(((ga_pack_plane*)0)->{0}));'.format(field))
        want.append('{} {} {}'.format(field, getattr(py, field).offset,
                                      C.sizeof(ftype)))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == want


def test_host_side_under_address_sanitizer():
    """``make asan-member-pack``: the two entries' checks, the gather's plane table
    and the grids of the three launches (member_pack_host.cpp) compiled with
    ``-fsanitize=address,undefined`` for the CPU and run against recording fakes of
    the launches (tests/host/member_pack_harness.cpp)."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-member-pack'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'member pack ok' in out.stdout


# -- the batch class -------------------------------------------------------------------
def test_device_population_batch_holds_views_and_pickles():
    from garage_amd._dtypes import Box, DeviceEpisodeBatch, EnvSpec
    spec = EnvSpec(Box(-1, 1, (4, )), Box(-1, 1, (4, )), max_episode_length=8)
    obs = torch.arange(32 * 4, dtype=torch.float32).reshape(32, 4)
    rew, st = obs[:, 0].clone(), obs[:, 1].to(torch.uint8)
    last = obs[:3] + 0.5
    ep_off = torch.tensor([0, 2, 5, 0, 3])  # 2 episodes, then 1: M + N entries
    packed = dict(obs_dev=obs, actions_dev=obs + 1, head_dev=None, rewards_dev=rew,
                  step_types_dev=st, last_obs_dev=last, ep_off_dev=ep_off,
                  env_info_planes={}, member_off=[0, 16, 32],
                  member_samples=[5, 3], episode_start=[0, 2, 3])
    members = [
        DeviceEpisodeBatch(spec, lengths=[2, 3], obs_dev=obs[0:5],
                           last_obs_dev=last[0:2], actions_dev=(obs + 1)[0:5],
                           rewards_dev=rew[0:5], step_types_dev=st[0:5],
                           ep_off_dev=ep_off[0:3], log_std=-0.5),
        DeviceEpisodeBatch(spec, lengths=[3], obs_dev=obs[16:19],
                           last_obs_dev=last[2:3], actions_dev=(obs + 1)[16:19],
                           rewards_dev=rew[16:19], step_types_dev=st[16:19],
                           ep_off_dev=ep_off[3:5], log_std=0.25)]
    pop = DevicePopulationBatch(members, **packed)
    assert len(pop) == 2 and pop.member_off.dtype == np.int64
    for m, b in enumerate(members):  # member_views states the constructor's slices
        for name, view in pop.member_views(m).items():
            want = getattr(b, name)
            assert (view is None and want is None) or torch.equal(view, want)
    copy = pickle.loads(pickle.dumps(pop))
    assert torch.equal(copy.obs_dev, obs) and copy.head_dev is None
    assert np.array_equal(copy.member_samples, [5, 3])
    for a, b in zip(copy.members, members):
        assert isinstance(a, DeviceEpisodeBatch) and a.head_dev is None
        assert torch.equal(a.obs_dev, b.obs_dev)
        assert torch.equal(a.ep_off_dev, b.ep_off_dev)
        assert torch.equal(a.last_obs_dev, b.last_obs_dev)
        assert np.array_equal(a.lengths, b.lengths) and a._log_std == b._log_std
        assert np.array_equal(a.rewards, b.rewards)  # the lazy host side works
    # the packed arrays are stored once: the members are views again
    assert copy.members[1].obs_dev.data_ptr() == copy.obs_dev[16].data_ptr()
    assert copy.members[1].ep_off_dev.data_ptr() == copy.ep_off_dev[3].data_ptr()
    with pytest.raises(ValueError, match='2 members need 3 offsets'):
        DevicePopulationBatch(members, **dict(packed, member_off=[0, 16]))
