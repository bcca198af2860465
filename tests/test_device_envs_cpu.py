"""Device PointEnv / GridWorldEnv batches, the parts that need no GPU: numpy
twins of the reference environments reproduce the committed goldens (which the
real reference produced, tests/golden/make_golden_device_envs.py) bit for bit,
the task draw, argument checking, the C structs and the C ABI's argument errors.
The GPU tests (test_device_envs_gpu.py) hold the kernels to the same goldens and
to ``HostVecEnv`` batches of these twins."""
import collections
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from garage_amd._dtypes import Box, Discrete, EnvSpec, StepType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EnvStep = collections.namedtuple('EnvStep',
                                 'observation reward step_type env_info')


class PointTwin:
    """``garage.envs.PointEnv`` (envs/point_env.py:79-170) in plain numpy."""

    def __init__(self, goal=(1., 1.), arena_size=5., done_bonus=0.,
                 never_done=False, max_episode_length=None):
        self._goal = np.array(goal, dtype=np.float32)
        self._arena, self._bonus = arena_size, done_bonus
        self._never_done = never_done
        self._max = max_episode_length
        self._point = np.zeros_like(self._goal)
        self.spec = EnvSpec(Box(-np.inf, np.inf, (3, )), Box(-0.1, 0.1, (2, )),
                            max_episode_length=max_episode_length)
        self._low = np.full(2, -0.1, np.float32)
        self._high = np.full(2, 0.1, np.float32)

    def reset(self):
        self._point = np.zeros_like(self._goal)
        dist = np.linalg.norm(self._point - self._goal)
        self._cnt = 0
        return np.concatenate([self._point, (dist, )]), dict(goal=self._goal)

    def step(self, action):
        a = np.clip(np.array(action, dtype=np.float32), self._low, self._high)
        self._point = np.clip(self._point + a, -self._arena, self._arena)
        dist = np.linalg.norm(self._point - self._goal)
        succ = dist < np.linalg.norm(self._low)
        reward = -dist
        if succ:
            reward += self._bonus
        self._cnt += 1
        st = StepType.get_step_type(step_cnt=self._cnt,
                                    max_episode_length=self._max,
                                    done=succ and not self._never_done)
        return EnvStep(np.concatenate([self._point, (dist, )]), float(reward),
                       st, {'success': succ})

    def close(self):
        pass


class GridTwin:
    """``garage.envs.GridWorldEnv`` (envs/grid_world_env.py:111-215) in plain
    numpy, without the reference's np.random.choice over one outcome."""

    def __init__(self, rows, max_episode_length=None):
        desc = np.array([list(r) for r in rows])
        desc[desc == '.'] = 'F'
        desc[desc == 'o'] = 'H'
        desc[desc == 'x'] = 'W'
        self._desc = desc
        self._r, self._c = desc.shape
        (sx, ), (sy, ) = np.nonzero(desc == 'S')
        self._start = sx * self._c + sy
        self._max = max_episode_length
        self.spec = EnvSpec(Discrete(self._r * self._c), Discrete(4),
                            max_episode_length=max_episode_length)

    def reset(self):
        self._state, self._cnt = self._start, 0
        return self._state, {}

    def step(self, action):
        x, y = divmod(self._state, self._c)
        inc = [[0, -1], [1, 0], [0, 1], [-1, 0]][int(action)]
        nx = min(max(x + inc[0], 0), self._r - 1)
        ny = min(max(y + inc[1], 0), self._c - 1)
        if (self._desc[nx, ny] != 'W'
                and self._desc[x, y] not in ('H', 'G')):
            self._state = nx * self._c + ny
        kind = self._desc[divmod(self._state, self._c)]
        done = kind in ('H', 'G')
        self._cnt += 1
        st = StepType.get_step_type(step_cnt=self._cnt,
                                    max_episode_length=self._max, done=done)
        return EnvStep(self._state, 1.0 if kind == 'G' else 0.0, st, {})

    def close(self):
        pass


def grid_rows(g, k):
    from garage_amd.envs import GRID_MAPS
    name = str(g['c%d_name' % k])
    return list(GRID_MAPS[name]) if name else [str(r) for r in g['c%d_rows' % k]]


def point_groups(g):
    for k in range(int(g['n_groups'])):
        arena, bonus, never, max_len = g['g%d_cfg' % k]
        yield k, dict(arena_size=float(arena), done_bonus=float(bonus),
                      never_done=bool(never), max_episode_length=int(max_len))


def _ended(st):
    return int(st) >= int(StepType.TERMINAL)


def test_point_twin_reproduces_the_reference(golden):
    g = golden('point_env')
    for k, cfg in point_groups(g):
        envs = [PointTwin(goal=goal, **cfg) for goal in g['g%d_goals' % k]]
        obs0 = np.stack([e.reset()[0] for e in envs])
        assert np.array_equal(obs0, g['g%d_obs0' % k])
        for t, acts in enumerate(g['g%d_actions' % k]):
            for i, e in enumerate(envs):
                es = e.step(acts[i])
                assert np.array_equal(es.observation, g['g%d_next_obs' % k][t, i])
                assert np.float32(es.reward) == g['g%d_reward' % k][t, i]
                assert int(es.step_type) == g['g%d_step_type' % k][t, i]
                assert es.env_info['success'] == g['g%d_success' % k][t, i]
                if _ended(es.step_type):
                    assert np.array_equal(e.reset()[0],
                                          g['g%d_obs_after' % k][t, i])


def test_grid_twin_reproduces_the_reference(golden):
    g = golden('grid_env')
    for k in range(int(g['n_cases'])):
        envs = [GridTwin(grid_rows(g, k), int(g['c%d_max_len' % k]))
                for _ in range(3)]
        assert [e.reset()[0] for e in envs] == list(g['c%d_start' % k])
        for t, acts in enumerate(g['c%d_actions' % k]):
            for i, e in enumerate(envs):
                es = e.step(acts[i])
                assert es.observation == g['c%d_next' % k][t, i]
                assert np.float32(es.reward) == g['c%d_reward' % k][t, i]
                assert int(es.step_type) == g['c%d_step_type' % k][t, i]
                if _ended(es.step_type):
                    assert e.reset()[0] == g['c%d_after' % k][t, i]


def test_sample_tasks_draws_like_the_reference(golden):
    from garage_amd.envs import PointVecEnv
    np.random.seed(123)
    tasks = PointVecEnv.sample_tasks(5)
    got = np.stack([t['goal'] for t in tasks])
    assert got.dtype == np.float64
    assert np.array_equal(got, golden('point_env')['sample_tasks_seed123'])


def test_arguments_are_checked_before_any_device_work():
    from garage_amd.envs import GridWorldVecEnv, PointVecEnv
    with pytest.raises(ValueError, match='outside the arena'):
        PointVecEnv(4, goal=(2.5, 0.), arena_size=2., max_episode_length=5)
    with pytest.raises(ValueError, match='finite'):
        PointVecEnv(4)
    with pytest.raises(ValueError, match='finite'):
        PointVecEnv(4, max_episode_length=np.inf)
    with pytest.raises(ValueError, match='finite'):
        GridWorldVecEnv(4, '4x4')
    with pytest.raises(ValueError, match='unknown grid map'):
        GridWorldVecEnv(4, '5x5', max_episode_length=9)
    with pytest.raises(ValueError, match='one S cell'):
        GridWorldVecEnv(2, ['FFG', 'FHF'], max_episode_length=9)
    with pytest.raises(ValueError, match='unknown grid cells'):
        GridWorldVecEnv(2, ['SFZ'], max_episode_length=9)
    with pytest.raises(ValueError, match='shape'):
        GridWorldVecEnv(2, ['4x4', '8x8'], max_episode_length=9)
    with pytest.raises(ValueError, match='one map per env'):
        GridWorldVecEnv(3, ['4x4', '4x4'], max_episode_length=9)


def test_grid_maps_are_the_reference_maps(golden):
    g = golden('grid_env')
    for k in range(int(g['n_cases'])):
        rows = grid_rows(g, k)
        assert GridTwin(rows).reset()[0] == g['c%d_start' % k][0]
    from garage_amd.envs import GRID_MAPS
    assert sorted(GRID_MAPS) == ['4x4', '4x4_safe', '8x8', 'chain']
    assert GRID_MAPS['chain'][0].index('S') == 14


def test_new_ctypes_structs_match_the_header():
    from garage_amd import _lib
    structs = {'ga_point_env': _lib.PointEnv, 'ga_grid_env': _lib.GridEnv,
               'ga_env_ref': _lib.EnvRef}
    lines = ['#include <stddef.h>', '#include <stdio.h>',
             '#include "garage_amd.h"', 'int main(void) {',
             'printf("%d %d %d\\n", GA_ENV_SYNTH, GA_ENV_POINT, GA_ENV_GRID);']
    want = ['{} {} {}'.format(_lib.ENV_SYNTH, _lib.ENV_POINT, _lib.ENV_GRID)]
    for cname, py in structs.items():
        lines.append('printf("{0} %zu\\n", sizeof({0}));'.format(cname))
        want.append('{} {}'.format(cname, ctypes.sizeof(py)))
        for field, ftype in py._fields_:
            lines.append('printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), '
                         'sizeof((({0}*)0)->{1}));'.format(cname, field))
            want.append('{}.{} {} {}'.format(cname, field,
                                             getattr(py, field).offset,
                                             ctypes.sizeof(ftype)))
    lines += ['return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe],
                       check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == want


def test_new_entry_points_report_argument_errors_without_a_gpu():
    from garage_amd import _lib
    C = ctypes

    def ref(kind, env):
        return C.byref(_lib.env_ref(kind, env))

    p = _lib.PointEnv(n=4, max_episode_length=5)
    with pytest.raises(_lib.GarageAmdError, match='null env state'):
        _lib.call('ga_env_reset', ref(_lib.ENV_POINT, p), None, None, 4, None)
    with pytest.raises(_lib.GarageAmdError, match='null env state'):
        _lib.call('ga_env_step', ref(_lib.ENV_POINT, p), None, 2, None, None,
                  4, None, None, None)
    gr = _lib.GridEnv(n=4, rows=4, cols=4, max_episode_length=5)
    with pytest.raises(_lib.GarageAmdError, match='null env state'):
        _lib.call('ga_env_reset', ref(_lib.ENV_GRID, gr), None, None, 16,
                  None)
    with pytest.raises(_lib.GarageAmdError, match='null env state'):
        _lib.call('ga_env_step_record', ref(_lib.ENV_GRID, gr),
                  C.byref(_lib.RecordArgs()), None, None, 1, None, None)
    buf = C.create_string_buffer(64)
    addr = C.addressof(buf)
    p2 = _lib.PointEnv(n=4, max_episode_length=0, point=addr, goal=addr, t=addr)
    with pytest.raises(_lib.GarageAmdError, match='max_episode_length'):
        _lib.call('ga_env_step_record', ref(_lib.ENV_POINT, p2),
                  C.byref(_lib.RecordArgs()), None, None, 2, None, None)
    # the synthetic env through the same three entries
    def synth(**kw):
        e = _lib.SynthEnv(n=4, obs_dim=6, act_dim=3, min_len=2, max_len=5,
                          episode=addr, t=addr, len=addr)
        for k, v in kw.items():
            setattr(e, k, v)
        return ref(_lib.ENV_SYNTH, e)

    def reset(e, ldo=8):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=8):
        _lib.call('ga_env_step', e, addr, 4, addr, addr, ldo, addr, addr, None)

    def record(e, ldo=8):
        rec = _lib.RecordArgs(
            n=4, col=0, Tcap=8, max_episode_length=5, reward=addr,
            step_type=addr, next_obs=addr, ldo=ldo, obs_dim=6, ep_t=addr,
            rew_buf=addr, st_buf=addr, tail_buf=addr, lastobs_buf=addr,
            done=addr, step_eps=addr, step_samples=addr)
        _lib.call('ga_env_step_record', e, C.byref(rec), None, addr, 4, addr,
                  None)

    for fn in (reset, step, record):
        for field in ('episode', 't', 'len'):
            with pytest.raises(_lib.GarageAmdError, match='null env state'):
                fn(synth(**{field: None}))
        with pytest.raises(_lib.GarageAmdError,
                           match='1 <= min <= max <= 65535'):
            fn(synth(min_len=6))
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(synth(), ldo=5)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(synth(), ldo=5)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        record(synth(), ldo=5)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_env_step', synth(), addr, 4, None, addr, 8, addr, addr,
                  None)  # the synthetic env reads the current observations
    desc, head, rec = _lib.MlpDesc(), _lib.HeadArgs(), _lib.RecordArgs()
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call('ga_rollout_env_steps', C.byref(desc), None, C.byref(head),
                  None, C.byref(rec), None, None, None, None, None, 1, None)
    bad = _lib.EnvRef(kind=7, env=addr)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _lib.call('ga_rollout_env_steps', C.byref(desc), addr, C.byref(head),
                  C.byref(bad), C.byref(rec), addr, addr, None, None, None, 1,
                  None)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _lib.call('ga_env_reset', C.byref(bad), None, addr, 8, None)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _lib.call('ga_env_step', C.byref(bad), addr, 4, addr, addr, 8, addr,
                  addr, None)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _lib.call('ga_env_step_record', C.byref(bad), C.byref(rec), None,
                  addr, 4, addr, None)
    with pytest.raises(_lib.GarageAmdError, match='unknown env kind'):
        _lib.call('ga_policy_env_step_fused_f32', C.byref(desc), addr,
                  C.byref(head), C.byref(bad), C.byref(rec), None, 1, None)
    with pytest.raises(_lib.GarageAmdError, match='null env'):
        _lib.call('ga_env_reset', C.byref(_lib.EnvRef(kind=_lib.ENV_POINT)),
                  None, addr, 8, None)


@pytest.mark.ref
def test_fixtures_regenerate_identically_from_the_reference():
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.join(
            ROOT, 'tests', 'golden', 'make_golden_device_envs.py'), '--check',
                        tmp], check=True, capture_output=True,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
        for name in ('point_env', 'grid_env', 'point_sampler'):
            a = np.load(os.path.join(tmp, name + '.npz'))
            b = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
            assert sorted(a.files) == sorted(b.files), name
            for k in a.files:
                assert np.array_equal(a[k], b[k]), (name, k)


def test_env_rollout_loop_under_address_sanitizer():
    """``make asan-env-loop``: ga_rollout_env_steps' host loop compiled with
    ``-fsanitize=address,undefined`` against recording fakes of the kernels
    (tests/host/rollout_loop_harness.cpp, suite env-loop): argument errors, the one-launch
    rollout per env kind (the synthetic env included), the per-step buffer
    ping-pong and the action rescale."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-env-loop'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'all checks passed' in out.stdout
