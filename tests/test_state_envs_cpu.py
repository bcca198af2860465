"""The seeded state-vector env kinds, what every kind states about itself and
needs no GPU, one case per row of ``_state_env_kinds.KINDS``: the Philox reset
draws against a pure-Python Philox4x32-10, the ctypes mirror of the kind's C
struct against the header, the argument errors of the entry points, and whether
``ga_rollout_env_steps`` takes the kind as discrete or continuous.  (MountainCar
is one kind with one struct: where the variants cannot differ only the
``mountain_car`` row is listed.)"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _state_env_helpers as h
import _state_env_kinds as kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@kinds.rows('cartpole', 'pendulum', 'double_pendulum', 'acrobot',
            'mountain_car', 'mountain_car_continuous')
def test_reset_draws_equal_a_pure_python_philox(row):
    cases, draws = row.draw_cases(), []
    for seed, env_id, counter in cases:
        got = row.reset_draw(seed, env_id, counter)
        want = h.reset_draw_py(row, seed, env_id, counter)
        assert got.dtype == np.float32 and got.shape == (row.state_dim, )
        assert got.tobytes() == want.tobytes(), (seed, env_id, counter)
        row.check_draw(got)
        draws.append(got)
    row.check_draws(row, cases, draws)
    # the twin starts its episodes there, and the counter advances
    for i in (0, 3, 69):
        env = row.new_twin(seed=5, env_id=37 + i)
        first, info = env.reset()
        assert info == {} and first.dtype == np.float32
        assert np.array_equal(env.state, row.reset_draw(5, 37 + i, 0))
        assert first.tobytes() == row.observe(env.state).tobytes()
        env.reset()
        assert np.array_equal(env.state, row.reset_draw(5, 37 + i, 1))


@kinds.rows('cartpole', 'pendulum', 'double_pendulum', 'acrobot',
            'mountain_car')
def test_ctypes_struct_matches_the_header(row):
    from garage_amd import _lib
    lines, want = h._layout_lines(row.cname, row.struct, row.kind_macro)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['cc', '-std=c99', '-Wall', '-Werror', '-I',
                        os.path.join(ROOT, 'include'), src, '-o', exe],
                       check=True)
        got = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split('\n')[:-1]
    assert got == ['{}'.format(row.kind_code)] + want
    assert row.kind_code == row.kind_number
    row.check_struct()
    assert _lib.load().ga_abi_version() == 5


def _struct(row, addr, **kw):
    fields = dict(n=4, max_episode_length=5, state=addr, t=addr, resets=addr)
    return row.struct(**{**fields, **row.struct_kw, **kw})


@kinds.rows('cartpole', 'pendulum', 'double_pendulum', 'acrobot',
            'mountain_car')
def test_argument_errors_without_a_gpu(row):
    from garage_amd import _lib
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)
    narrow = row.obs_dim - 1  # observation rows narrower than the kind's

    def env(kind=row.kind_code, **kw):
        return C.byref(_lib.env_ref(kind, _struct(row, addr, **kw)))

    def reset(e, ldo=row.ldo):
        _lib.call('ga_env_reset', e, None, addr, ldo, None)

    def step(e, ldo=row.ldo):
        _lib.call('ga_env_step', e, addr, 1, None, addr, ldo, addr, addr, None)

    def record(e, ldo=row.ldo):
        rec = _lib.RecordArgs(n=4, col=0, Tcap=8, max_episode_length=5,
                              reward=addr, step_type=addr, next_obs=addr,
                              ldo=ldo, obs_dim=row.obs_dim, ep_t=addr,
                              rew_buf=addr, st_buf=addr, tail_buf=addr,
                              lastobs_buf=addr, done=addr, step_eps=addr,
                              step_samples=addr)
        _lib.call('ga_env_step_record', e, C.byref(rec), None, addr, 1, addr,
                  None)

    for fn in (reset, step, record):
        for field in ('state', 't', 'resets'):
            with pytest.raises(_lib.GarageAmdError, match='null env state'):
                fn(env(**{field: None}))
        for bad in (0, 65536):
            with pytest.raises(_lib.GarageAmdError,
                               match='max_episode_length'):
                fn(env(max_episode_length=bad))
        with pytest.raises(_lib.GarageAmdError, match='bad env size'):
            fn(env(n=0))
        for fields, match in row.struct_errors:
            with pytest.raises(_lib.GarageAmdError, match=match):
                fn(env(**fields))
        for unknown in row.unknown_kinds:
            with pytest.raises(_lib.GarageAmdError,
                               match='unknown env kind {}'.format(unknown)):
                fn(env(kind=unknown))
    with pytest.raises(_lib.GarageAmdError, match='bad obs buffer'):
        reset(env(), ldo=narrow)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        step(env(), ldo=narrow)
    with pytest.raises(_lib.GarageAmdError, match='leading dimensions'):
        record(env(), ldo=narrow)
    with pytest.raises(_lib.GarageAmdError, match='null pointer'):
        _lib.call(row.draw_entry, 0, 0, 0, None)
    for bad in row.bad_lengths:
        for variant in kinds.variants(row):
            with pytest.raises(ValueError):
                variant.new_batch(4, max_episode_length=bad)
            with pytest.raises(ValueError):
                variant.new_twin(max_episode_length=bad)


@kinds.rows('cartpole', 'pendulum', 'double_pendulum', 'acrobot',
            'mountain_car', 'mountain_car_continuous')
def test_rollout_env_steps_asks_whether_the_kind_is_discrete(row):
    """With rescale arguments a discrete kind fails the "continuous action
    space" check; a continuous one passes it and fails the next one (a rollout
    of more steps than the buffer holds); an unknown kind code is refused --
    all before any device call.  MountainCar's struct says which it is."""
    from garage_amd import _lib
    C = ctypes
    buf = C.create_string_buffer(256)
    addr = C.addressof(buf)
    desc = _lib.MlpDesc()
    head = _lib.HeadArgs(col=0, Tcap=4)
    rec = _lib.RecordArgs()
    norm = _lib.NormArgs(act_low=addr, act_high=addr, scaled_action=addr,
                         expected_action_scale=1.0, reward_scale=1.0)

    def steps(kind):
        ref = _lib.env_ref(kind, _struct(row, addr))
        _lib.call('ga_rollout_env_steps', C.byref(desc), addr, C.byref(head),
                  C.byref(ref), C.byref(rec), addr, addr, C.byref(norm), None,
                  None, 5, None)

    refused = ('continuous action space' if row.discrete else
               'steps exceed the rollout buffer')
    with pytest.raises(_lib.GarageAmdError, match=refused):
        steps(row.kind_code)
    for unknown in row.unknown_kinds:
        with pytest.raises(_lib.GarageAmdError,
                           match='unknown env kind {}'.format(unknown)):
            steps(unknown)
