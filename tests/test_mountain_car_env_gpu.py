"""``MountainCarVecEnv`` on the GPU, both variants: the procedures it shares
with the other seeded state-vector kinds (``_state_env_bodies.py``, on the rows
``MOUNTAIN_CAR`` and ``MOUNTAIN_CAR_CONTINUOUS`` of ``_state_env_kinds.py``)
and ``NormalizedVecEnv`` around either variant (statistics inside the launch
for the classes, the force rescale on the per-step path)."""
import numpy as np
import pytest
import torch

import _state_env_bodies as bodies
import _state_env_helpers as h
import _state_env_kinds as kinds
from _state_env_helpers import TIMEOUT, _bits, _np, _same
from _state_env_kinds import MOUNTAIN_CAR, MOUNTAIN_CAR_CONTINUOUS

pytestmark = pytest.mark.gpu
P = MOUNTAIN_CAR.P


# the shared procedures, for either variant
VARIANTS = pytest.mark.parametrize(
    'row', [MOUNTAIN_CAR, MOUNTAIN_CAR_CONTINUOUS],
    ids=['discrete', 'continuous'])


@VARIANTS
@pytest.mark.parametrize('P', [1, 2, 7, 1000])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 65])
def test_reset_and_step_kernels_equal_the_twin_bit_for_bit(n, P, row):
    bodies.reset_and_step_kernels_equal_the_twin_bit_for_bit(row, n, P)


@VARIANTS
def test_one_step_from_the_whole_state_box_equals_the_twin(row):
    bodies.one_step_from_the_whole_state_box_equals_the_twin(row)


@VARIANTS
@kinds.cases(MOUNTAIN_CAR)
def test_one_launch_rollout_equals_python_driven_steps(case, row):
    bodies.one_launch_rollout_equals_python_driven_steps(row, case)


@VARIANTS
def test_one_launch_rollout_replays_on_the_host_twin(row):
    bodies.one_launch_rollout_replays_on_the_host_twin(row)


@VARIANTS
def test_device_batch_equals_a_host_batch_of_the_twins(row):
    bodies.device_batch_equals_a_host_batch_of_the_twins(row)


@VARIANTS
def test_pickled_sampler_continues_identically(row):
    bodies.pickled_sampler_continues_identically(row)


@VARIANTS
def test_fragment_worker_fragments_join_up(row):
    bodies.fragment_worker_fragments_join_up(row)


@VARIANTS
def test_population_members_equal_lone_workers_and_their_statistics(row):
    bodies.population_members_equal_lone_workers_and_their_statistics(row)


def test_normalized_mountain_car_statistics_inside_the_launch():
    """``NormalizedVecEnv(normalize_obs, normalize_reward)`` around the
    discrete variant: no rescale, so each call's first steps stay one launch;
    native against Python-driven steps, two calls in a row."""
    n = 70
    for a in h.normalized_statistics_inside_the_launch(
            MOUNTAIN_CAR, n, (n * 2 * P, n * 2 * P + 17)):
        assert np.isfinite(a.rewards).all()
        assert len(np.unique(a.rewards)) > 5  # normalised: no longer all -1


def test_normalized_continuous_car_rescales_the_force():
    """``NormalizedVecEnv(normalize_obs)`` around the continuous variant: the
    force bounds are finite, so the policy's actions are rescaled (and so
    clipped) to them in a launch of their own and the rollout takes per-step
    launches; native against Python-driven steps, two calls in a row.  The car
    is stepped with, and charged for, the rescaled force."""
    from garage_amd.envs import MountainCarEnv
    n = 40
    wrap = h.normalized(normalize_obs=True, obs_alpha=0.05)

    out = []
    for native in (True, False):
        s, w = h.make(MOUNTAIN_CAR_CONTINUOUS, (64, 64), n=n, native=native,
                      wrap=wrap)
        assert w.env._act_low is not None and w._fused_ok()
        out.append([s.obtain_samples(itr, num, None).to_host()
                    for itr, num in enumerate((n * 2 * P, n * 2 * P + 17))])
    for a, b in zip(*out):
        _same(a, b)
        assert np.isfinite(a.observations).all()
        types_, ends = h._ends(a)
        assert set(types_[ends].tolist()) == {TIMEOUT}
        f = np.float32
        acts = np.asarray(a.actions, dtype=f)[:, 0]
        assert np.abs(acts).max() > 1
        pushes = h.rescaled(acts, -1.0, 1.0)
        assert np.array_equal(_bits(a.rewards),
                              _bits(f(0) - f(0.1) * (pushes * pushes)))
    k = 3
    for native in (True, False):
        s, w = h.make(MOUNTAIN_CAR_CONTINUOUS, (64, 64), n=n, native=native,
                      wrap=wrap)
        w._start()
        b = w._alloc_buffers(n * P)
        if native:
            assert w._native_steps(b, 0, k)
        else:
            for col in range(k):
                w._step(b, col)
        torch.cuda.synchronize()
        assert (_np(w.env._env._resets) == 1).all()
        policy_actions = _np(b['act'])[:, :k, 0]
        pushes = h.rescaled(policy_actions, -1.0, 1.0)
        assert (np.abs(pushes) <= 1).all()
        state = h.draws(MOUNTAIN_CAR_CONTINUOUS, 21, 3, n)
        for t in range(k):
            state, _, _, done = MountainCarEnv.advance(state, pushes[:, t],
                                                       True)
            assert not done.any()
        assert np.array_equal(_bits(w.env._env.get_state()), _bits(state))
