"""``PopulationTRPO`` on 39-wide observations (the wide kernel of ``members_natural.hip``):
the two iterations of ``tests/test_population_trpo_gpu.py`` and every comparison it makes
with a lone ``TRPO`` -- exact candidate parameters, the acceptance rule, ``descent_step``
to 1e-3 -- with the three Gaussian members on a ``SyntheticVecEnv`` in the Pendulum's
place."""
import pytest

import test_population_trpo_gpu as narrow

pytestmark = pytest.mark.gpu


def test_two_iterations_end_to_end_at_39_inputs(monkeypatch):
    from garage_amd import _lib, envs
    monkeypatch.setattr(
        envs, 'PendulumVecEnv',
        lambda n_envs, max_episode_length, seed: envs.SyntheticVecEnv(
            n_envs, 39, 2, max_episode_length, seed=seed))
    lib = _lib.load()
    before = int(lib.ga_narrow_wide_launches())
    narrow.test_two_iterations_end_to_end('gaussian')
    # per iteration the gradient's pass, 10 + 1 products and a backtrack round at least,
    # beside the value functions' wide steps
    assert int(lib.ga_narrow_wide_launches()) - before >= 2 * 13
