"""The frame the five seeded state-vector env kinds share on the device
(``rollout_dev.h``: ``StateEnv<K>`` -- counters, step type, store order) at the
sizes around the env kernels' 256-thread block, one row of
``_state_env_kinds.KINDS`` per kind.

Each case allocates three members more than the kernels are told of and poisons
those guard rows, runs ``ga_env_step`` with a masked ``ga_env_reset`` of the
ended members after every step, and compares every value the frame stores, bit
for bit, with one host twin object per member driven through its own
``reset`` / ``step``.  The members start their first episode at different step
counts, so every step ends a third of them and every masked reset has set and
clear flags on both sides of a block boundary.
"""
import numpy as np
import pytest
import torch

import _state_env_kinds as kinds
from _state_env_helpers import GUARD, _bits, _guards_intact, _np, _poison

pytestmark = pytest.mark.gpu

P, STEPS = 3, 6  # max_episode_length, steps per case
SEED, ID0 = 11, 1000


def _frame_equals_twins(env, twins, n, obs, where):
    """What the frame keeps of members 0 .. n - 1 against the twins' own, and
    the guard rows."""
    O = env.obs_dim
    assert np.array_equal(_bits(_np(env.obs)[:n, :O]), _bits(obs)), where
    assert (_np(env.obs)[:n, O:] == 0).all(), where
    assert np.array_equal(_bits(env.get_state()[:n]),
                          _bits(np.stack([tw.state for tw in twins]))), where
    assert np.array_equal(_np(env._t)[:n], [tw._t for tw in twins]), where
    assert np.array_equal(_np(env._resets)[:n],
                          [tw.resets for tw in twins]), where
    _guards_intact(env, n)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
@pytest.mark.parametrize('kind', sorted(kinds.KINDS))
def test_frame_equals_one_twin_per_member_bit_for_bit(kind, n):
    row = kinds.KINDS[kind]
    env = row.new_batch(n + GUARD, max_episode_length=P, seed=SEED,
                        env_id0=ID0)
    twins = [row.new_twin(seed=SEED, env_id=ID0 + i, max_episode_length=P)
             for i in range(n)]
    O = env.obs_dim
    env._c.n = n  # the kernels' batch; rows n .. n + 2 are guards
    _poison(env, n)
    env.reset_all()
    obs = np.stack([tw.reset()[0] for tw in twins])
    # member i has taken i % P steps of its first episode already
    env._t[:n] = torch.arange(n, dtype=torch.int32, device=env.device) % P
    for i, tw in enumerate(twins):
        tw._t = i % P
    _frame_equals_twins(env, twins, n, obs, 'reset_all')

    actions = row.frame_actions(np.random.RandomState(5 + n),
                                (STEPS, n)).astype(np.float32)
    act = torch.zeros(n + GUARD, 4, device=env.device)
    ends = 0
    for t in range(STEPS):
        act[:n, 0] = torch.from_numpy(actions[t])
        env.step_all(act)
        steps = [tw.step(actions[t, i]) for i, tw in enumerate(twins)]
        obs = np.stack([es.observation for es in steps])
        types = np.array([int(es.step_type) for es in steps])
        assert np.array_equal(_bits(_np(env.next_obs)[:n, :O]), _bits(obs)), t
        assert np.array_equal(_bits(_np(env.reward)[:n]),
                              _bits([es.reward for es in steps])), t
        assert np.array_equal(_np(env.step_type)[:n], types), t
        # TIMEOUT exactly where the member's P-th step is, whatever `done` says
        due = np.array([tw._t for tw in twins]) == P
        assert np.array_equal(types == 3, due), t
        # the ended members are reset, the others keep state and observation
        ended = types >= 2
        ends += int(ended.sum())
        flags = np.ones(n + GUARD, dtype=np.uint8)  # (guard flags: not read)
        flags[:n] = ended
        env.advance()
        env.hold()
        env.reset_where(torch.from_numpy(flags).to(env.device))
        env.advance()
        for i in np.nonzero(ended)[0]:
            obs[i] = twins[i].reset()[0]
        _frame_equals_twins(env, twins, n, obs, t)
    # every member finished two episodes; two thirds of them began a third
    assert ends >= 2 * n
