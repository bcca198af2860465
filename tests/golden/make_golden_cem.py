"""Generate ``cem.npz`` by running the REAL reference ``garage.np.algos.CEM``.

Run in the build container only (needs the reference checkout that
``_ref_harness.py`` imports)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cem.py

The real ``CEM`` is driven for ``EPOCHS`` epochs by a flat-vector stub policy
and a stub trainer whose one-step episodes carry the reward
``-(||theta - theta*||^2)`` of the policy's current parameters: a continuous
function of the sample, so ``argsort`` meets no ties.  Written: every sampled
vector, ``_cur_mean`` / ``_cur_std`` after each epoch, the value each
``_train_once`` and ``train`` returned, and the keys each iteration logged, in
order (plain arrays only).  ``--check DIR`` writes into DIR instead.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_harness as ref  # noqa: E402

ref.install()

import akro  # noqa: E402
import garage._functions as gfun  # noqa: E402
import garage.np.algos.cem as cem_mod  # noqa: E402
from garage import EnvSpec, EpisodeBatch, StepType  # noqa: E402
from garage.np.algos import CEM  # noqa: E402

OUT = HERE

# the settings of tests/test_cem_cpu.py
N_SAMPLES, BEST_FRAC, EXTRA_DECAY, EPOCHS = 8, 0.25, 10, 3
N_PARAMS, EPISODES, SEED = 6, 2, 11
DISCOUNT, INIT_STD, EXTRA_STD = 0.99, 1, 1.


def theta_star():
    return np.linspace(-1.0, 1.5, N_PARAMS)


def theta_0():
    return 0.25 * np.cos(np.arange(N_PARAMS, dtype=np.float64))


def reward_of(theta):
    """The stub episodes' reward for the parameter vector ``theta``."""
    d = np.asarray(theta, dtype=np.float64) - theta_star()
    return -np.sum(d * d)


class KeyRecorder(ref.TabularRecorder):
    """``TabularRecorder`` that also keeps the order of the ``record`` calls."""

    def __init__(self):
        super().__init__()
        self.keys = []

    def record(self, key, val):
        super().record(key, val)
        self.keys.append(self._prefix + key)


class FlatPolicy:
    """What ``CEM`` needs of a flat-vector policy (``np/policies``)."""

    def __init__(self, theta):
        self._theta = np.array(theta, dtype=np.float64)

    def get_param_values(self):
        return self._theta.copy()

    def set_param_values(self, theta):
        self._theta = np.array(theta, dtype=np.float64)


def one_step_episodes(spec, reward):
    n = EPISODES
    return EpisodeBatch(
        env_spec=spec, episode_infos={},
        observations=np.zeros((n, 2), np.float32),
        last_observations=np.zeros((n, 2), np.float32),
        actions=np.zeros((n, 1), np.float32),
        rewards=np.full(n, reward, dtype=np.float64),
        env_infos={}, agent_infos={},
        step_types=np.asarray([StepType.TERMINAL] * n, dtype=StepType),
        lengths=np.ones(n, dtype='l'))


class StubTrainer:
    """``step_epochs`` / ``obtain_episodes`` / ``step_itr`` of ``garage.Trainer``."""

    def __init__(self, spec, policy, epochs):
        self._spec, self._policy, self._epochs = spec, policy, epochs
        self.step_itr = 0
        self.step_episode = None

    def step_epochs(self):
        for epoch in range(self._epochs):
            yield epoch

    def obtain_episodes(self, itr):
        del itr
        return one_step_episodes(self._spec,
                                 reward_of(self._policy.get_param_values()))


def gen_cem():
    spec = EnvSpec(akro.Box(-1, 1, (2, )), akro.Box(-1, 1, (1, )),
                   max_episode_length=1)
    policy = FlatPolicy(theta_0())
    algo = CEM(spec, policy, None, N_SAMPLES, discount=DISCOUNT,
               init_std=INIT_STD, best_frac=BEST_FRAC, extra_std=EXTRA_STD,
               extra_decay_time=EXTRA_DECAY)
    rec = KeyRecorder()
    cem_mod.tabular = rec
    gfun.tabular = rec
    trainer = StubTrainer(spec, policy, EPOCHS)
    evaluated, returned, keys, means, stds = [], [], [], [], []
    real_train_once = algo._train_once

    def train_once(itr, episodes):
        evaluated.append(policy.get_param_values())
        rec.keys = []
        rtn = real_train_once(itr, episodes)
        returned.append(rtn)
        keys.append(list(rec.keys))
        if (itr + 1) % N_SAMPLES == 0:
            means.append(np.array(algo._cur_mean))
            stds.append(np.array(algo._cur_std))
        return rtn

    algo._train_once = train_once
    np.random.seed(SEED)
    last = algo.train(trainer)
    out = dict(
        theta_star=theta_star(), theta_0=theta_0(),
        # (EPOCHS * N_SAMPLES, P): the vector each iteration evaluated
        evaluated=np.asarray(evaluated),
        # the first candidate of the epoch after the last one
        next_candidate=np.asarray(algo._cur_params),
        cur_mean=np.asarray(means), cur_std=np.asarray(stds),
        returned=np.asarray(returned, dtype=np.float64),
        train_returned=np.float64(last),
        keys=np.asarray(['\n'.join(k) for k in keys]),
        settings=np.asarray([N_SAMPLES, BEST_FRAC, EXTRA_DECAY, EPOCHS,
                             N_PARAMS, EPISODES, SEED, DISCOUNT, INIT_STD,
                             EXTRA_STD], dtype=np.float64))
    path = os.path.join(OUT, 'cem.npz')
    np.savez_compressed(path, **out)
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--check':
        OUT = sys.argv[2]
    gen_cem()
