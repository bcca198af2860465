"""The seeded state-vector env kinds as the tests see them: one ``Kind`` record
per row of ``KINDS`` -- what ``_state_env_bodies.py``,
``test_state_env_frame_gpu.py`` and ``test_state_envs_cpu.py`` need to run one
body for every kind.

A row names its classes (looked up in ``garage_amd.envs`` when first used, so
importing this module needs no library), states its shapes, seeds and scripted
material, and holds, as callables, the assertions that only make sense for its
kind: the invariants after a kernel step, what a whole rollout must look like,
what the population's returns must equal.  A shared body never asks which kind
it runs; a row takes part in a GPU procedure where its
``test_<kind>_env_gpu.py`` calls the body, and in a CPU one where the test
lists it.

A new kind adds one row here next to its dynamics and its physics tests, calls
the bodies that hold for it from its own GPU file, and puts its name into the
lists of ``test_state_envs_cpu.py``."""
import numpy as np
import pytest

import _state_env_helpers as h

TERMINAL, TIMEOUT = h.TERMINAL, h.TIMEOUT
F = np.float32

# the network cases of the one-launch rollout test: (id, hidden, options,
# launches of kinds (13, 14))
_RELU_LN = 'relu-ln'  # hidden_nonlinearity=torch.relu, layer_normalization
CASES_3 = [('a-tanh-resident', (64, 64), None, (1, 0)),
           ('b-relu-ln-resident', (64, 64), _RELU_LN, (1, 0)),
           ('c-four-layers-streamed', (32, 32, 32), None, (0, 0))]
CASES_4 = CASES_3 + [('d-320-wide', (320, ), None, (0, 1))]
CASES_5 = CASES_3 + [('d-320-320-streamed-wide', (320, 320), None, (0, 1)),
                     ('e-512-wide', (512, ), None, (0, 1))]


def options_of(case_options):
    import torch
    if case_options == _RELU_LN:
        return dict(hidden_nonlinearity=torch.relu, layer_normalization=True)
    return case_options


class Kind:
    """One row.  Defaults are for a kind with nothing scripted.

    Every row states:
      name; batch, twin, draw (names in ``garage_amd.envs``) and ``kw``;
      struct_name, kind_macro, kind_number, cname, draw_entry, ldo (the C
        struct, its kind code, the reset-draw entry, a valid leading dimension);
      obs_dim, state_dim, discrete (the action is a class index);
      stream, draw_blocks, draw_from_words, draw_cases, check_draw, check_draws
        (the reset draw restated, and what the draws must satisfy);
      unknown_kinds, struct_errors, bad_lengths (what the entry points refuse);
      frame_actions (the action draw of the frame test);
      N, P, NUM, rollout_policy_kw, rollout_cases, check_rollout,
        replay_resets, replay_action, check_replay, check_host_call,
        check_pickled, pickle_min_resets, SCRIPTED, near_end (the rollouts).
    A row of the kernel tests adds kernel_steps, kernel_twins, kernel_actions,
    edge_states, hold, check_spec, bad_states (rejected ``set_state`` inputs
    with the error text), check_step, check_kernel_tally, timeout_seen; of the
    whole-box test, advance and box_sample; of the fragment test,
    fragment_endings; of the population test, POP_*, DISCOUNT, pop_policy_kw,
    pop_scale, pop_log_std, pop_starts, pop_actions_head and check_pop_member /
    _stats / _final; of the CEM test, check_cem_episodes / _final."""
    kw = {}                  # constructor keywords of the batch and the twin
    rollout_policy_kw = {}   # ... of the rollout tests' policy
    SCRIPTED = 0             # members that start one step from an episode end
    near_end = None          # count -> that many such states
    pop_starts = None        # (row, n, env_id0) -> the population's first states
    pop_log_std = None       # (first, step) of the members' log-std
    pop_actions_head = 50    # how many actions of members 0 and 1 must differ
    replay_resets = 24       # reset counters the replay looks up per member
    pickle_min_resets = 3    # every member was reset this often by call 0
    draw_blocks = 1          # Philox blocks of a reset draw
    struct_kw = {}           # fields of the C struct besides the frame's
    struct_errors = ()       # (fields, error text) the entry points refuse
    # max_episode_length values the constructors refuse
    bad_lengths = (None, float('inf'), 0, 65536)
    # what the struct's layout must satisfy besides equalling the header's
    check_struct = staticmethod(lambda: None)
    # what a call's batch of the host-batch test must hold besides equality
    check_host_call = staticmethod(lambda eps: None)
    # what the unpickled env must keep besides state and counters
    check_pickled = staticmethod(lambda ea, eb: None)

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return self.name

    def _env(self, name):
        from garage_amd import envs
        return getattr(envs, name)

    def new_batch(self, n, **kw):
        return self._env(self.batch)(n, **kw, **self.kw)

    def new_twin(self, **kw):
        return self._env(self.twin)(**kw, **self.kw)

    @property
    def twin_cls(self):
        return self._env(self.twin)

    def reset_draw(self, seed, env_id, counter):
        return self._env(self.draw)(seed, env_id, counter)

    def observe(self, states):
        return self.twin_cls.observe(np.asarray(states, dtype=F))

    def policy(self, spec, **kw):
        from garage_amd import policies
        name = ('CategoricalMLPPolicy' if self.discrete else
                'GaussianMLPPolicy')
        return getattr(policies, name)(spec, **kw)

    @property
    def struct(self):
        from garage_amd import _lib
        return getattr(_lib, self.struct_name)

    @property
    def kind_code(self):
        from garage_amd import _lib
        return getattr(_lib, self.kind_macro[3:])  # GA_ENV_X -> ENV_X


# -- what rollouts of several kinds have in common ----------------------------
def _ends_both_ways(row, whole):
    """Episodes end both ways inside the launch's 24 steps, resets follow."""
    types_, ends = h._ends(whole)
    assert int(whole.lengths.sum()) >= row.NUM
    assert whole.lengths.max() <= row.P
    assert set(types_[ends].tolist()) == {TERMINAL, TIMEOUT}
    assert len(whole.lengths) >= 3 * row.N
    assert (np.delete(types_, ends) < 2).all()
    assert (whole.lengths[types_[ends] == TIMEOUT] == row.P).all()
    return types_, ends


def _inside_the_box(whole, env):
    box = env.spec.observation_space
    assert (whole.observations >= box.low).all()
    assert (whole.observations <= box.high).all()


def _raises_under_normalize(row):
    """normalize() rescales a bounded action: the population launch has no
    rescale."""
    from garage_amd.envs import NormalizedVecEnv
    from garage_amd.sampler import GpuPopulationSampler
    n = row.POP_M * row.POP_G
    gpol = pop_policy(row, pop_env(row, n).spec)
    with pytest.raises(ValueError, match='rescales actions'):
        GpuPopulationSampler(gpol, NormalizedVecEnv(pop_env(row, n)),
                             n_members=row.POP_M,
                             max_episode_length=row.POP_P, seed=row.POP_SEED)


def pop_env(row, n, env_id0=0):
    return row.new_batch(n, max_episode_length=row.POP_P, seed=3,
                         env_id0=env_id0)


def pop_policy(row, spec):
    return row.policy(spec, hidden_sizes=(8, 8), **row.pop_policy_kw)


def _log_std_is_the_members(got, vector):
    assert np.all(got.agent_infos['log_std'] == F(vector[0]))


def _distinct_rewards(st, host, lengths, term):
    # the sums really ran over distinct, non-integer rewards
    assert len(np.unique(host.rewards)) > len(host.rewards) // 2


def _first_differ_and_all_distinct(row, cases, draws):
    # another env id or another counter: another state
    assert not np.array_equal(draws[0], draws[1])
    assert not np.array_equal(draws[0], draws[2])
    assert len({d.tobytes() for d in draws}) == len(draws)


def _grid_distinct_and_high_word(row, cases, draws):
    # another seed, env id or counter: another state
    assert len({d.tobytes() for d in draws}) == len(draws) == 18
    # the key's high word counts
    at = cases.index(((7 << 32) | 11, 1, 1))
    assert row.reset_draw(11, 1, 1).tobytes() != draws[at].tobytes()


def _within_a_tenth(got):
    assert (np.abs(got) <= np.float32(0.1)).all()


# -- cartpole -----------------------------------------------------------------
def _cartpole_draw(got):
    assert ((got > -0.05) & (got < 0.05)).all()


def _cartpole_draws(row, cases, draws):
    from garage_amd.envs import CartPoleEnv, cartpole_reset_draw
    _first_differ_and_all_distinct(row, cases, draws)
    # roughly uniform over the interval
    flat = np.concatenate(draws)
    assert abs(flat.mean()) < 0.005 and flat.min() < -0.045 < 0.045 < flat.max()
    # env_id0 shifts the stream: member i of a batch with env_id0 = k is member
    # i + k of a batch with env_id0 = 0 (the batch draws env_id0 + i)
    k = 37
    for i in (0, 3, 69):
        a = CartPoleEnv(seed=5, env_id=k + i)
        b = CartPoleEnv(seed=5, env_id=i)
        first, _ = a.reset()
        assert np.array_equal(first, cartpole_reset_draw(5, i + k, 0))
        assert not np.array_equal(first, b.reset()[0])
        # the counter advances with every reset
        assert np.array_equal(a.reset()[0], cartpole_reset_draw(5, i + k, 1))


def _cartpole_rollout(row, whole, env):
    assert int(whole.lengths.sum()) >= row.NUM and whole.lengths.max() <= 30
    assert np.isfinite(whole.agent_infos['prob']).all()
    assert set(np.unique(whole.actions)) == {0.0, 1.0}
    # both endings occur (the reset inside the launch is exercised)
    assert h._ending_types(whole) == {2, 3}


def _cartpole_replay(row, whole, counters, order):
    assert len(counters) == row.N  # every member finished an episode


CARTPOLE = Kind(
    name='cartpole', batch='CartPoleVecEnv', twin='CartPoleEnv',
    draw='cartpole_reset_draw', struct_name='CartPoleEnv',
    kind_macro='GA_ENV_CARTPOLE', draw_entry='ga_cartpole_reset_draw',
    obs_dim=4, state_dim=4, discrete=True,
    frame_actions=lambda rng, shape: rng.randint(0, 2, shape),
    N=48, P=30, NUM=3 * 48 * 30 // 2, rollout_cases=CASES_3,
    check_rollout=_cartpole_rollout,
    replay_resets=3 * 48 * 30 // 2 // 48,  # more than a member can have
    replay_action=lambda a: int(a.reshape(-1)[0]),
    check_replay=_cartpole_replay,
    pickle_min_resets=1,
    stream=5, draw_cases=h.random_draw_cases,
    draw_from_words=lambda w: [F(-0.05) + F(0.1) * h.unit(x) for x in w],
    check_draw=_cartpole_draw, check_draws=_cartpole_draws,
    cname='ga_cartpole_env', kind_number=4, ldo=4, unknown_kinds=(),
)


# -- pendulum -----------------------------------------------------------------
def _pendulum_rollout(row, whole, env):
    # never done: every episode runs its P steps and ends in a TIMEOUT
    assert len(whole.lengths) == 3 * row.N and (whole.lengths == row.P).all()
    assert h._ending_types(whole) == {TIMEOUT}
    assert (np.asarray([int(s) for s in whole.step_types]) != 2).all()
    assert np.isfinite(whole.agent_infos['mean']).all()
    assert np.isfinite(whole.observations).all()
    # the batch keeps the policy's own actions, not the clipped torques
    assert np.abs(whole.actions).max() > 2
    assert (whole.rewards <= 0).all()
    assert len(np.unique(whole.rewards)) > row.NUM // 2


def _pendulum_replay(row, whole, counters, order):
    # every step that closes an episode is a TIMEOUT
    assert (np.asarray([int(s) for s in whole.step_types]) != TERMINAL).all()
    assert counters == {i: 2 for i in range(row.N)}
    # the batch is sorted by (completion step, member): all end together
    assert order == list(range(row.N)) * 3


def _pendulum_pop_member(row, got, vector):
    assert (got.lengths == row.POP_P).all()
    _log_std_is_the_members(got, vector)


def _pendulum_pop_stats(st, host, lengths, term):
    assert not st.terminated.any()
    assert not term.any()
    _distinct_rewards(st, host, lengths, term)
    assert len(np.unique(st.undiscounted_returns)) == len(lengths)


def _pendulum_pop_final(row, stats, terminated, returns):
    _raises_under_normalize(row)


def _pendulum_cem_episodes(episodes, length, tally):
    assert (np.asarray(episodes.lengths) == length).all()


def _pendulum_cem_final(returned, length, tally):
    assert np.isfinite(returned).all() and (returned < 0).all()
    assert len(np.unique(returned)) > 1


def _pendulum_words(w):
    return [(-F(3.141592653589793)) + F(6.283185307179586) * h.unit(w[0]),
            F(-1.0) + F(2.0) * h.unit(w[1])]


def _pendulum_draw(got):
    from garage_amd.envs import PendulumEnv
    assert abs(got[0]) <= PendulumEnv.PI and abs(got[1]) < 1


def _pendulum_draws(row, cases, draws):
    from garage_amd.envs import PendulumEnv, pendulum_reset_draw
    _first_differ_and_all_distinct(row, cases, draws)
    # the key's high word counts
    assert cases[3] == ((7 << 32) | 11, 5, 3)
    assert not np.array_equal(pendulum_reset_draw(11, 5, 3), draws[3])
    # roughly uniform over the two intervals
    d = np.stack(draws)
    assert abs(d[:, 0].mean()) < 0.3 and d[:, 0].min() < -2.8 < 2.8 < d[:, 0].max()
    assert abs(d[:, 1].mean()) < 0.1 and d[:, 1].min() < -0.9 < 0.9 < d[:, 1].max()
    # the twin's first observation, restated
    for i in (0, 3, 69):
        a = PendulumEnv(seed=5, env_id=37 + i)
        first, _ = a.reset()
        sn, cs = PendulumEnv.sincos(a.state[0])
        assert first.tobytes() == np.array([cs, sn, a.state[1]],
                                           np.float32).tobytes()


PENDULUM = Kind(
    name='pendulum', batch='PendulumVecEnv', twin='PendulumEnv',
    draw='pendulum_reset_draw', struct_name='PendulumEnv',
    kind_macro='GA_ENV_PENDULUM', draw_entry='ga_pendulum_reset_draw',
    obs_dim=3, state_dim=2, discrete=False,
    frame_actions=lambda rng, shape: rng.uniform(-2.5, 2.5, shape),
    # 48 envs are three workgroups of 16; 2.5 n P samples: three episodes per
    # env, two resets in the launch
    N=48, P=30, NUM=5 * 48 * 30 // 2, rollout_cases=CASES_4,
    check_rollout=_pendulum_rollout,
    replay_resets=4,  # more resets than a member has in this batch
    replay_action=lambda a: a, check_replay=_pendulum_replay,
    POP_SEED=5, POP_M=3, POP_G=16, POP_P=12, POP_NUM=40, DISCOUNT=0.99,
    pop_policy_kw=dict(learn_std=True), pop_scale=0.5, pop_log_std=(0.5, 0.3),
    pop_actions_head=None,
    check_pop_member=_pendulum_pop_member, check_pop_stats=_pendulum_pop_stats,
    check_pop_final=_pendulum_pop_final,
    check_cem_episodes=_pendulum_cem_episodes,
    check_cem_final=_pendulum_cem_final,
    stream=6, draw_cases=h.random_draw_cases, draw_from_words=_pendulum_words,
    check_draw=_pendulum_draw, check_draws=_pendulum_draws,
    cname='ga_pendulum_env', kind_number=5, ldo=4, unknown_kinds=(7, ),
)


# -- double pendulum ----------------------------------------------------------
def _tip_threshold_states():
    """Three states ``(0, th, th + d, 0, 0, 0)`` whose step under zero action
    ends with ``y_tip`` exactly 1, one ulp below and one ulp above (found on
    the twin, among consecutive float32 angles around the crossing, for a few
    offsets ``d``: one family alone skips some values of the sum)."""
    from garage_amd.envs import DoublePendulumEnv
    f = np.float32

    def y_after(th, d):
        st = np.zeros((len(th), 6), dtype=f)
        st[:, 1], st[:, 2] = th, th + f(d)
        new, _, _, done = DoublePendulumEnv.advance(st, np.zeros(len(th), f))
        return DoublePendulumEnv._trig(new[:, 1], new[:, 2])[5], done, st

    wants = (f(1.0), np.nextafter(f(1.0), f(0)), np.nextafter(f(1.0), f(2)))
    found = {}
    for d in (0.0, 0.013, -0.027, 0.041):
        coarse = np.linspace(0.2, 0.7, 4001).astype(f)
        y, _, _ = y_after(coarse, d)
        k = int(np.nonzero(y <= 1)[0][0])
        lo = coarse[k - 1]
        span = int((coarse[k].view(np.uint32) - lo.view(np.uint32))) + 1
        th = (lo.view(np.uint32) + np.arange(span, dtype=np.uint32)).view(f)
        y, done, st = y_after(th, d)
        for want in wants:
            hit = np.nonzero(y == want)[0]
            if len(hit) and want.tobytes() not in found:
                assert bool(done[hit[0]]) == bool(want <= 1)
                found[want.tobytes()] = tuple(st[hit[0]])
    assert len(found) == 3, len(found)
    return [found[w.tobytes()] for w in wants]


def _double_pendulum_edge_states():
    """Scripted starts and their first actions: the wraps of both angles either
    way, the +-100 speed guard, every +-10 clip of the observation, y_tip
    within one ulp of 1, the folds of sincos, the fixed point, a fallen one."""
    from garage_amd.envs import PendulumEnv
    f = np.float32
    pi, half = PendulumEnv.PI, PendulumEnv.HALF_PI
    rows = [((0, pi, -pi, 0, 5, -5), 0.5),
            ((0, -pi, pi, 0, -5, 5), -0.5),
            ((0, np.nextafter(pi, f(0)), 0.1, 0, 3, 0), 0.0),
            ((0, 0.3, -0.2, 99.99, 99.99, -99.99), 1.6),
            ((0, 0.3, -0.2, -99.99, -99.99, 99.99), -1.6),
            ((0.5, 0.1, 0.1, 11, -11, 4), 1.0),
            ((-0.5, -0.1, 0.1, -11, 11, -4), -1.0)]
    rows += [(s, 0.0) for s in _tip_threshold_states()]
    rows += [((0, half, -half, 0, 0, 0), 0.3),
             ((0, 0, 0, 0, 0, 0), 0.0),
             ((0, 1.5, 1.5, 0, 0, 0), 0.0)]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


def _double_pendulum_spec(env):
    assert env.spec.action_space.low.tolist() == [-1.0]
    assert env.spec.action_space.high.tolist() == [1.0]


def _double_pendulum_bad_states(rows):
    from garage_amd.envs import PendulumEnv
    bad = np.zeros((rows, 6), dtype=F)
    bad[5, 2] = np.nextafter(PendulumEnv.PI, F(9))
    return [('set_state', np.zeros((rows, 5))), (r'\[-PI, PI\]', bad)]


def _double_pendulum_step(state, obs, rew, box, tally):
    from garage_amd.envs import PendulumEnv
    assert np.isfinite(state).all() and np.isfinite(rew).all()
    assert (np.abs(state[:, 1:3]) <= PendulumEnv.PI).all()
    assert (np.abs(state[:, 3:]) <= 100).all()


def _double_pendulum_rollout(row, whole, env):
    # episodes end both ways, most of them inside the launch's 24 steps
    types_, ends = _ends_both_ways(row, whole)
    assert (whole.lengths[types_[ends] == TERMINAL] < row.P).all()
    assert np.isfinite(whole.agent_infos['mean']).all()
    assert np.isfinite(whole.observations).all()
    assert (whole.observations[:, 8:] == 0).all()
    # the batch keeps the policy's own actions, not the clipped pushes
    assert np.abs(whole.actions).max() > 1
    assert len(np.unique(whole.rewards)) > row.NUM // 2
    # the terminating step keeps its reward (alive bonus included)
    assert (whole.rewards[ends] > 0).all()


def _finished_two_episodes(row, whole, counters, order):
    assert len(counters) == row.N and min(counters.values()) >= 2


def _double_pendulum_pop_member(row, got, vector):
    _log_std_is_the_members(got, vector)


def _double_pendulum_pop_final(row, stats, terminated, returns):
    terminated = np.concatenate(terminated)
    print('population: {} episodes, {} terminated'.format(
        len(terminated), int(terminated.sum())))
    assert terminated.any() and not terminated.all()
    _raises_under_normalize(row)


def _double_pendulum_cem_episodes(episodes, length, tally):
    lengths = np.asarray(episodes.lengths)
    assert (1 <= lengths).all() and (lengths <= length).all()
    tally.append(np.asarray(episodes.terminated))


def _double_pendulum_cem_final(returned, length, tally):
    assert np.isfinite(returned).all() and (returned > 0).all()
    assert len(np.unique(returned)) > 1
    assert np.concatenate(tally).any()


def _double_pendulum_draws(row, cases, draws):
    from garage_amd.envs import DoublePendulumEnv
    _grid_distinct_and_high_word(row, cases, draws)
    assert len(set(h.reset_draw_py(row, 0, 0, 0).tolist())) == 6  # six words
    # the constants are the issue's, each rounded once
    for got, want in zip((DoublePendulumEnv.D1, DoublePendulumEnv.D2,
                          DoublePendulumEnv.D3, DoublePendulumEnv.D4,
                          DoublePendulumEnv.D5, DoublePendulumEnv.D6,
                          DoublePendulumEnv.F1, DoublePendulumEnv.F2),
                         (18.9, 3.78, 1.26, 2.016, 0.756, 0.504, 37.0818,
                          12.3606)):
        assert got == np.float32(want) and isinstance(got, np.float32)


DOUBLE_PENDULUM = Kind(
    name='double_pendulum', batch='DoublePendulumVecEnv',
    twin='DoublePendulumEnv', draw='double_pendulum_reset_draw',
    struct_name='DoublePendulumEnv', kind_macro='GA_ENV_DOUBLE_PENDULUM',
    draw_entry='ga_double_pendulum_reset_draw',
    obs_dim=11, state_dim=6, discrete=False,
    frame_actions=lambda rng, shape: rng.uniform(-1.3, 1.3, shape),
    # the kernel test: 12 steps against twin objects, pushes beyond the clips
    kernel_steps=12, kernel_twins=h._TwinObjects,
    kernel_actions=lambda rng, shape: rng.uniform(-1.6, 1.6, shape),
    edge_states=_double_pendulum_edge_states,
    hold=[(11, 0)],  # the fixed point stays up: TIMEOUT at step P
    check_spec=_double_pendulum_spec, bad_states=_double_pendulum_bad_states,
    check_step=_double_pendulum_step,
    timeout_seen=lambda n, P: P <= 2 or (P == 7 and n >= 15),
    check_kernel_tally=lambda n, tally: None,
    N=33, P=7, NUM=33 * 24,  # 24 steps in the one launch
    rollout_policy_kw=dict(init_std=0.5), rollout_cases=CASES_4,
    check_rollout=_double_pendulum_rollout,
    replay_action=lambda a: a, check_replay=_finished_two_episodes,
    fragment_endings={TERMINAL, TIMEOUT},
    POP_SEED=5, POP_M=4, POP_G=16, POP_P=7, POP_NUM=16 * 24, DISCOUNT=0.99,
    pop_policy_kw=dict(learn_std=True), pop_scale=0.2, pop_log_std=(0.1, 0.5),
    check_pop_member=_double_pendulum_pop_member,
    check_pop_stats=_distinct_rewards,
    check_pop_final=_double_pendulum_pop_final,
    check_cem_episodes=_double_pendulum_cem_episodes,
    check_cem_final=_double_pendulum_cem_final,
    stream=7, draw_blocks=2, draw_cases=h.grid_draw_cases,
    draw_from_words=lambda w: [F(-0.1) + F(0.2) * h.unit(x) for x in w[:6]],
    check_draw=_within_a_tenth, check_draws=_double_pendulum_draws,
    cname='ga_double_pendulum_env', kind_number=6, ldo=12,
    unknown_kinds=(7, ),
)


# -- acrobot ------------------------------------------------------------------
def _acrobot_near_goal(count, classes=(0, 1, 2)):
    """``count`` distinct states (th1 from 2.2 up, the arm straight, moving up)
    whose next step ends the episode whatever the class."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    th1 = np.linspace(2.2, 3.0, 161).astype(f)
    st = np.stack([th1, np.zeros_like(th1), np.full_like(th1, 2.0),
                   np.zeros_like(th1)], axis=-1)
    ok = np.ones(len(st), dtype=bool)
    for k in classes:
        ok &= AcrobotEnv.advance(st, np.full(len(st), k))[3]
    st = st[ok]
    assert len(st) >= count
    return st[np.linspace(0, len(st) - 1, count).astype(int)]


def _acrobot_edge_states():
    """Scripted starts and their first classes: both speed clips either way,
    angles at exactly +-PI, the folds of sincos, one step from the goal, the
    fixed point."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    pi, half = AcrobotEnv.PI, f(1.5707963267948966)
    v1, v2 = AcrobotEnv.MAX_VEL_1, AcrobotEnv.MAX_VEL_2
    rows = [((1.598, -1.980, -v1, -v2), 0),   # the largest stage angle
            ((-1.598, 1.980, v1, v2), 2),
            ((0.3, -0.2, v1, -v2), 2),
            ((0.3, -0.2, -v1, v2), 0),
            ((pi, -pi, 1, -1), 1),
            ((-pi, pi, -3, 3), 3),
            ((np.nextafter(pi, f(0)), 0.1, 3, 0), -1),
            ((half, -half, 0, 0), 2),
            ((0, 0, 0, 0), 1)]
    rows += [(tuple(s), k) for s, k in zip(_acrobot_near_goal(3), (0, 1, 2))]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


def _acrobot_spec(env):
    assert env.spec.action_space.n == 3


def _acrobot_bad_states(rows):
    from garage_amd.envs import AcrobotEnv
    angle = np.zeros((rows, 4), dtype=F)
    angle[5, 1] = np.nextafter(AcrobotEnv.PI, F(9))
    speed = np.zeros((rows, 4), dtype=F)
    speed[5, 3] = np.nextafter(AcrobotEnv.MAX_VEL_2, F(99))
    return [('set_state', np.zeros((rows, 5))), (r'\[-PI, PI\]', angle),
            ('speeds', speed)]


def _acrobot_advance(state, actions):
    from garage_amd.envs import AcrobotEnv
    return AcrobotEnv.advance(state, np.asarray(actions).astype(int))


def _acrobot_step(state, obs, rew, box, tally):
    from garage_amd.envs import AcrobotEnv
    assert (np.abs(state[:, :2]) <= AcrobotEnv.PI).all()
    assert (obs >= box.low).all() and (obs <= box.high).all()


def _acrobot_box(n):
    """States drawn from the whole box -- a quarter on the faces of the speed
    box, where the RK4 stages overshoot by tens of radians -- with all
    classes, and what one step from them must reach."""
    from garage_amd.envs import AcrobotEnv
    f = np.float32
    rng = np.random.RandomState(12)
    hi = np.asarray([AcrobotEnv.PI, AcrobotEnv.PI, AcrobotEnv.MAX_VEL_1,
                     AcrobotEnv.MAX_VEL_2], dtype=f)
    st = (rng.uniform(-1, 1, (n, 4)) * hi).astype(f)
    st[:n // 8, 2] = np.where(st[:n // 8, 2] < 0, -1, 1) * hi[2]
    st[:n // 4, 3] = np.where(st[:n // 4, 3] < 0, -1, 1) * hi[3]
    st = np.clip(st, -hi, hi)
    actions = rng.randint(-1, 4, n).astype(f)

    def reached(new):
        assert (np.abs(new[:, 2]) == hi[2]).any()
        assert (np.abs(new[:, 3]) == hi[3]).any()

    return st, actions, reached


def _acrobot_classes(whole):
    # all three classes drive the env
    assert set(np.unique(whole.actions)) == {0.0, 1.0, 2.0}


def _acrobot_rollout(row, whole, env):
    types_, ends = _ends_both_ways(row, whole)
    assert (types_[ends] == TERMINAL).sum() >= row.SCRIPTED
    assert (whole.lengths[types_[ends] == TERMINAL] < row.P).all()
    assert np.isfinite(whole.agent_infos['prob']).all()
    assert whole.agent_infos['prob'].shape[-1] == 3
    _acrobot_classes(whole)
    # -1 per step, 0 on the terminating step only
    want = np.full(len(types_), -1, dtype=np.float32)
    want[ends[types_[ends] == TERMINAL]] = 0
    assert np.array_equal(whole.rewards, want)
    _inside_the_box(whole, env)


def _acrobot_pop_starts(row, n, env_id0=0):
    """The first states of ``n`` envs from ``env_id0`` on: of each member's 16,
    five one step from the goal, the others their reset draws."""
    states = h.draws(row, 3, env_id0, n)
    near = _acrobot_near_goal(row.POP_SCRIPTED)
    for lo in range(0, n, row.POP_G):
        states[lo:lo + row.POP_SCRIPTED] = near
    return states


def _acrobot_pop_member(row, got, vector):
    assert set(np.unique(got.actions)) <= {0.0, 1.0, 2.0}


def _acrobot_pop_stats(st, host, lengths, term):
    # sparse reward: the return is the length, less the terminating step
    assert np.array_equal(st.undiscounted_returns,
                          -(lengths - np.asarray(term, dtype=np.int64)))


def _acrobot_pop_final(row, stats, terminated, returns):
    terminated = np.concatenate(terminated)
    print('population: {} episodes, {} terminated'.format(
        len(terminated), int(terminated.sum())))
    # both occur: the scripted starts swing up, every other episode times out
    assert terminated.sum() >= row.POP_M * row.POP_SCRIPTED
    assert (~terminated).sum() >= row.POP_M * row.POP_G


def _acrobot_cem_episodes(episodes, length, tally):
    lengths = np.asarray(episodes.lengths)
    assert (1 <= lengths).all() and (lengths <= length).all()
    und = np.asarray(episodes.undiscounted_returns)
    term = np.asarray(episodes.terminated)
    assert np.array_equal(und, -(lengths - term))


def _acrobot_cem_final(returned, length, tally):
    """Scored on returns that tie (every episode that does not swing up
    returns -20)."""
    assert np.isfinite(returned).all()
    assert (returned <= 0).all() and (returned >= -length).all()


def _acrobot_draws(row, cases, draws):
    _grid_distinct_and_high_word(row, cases, draws)
    assert len(set(h.reset_draw_py(row, 0, 0, 0).tolist())) == 4


ACROBOT = Kind(
    name='acrobot', batch='AcrobotVecEnv', twin='AcrobotEnv',
    draw='acrobot_reset_draw', struct_name='AcrobotEnv',
    kind_macro='GA_ENV_ACROBOT', draw_entry='ga_acrobot_reset_draw',
    obs_dim=6, state_dim=4, discrete=True,
    # all three classes and the out-of-range indices 3 and -1
    frame_actions=lambda rng, shape: rng.randint(-1, 4, shape),
    kernel_steps=40, kernel_twins=h._Twins,
    kernel_actions=lambda rng, shape: rng.randint(-1, 4, shape),
    edge_states=_acrobot_edge_states,
    hold=[(8, 1)],  # the fixed point stays down: TIMEOUT at step P
    check_spec=_acrobot_spec, bad_states=_acrobot_bad_states,
    advance=_acrobot_advance, check_step=_acrobot_step,
    timeout_seen=lambda n, P: P <= 7,
    check_kernel_tally=lambda n, tally: None,
    box_sample=_acrobot_box,
    N=64, P=7, NUM=64 * 24,  # 24 steps in the one launch
    SCRIPTED=20,  # members 0 .. 19 start one step from the goal
    near_end=_acrobot_near_goal, rollout_cases=CASES_5,
    check_rollout=_acrobot_rollout,
    replay_action=lambda a: a, check_replay=_finished_two_episodes,
    check_host_call=_acrobot_classes,
    fragment_endings={TIMEOUT},
    POP_SEED=5, POP_M=4, POP_G=16, POP_P=7, POP_NUM=16 * 24, DISCOUNT=0.99,
    POP_SCRIPTED=5,  # of each member's 16 envs
    pop_policy_kw={}, pop_scale=0.5, pop_starts=_acrobot_pop_starts,
    check_pop_member=_acrobot_pop_member, check_pop_stats=_acrobot_pop_stats,
    check_pop_final=_acrobot_pop_final,
    check_cem_episodes=_acrobot_cem_episodes,
    check_cem_final=_acrobot_cem_final,
    stream=8, draw_cases=h.grid_draw_cases,
    draw_from_words=lambda w: [F(-0.1) + F(0.2) * h.unit(x) for x in w],
    check_draw=_within_a_tenth, check_draws=_acrobot_draws,
    # 7 and 9 stay kinds that are refused as unknown (the tests of the earlier
    # kinds rely on it), so the two kinds after the double pendulum are 8, 10
    cname='ga_acrobot_env', kind_number=8, ldo=8, unknown_kinds=(7, 9, 11),
)


# -- mountain car, both variants ----------------------------------------------
def _past_goal(count):
    """``count`` distinct states below the goal line, moving right fast enough
    that the next step passes it whatever the action, in either variant."""
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    st = np.stack([np.linspace(0.47, 0.499, count), np.full(count, 0.06)],
                  axis=-1).astype(f)
    for continuous, acts in ((False, (0, 1, 2)), (True, (-1.0, 0.0, 1.0))):
        for a in acts:
            act = np.full(count, a, dtype=f if continuous else int)
            assert MountainCarEnv.advance(st, act, continuous)[3].all()
    return st


def _car_edge_states(continuous):
    """Scripted starts and their first actions: on the left wall moving left
    and at rest, running into it, on the right wall at full speed, one step
    from each goal line, past the goal moving left, and actions past +-1 /
    out of range."""
    from garage_amd.envs import MountainCarEnv
    f = np.float32
    lo, hi, vmax = (MountainCarEnv.MIN_X, MountainCarEnv.MAX_X,
                    MountainCarEnv.MAX_V)
    left, right, coast = ((-1.7, 1.7, 0.0) if continuous else (0, 2, 1))
    odd = 0.3 if continuous else 3
    rows = [((lo, -0.03), left), ((lo, 0), coast), ((lo, 0.02), right),
            ((-1.19, -vmax), left), ((-1.15, -0.05), odd),
            ((hi, vmax), right), ((0.58, vmax), right),
            ((0.499, 0.03), right), ((0.449, 0.03), right),
            ((0.499, 0.0005), left), ((0.55, -0.02), left),
            ((-0.5, 0), -1.0 if continuous else -1)]
    return (np.asarray([r[0] for r in rows], dtype=f),
            np.asarray([r[1] for r in rows], dtype=f))


def _car_spec(continuous):
    def check(env):
        assert env._c.continuous == int(continuous)
        if continuous:
            assert env.spec.action_space.low.tolist() == [-1.0]
            assert env.spec.action_space.high.tolist() == [1.0]
        else:
            assert env.spec.action_space.n == 3
    return check


def _car_bad_states(rows):
    from garage_amd.envs import MountainCarEnv
    out = [('set_state', np.zeros((rows, 3)))]
    for j, v in ((0, MountainCarEnv.MAX_X), (1, MountainCarEnv.MAX_V),
                 (0, MountainCarEnv.MIN_X), (1, -MountainCarEnv.MAX_V)):
        bad = np.zeros((rows, 2), dtype=F)
        bad[5, j] = np.nextafter(v, F(9) * np.sign(v))
        out.append(('set_state needs x', bad))
    return out


def _car_advance(continuous):
    def advance(state, actions):
        from garage_amd.envs import MountainCarEnv
        actions = np.asarray(actions)
        return MountainCarEnv.advance(
            state, actions if continuous else actions.astype(int), continuous)
    return advance


def _car_step(state, obs, rew, box, tally):
    from garage_amd.envs import MountainCarEnv
    assert (obs >= box.low).all() and (obs <= box.high).all()
    on_wall = obs[:, 0] == MountainCarEnv.MIN_X
    assert (obs[on_wall, 1] >= 0).all()
    tally.append(int(on_wall.sum()))


def _car_kernel_tally(n, tally):
    print('steps that ended on the wall', sum(tally))
    if n >= 15:
        assert sum(tally) >= 2


def _car_box(continuous):
    def sample(n):
        """States drawn from the whole box, its faces included, with every
        kind of action, and what one step from them must reach."""
        from garage_amd.envs import MountainCarEnv
        f = np.float32
        rng = np.random.RandomState(13)
        lo = np.asarray([MountainCarEnv.MIN_X, -MountainCarEnv.MAX_V], dtype=f)
        hi = np.asarray([MountainCarEnv.MAX_X, MountainCarEnv.MAX_V], dtype=f)
        st = np.stack([rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)],
                      axis=-1).astype(f)
        st[:100, 0], st[100:200, 0] = lo[0], hi[0]
        st[200:300, 1], st[300:400, 1] = lo[1], hi[1]
        st = np.clip(st, lo, hi)
        if continuous:
            actions = rng.uniform(-1.6, 1.6, n).astype(f)
        else:
            actions = rng.randint(-1, 4, n).astype(f)

        def reached(new):
            assert ((new[:, 0] == lo[0]) & (new[:, 1] == 0)).any()

        return st, actions, reached
    return sample


def car_rewards(continuous):
    def check(eps):
        """-1 every step; or +100 on the goal step, minus 0.1 a^2 of the
        policy's own (unclipped) action."""
        types_, ends = h._ends(eps)
        if continuous:
            f = np.float32
            a = np.asarray(eps.actions, dtype=f)[:, 0]
            bonus = np.zeros(len(a), dtype=f)
            bonus[ends[types_[ends] == TERMINAL]] = 100
            assert np.array_equal(h._bits(eps.rewards),
                                  h._bits(bonus - f(0.1) * (a * a)))
            assert np.abs(a).max() > 1  # the batch keeps the unclipped actions
        else:
            assert (eps.rewards == -1).all()
            assert set(np.unique(eps.actions)) == {0.0, 1.0, 2.0}
    return check


def _car_rollout(continuous):
    def check(row, whole, env):
        types_, ends = _ends_both_ways(row, whole)
        assert (types_[ends] == TERMINAL).sum() == row.SCRIPTED
        assert (whole.lengths[types_[ends] == TERMINAL] == 1).all()
        head = 'mean' if continuous else 'prob'
        assert np.isfinite(whole.agent_infos[head]).all()
        car_rewards(continuous)(whole)
        _inside_the_box(whole, env)
    return check


def _car_pickled(continuous):
    def check(ea, eb):
        assert eb.continuous == continuous
        assert eb._c.continuous == int(continuous)
        assert eb.spec.action_space.flat_dim == ea.spec.action_space.flat_dim
    return check


def _car_pop_starts(row, n, env_id0=0):
    """The first states of ``n`` envs from ``env_id0`` on: their reset draws,
    but for global env 21, one step from the goal."""
    states = h.draws(row, 3, env_id0, n)
    if env_id0 <= row.POP_AT_GOAL < env_id0 + n:
        states[row.POP_AT_GOAL - env_id0] = _past_goal(3)[1]
    return states


def _car_pop_member(continuous):
    def check(row, got, vector):
        if continuous:
            _log_std_is_the_members(got, vector)
    return check


def _car_pop_final(continuous):
    def check(row, stats, terminated, returns):
        # exactly one env reached the goal, once: member 1's, on its first step
        counts = [int(t.sum()) for t in terminated]
        print('population: terminated episodes per member', counts)
        assert counts == [0, 1, 0, 0]
        hit = int(np.nonzero(terminated[1])[0][0])
        assert stats[1].lengths[hit] == 1
        best = max(float(r.max()) for r in returns)
        if continuous:  # +100 less the cost of one action: the one above 0
            assert 90 < returns[1][hit] == best
            assert sum(int((r > 0).sum()) for r in returns) == 1
            _raises_under_normalize(row)
        else:  # -1 against -7 everywhere else
            assert returns[1][hit] == best == -1
            assert sum(int((r > -row.POP_P).sum()) for r in returns) == 1
    return check


def _car_draw(got):
    assert np.float32(-0.6) <= got[0] <= np.float32(-0.4)
    assert got[1] == 0


def _car_struct():
    import ctypes
    from garage_amd import _lib
    # `continuous` sits where the neighbours have their padding
    assert _lib.MountainCarEnv.continuous.offset == _lib.PendulumEnv.pad_.offset
    assert (ctypes.sizeof(_lib.MountainCarEnv) ==
            ctypes.sizeof(_lib.PendulumEnv))


def _car(name, continuous):
    return Kind(
        name=name, batch='MountainCarVecEnv', twin='MountainCarEnv',
        draw='mountain_car_reset_draw', kw={'continuous': continuous},
        struct_name='MountainCarEnv', kind_macro='GA_ENV_MOUNTAIN_CAR',
        draw_entry='ga_mountain_car_reset_draw',
        obs_dim=2, state_dim=2, discrete=not continuous,
        # forces outside [-1, 1]; or all three classes and the out-of-range
        # indices 3 and -1
        frame_actions=(lambda rng, shape: rng.uniform(-1.6, 1.6, shape))
        if continuous else (lambda rng, shape: rng.randint(-1, 4, shape)),
        kernel_steps=40, kernel_twins=h._Twins,
        kernel_actions=(lambda rng, shape: rng.uniform(-1.6, 1.6, shape))
        if continuous else (lambda rng, shape: rng.randint(-1, 4, shape)),
        edge_states=lambda: _car_edge_states(continuous), hold=[],
        check_spec=_car_spec(continuous), bad_states=_car_bad_states,
        advance=_car_advance(continuous), check_step=_car_step,
        timeout_seen=lambda n, P: P <= 7,
        check_kernel_tally=_car_kernel_tally,
        box_sample=_car_box(continuous),
        N=64, P=7, NUM=64 * 24,  # 24 steps in the one launch
        SCRIPTED=20,  # members 0 .. 19 start one step from the goal
        near_end=_past_goal,
        rollout_policy_kw=dict(init_std=0.8) if continuous else {},
        rollout_cases=CASES_5, check_rollout=_car_rollout(continuous),
        replay_action=lambda a: a, check_replay=_finished_two_episodes,
        check_host_call=car_rewards(continuous),
        check_pickled=_car_pickled(continuous),
        fragment_endings={TIMEOUT},
        POP_SEED=5, POP_M=4, POP_G=16, POP_P=7, POP_NUM=16 * 24,
        DISCOUNT=0.99,
        POP_AT_GOAL=21,  # the one env (member 1's sixth) below the line
        pop_policy_kw=dict(learn_std=True) if continuous else {},
        pop_scale=0.2, pop_log_std=(0.3, 0.5), pop_starts=_car_pop_starts,
        check_pop_member=_car_pop_member(continuous),
        check_pop_stats=lambda st, host, lengths, term: None,
        check_pop_final=_car_pop_final(continuous),
        stream=9, draw_cases=h.grid_draw_cases,
        draw_from_words=lambda w: [F(-0.6) + F(0.2) * h.unit(w[0]), 0],
        check_draw=_car_draw, check_draws=_grid_distinct_and_high_word,
        cname='ga_mountain_car_env', kind_number=10, ldo=4,
        unknown_kinds=(7, 9, 11), struct_kw=dict(continuous=int(continuous)),
        struct_errors=[(dict(continuous=bad), 'continuous must be 0 or 1')
                       for bad in (-1, 2)],
        # (None is the variant's own length)
        bad_lengths=(float('inf'), 0, 65536), check_struct=_car_struct,
    )


MOUNTAIN_CAR = _car('mountain_car', False)
MOUNTAIN_CAR_CONTINUOUS = _car('mountain_car_continuous', True)

KINDS = {k.name: k for k in (CARTPOLE, PENDULUM, DOUBLE_PENDULUM, ACROBOT,
                             MOUNTAIN_CAR, MOUNTAIN_CAR_CONTINUOUS)}


def variants(row):
    """The rows that share ``row``'s batch class (MountainCar has two)."""
    return [k for k in KINDS.values() if k.batch == row.batch]


def rows(*names):
    """``pytest.mark.parametrize`` over the named rows, the id a row's name."""
    return pytest.mark.parametrize(
        'row', [pytest.param(KINDS[n], id=n) for n in names])


def cases(row):
    """``pytest.mark.parametrize`` over the row's network cases, the id a
    case's."""
    return pytest.mark.parametrize('case', row.rollout_cases,
                                   ids=[case[0] for case in row.rollout_cases])
