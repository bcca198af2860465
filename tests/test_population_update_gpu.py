"""A population of narrow learners trained in shared launches
(``ga_update_epoch_members``, ``PopulationPPO``).

The contract is the project's twin rule: each member gets, bit for bit, what a lone
learner on the member's batch gets from ``ga_update_epoch`` on the narrow path
(``ga_set_small_step(0)``, ``ga_set_narrow_step(1)``) -- parameters, both Adam moments,
gradients and per-step losses at the entry point; both networks' parameters and
moments and the logged scalars at the algorithm.
"""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GA_PROF_NARROW_STEP = 11
GA_PROF_MEMBERS_STEP = 15
SIZES = (130, 64, 200, 1, 65)      # mb = 64: 3, 1, 4, 1, 2 steps
STEP0 = (0, 7, 1000, 3, 1)
SENTINEL = 12345.0
PAD = 8                            # floats between two members' rows

# H, in_w, kind, A, algo, members, mb, options
CASES = [
    (64, 4, 2, 2, 0, 5, 64, {}),
    (64, 4, 2, 2, 0, 5, 100, {}),
    (64, 4, 2, 2, 0, 5, 0, {}),
    (64, 4, 1, 1, 0, 5, 64, {}),
    (64, 4, 1, 1, 0, 5, 100, {}),
    (64, 4, 1, 1, 0, 3, 0, {}),
    (32, 4, 2, 3, 0, 3, 64, {}),
    (32, 4, 2, 2, 1, 5, 64, {}),
    (64, 4, 2, 3, 0, 3, 64, {'double_softmax': 1}),
    (64, 4, 2, 2, 0, 5, 64, {'ent_flags': 1}),
    (64, 4, 2, 2, 0, 3, 100, {'ent_flags': 7}),
    (64, 11, 0, 1, 0, 5, 64, {}),
    (64, 11, 0, 6, 0, 5, 64, {}),
    (64, 17, 0, 6, 0, 3, 100, {}),
    (32, 17, 0, 1, 1, 5, 64, {}),
    (32, 11, 0, 6, 0, 1, 64, {}),
    (64, 11, 0, 1, 0, 3, 64, {'learn_std': 0}),
    (64, 11, 0, 6, 0, 3, 0, {'ent_flags': 1}),
    (64, 11, 0, 1, 0, 3, 64, {'clamp': True}),
    (32, 11, 1, 1, 0, 5, 64, {}),
    (64, 17, 1, 1, 0, 5, 0, {}),
    (32, 17, 1, 1, 0, 1, 100, {}),
    (64, 4, 2, 2, 0, 1, 64, {}),
    (64, 4, 2, 2, 0, 1, 0, {}),
    (32, 4, 0, 6, 1, 5, 100, {}),
    (32, 17, 2, 3, 0, 5, 100, {}),
    (64, 17, 2, 2, 1, 3, 0, {}),
    (32, 4, 1, 1, 0, 3, 64, {'learn_std': 0}),
    (64, 11, 0, 6, 1, 5, 64, {'ent_flags': 5}),
    (32, 11, 2, 2, 0, 5, 0, {'double_softmax': 1}),
    # Full-batch members of 24 and 130 tiles: where the optimizer launch's two
    # summation trees differ (5 .. 128 tiles: 64 quads a workgroup, 4 shares) and
    # where it takes the other one (> 128 tiles: 16 quads, 16 shares), both in ONE
    # launch, and a 32-tile minibatch.
    (64, 4, 2, 2, 0, 2, 0, {'sizes': (1500, 8300)}),
    (64, 4, 1, 1, 0, 2, 0, {'sizes': (8300, 1500)}),
    (32, 11, 0, 6, 0, 3, 0, {'sizes': (1500, 130, 8300)}),
    (64, 17, 0, 1, 1, 2, 2048, {'sizes': (8300, 1500)}),
    (32, 4, 1, 1, 0, 1, 0, {'sizes': (8300, )}),
]


def _case_id(c):
    H, in_w, kind, A, algo, M, mb, opt = c
    return 'H{}-in{}-kind{}-A{}-{}-M{}-mb{}{}'.format(
        H, in_w, kind, A, 'vpg' if algo else 'ppo', M, mb,
        ''.join('-{}{}'.format(k, 'x'.join(map(str, v)) if k == 'sizes' else v)
                for k, v in sorted(opt.items())))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _steps(S, mb):
    return 1 if mb == 0 else -(-S // mb)


class _Population:
    """Random members of one case, every buffer the members' pass writes placed in
    sentinel-filled surroundings, and copies for the lone runs."""

    def __init__(self, case, seed=0):
        from garage_amd import _lib
        from garage_amd.engine import FlatMLP, round4
        H, in_w, kind, A, algo, M, mb, opt = case
        self.case = case
        dev = torch.device('cuda')
        g = torch.Generator(device='cpu').manual_seed(seed)
        self.net = net = FlatMLP(in_w, A, (H, H), dev)
        self.lib = lib = _lib.load()
        n_flat = net.n_flat
        self.stride = stride = n_flat + PAD

        def rows(scale, positive=False):
            t = torch.full((M + 2, stride), SENTINEL)
            v = torch.randn(M, n_flat, generator=g) * scale
            t[1:M + 1, :n_flat] = v.abs() if positive else v
            return t.to(dev)

        self.params, self.grads = rows(0.2), rows(1.0)
        self.exp_avg, self.exp_avg_sq = rows(0.01), rows(1e-4, positive=True)
        self.params[1:M + 1, 0] = torch.linspace(-0.5, 0.1, M)  # log std
        self.members = []
        for m in range(M):
            S = opt.get('sizes', SIZES)[m]
            X = torch.zeros(S, round4(in_w))
            X[:, :in_w] = torch.randn(S, in_w, generator=g)
            if kind == 2:
                act = torch.zeros(S, 4)
                act[:, 0] = torch.randint(0, A, (S, ), generator=g).float()
            else:
                act = torch.zeros(S, round4(A))
                act[:, :A] = torch.randn(S, A, generator=g)
            d = dict(
                S=S, X=X.to(dev), actions=act.to(dev),
                adv=torch.randn(S, generator=g).to(dev),
                old_ll=(-1.0 * A + 0.1 * torch.randn(S, generator=g)).to(dev),
                returns=torch.randn(S, generator=g).to(dev),
                perm=None if mb == 0 else torch.randperm(
                    S, generator=g).to(torch.int32).to(dev),
                lr=1e-3 * (m + 1), clip=0.1 + 0.05 * m,
                ent_coeff=0.01 * (m + 1) if opt.get('ent_flags', 0) & 1 else 0.0,
                step0=STEP0[m], n_steps=_steps(S, mb))
            d['losses'] = torch.full((d['n_steps'] + 2, ), SENTINEL, device=dev)
            self.members.append(d)
        max_rows = max(d['S'] if mb == 0 else min(d['S'], mb)
                       for d in self.members)
        self.need = int(lib.ga_update_members_partials_floats(
            C.byref(net._desc), M, max_rows))
        assert self.need > 0
        self.partials = torch.full((self.need + 2 * PAD, ), SENTINEL, device=dev)
        self.n_steps = max(d['n_steps'] for d in self.members)

    def _shared(self, a):
        H, in_w, kind, A, algo, M, mb, opt = self.case
        a.kind, a.algo = kind, algo
        a.ent_flags = opt.get('ent_flags', 0)
        if opt.get('clamp'):
            # member 0's log std (-0.5) lies under the lower clamp
            a.has_min, a.min_log_std, a.has_max, a.max_log_std = 1, -0.3, 1, 0.05
        a.double_softmax = opt.get('double_softmax', 0)
        a.learn_std = opt.get('learn_std', 1)
        a.beta1, a.beta2, a.eps, a.mb = 0.9, 0.999, 1e-8, mb

    def run_members(self):
        from garage_amd import _lib
        M = self.case[5]
        a = _lib.UpdateMembersArgs()
        a.desc = C.pointer(self.net._desc)
        self._shared(a)
        a.n_members = M
        arr = (_lib.MemberUpdate * M)()
        for m, d in enumerate(self.members):
            u = arr[m]
            u.params = self.params[m + 1].data_ptr()
            u.grads = self.grads[m + 1].data_ptr()
            u.exp_avg = self.exp_avg[m + 1].data_ptr()
            u.exp_avg_sq = self.exp_avg_sq[m + 1].data_ptr()
            u.X, u.ldx, u.S = d['X'].data_ptr(), d['X'].stride(0), d['S']
            u.perm = None if d['perm'] is None else d['perm'].data_ptr()
            u.actions, u.lda = d['actions'].data_ptr(), d['actions'].stride(0)
            u.old_ll, u.adv = d['old_ll'].data_ptr(), d['adv'].data_ptr()
            u.returns = d['returns'].data_ptr()
            u.step0, u.lr = d['step0'], d['lr']
            u.clip, u.ent_coeff = d['clip'], d['ent_coeff']
            u.losses = d['losses'][1:].data_ptr()
        a.members_host = arr
        a.partials = self.partials[PAD:].data_ptr()
        a.partials_floats = self.need
        _lib.call('ga_update_epoch_members', C.byref(a), _lib.stream_ptr())
        torch.cuda.synchronize()

    def surroundings_intact(self):
        M, n_flat = self.case[5], self.net.n_flat
        ok = True
        for t in (self.params, self.exp_avg, self.exp_avg_sq, self.grads):
            ok &= bool((t[0] == SENTINEL).all() and (t[M + 1] == SENTINEL).all()
                       and (t[1:M + 1, n_flat:] == SENTINEL).all())
        ok &= bool((self.partials[:PAD] == SENTINEL).all()
                   and (self.partials[PAD + self.need:] == SENTINEL).all())
        for d in self.members:
            ok &= bool(d['losses'][0] == SENTINEL
                       and d['losses'][-1] == SENTINEL)
        return ok

    def run_lone(self, m, state):
        """``ga_update_epoch`` on copies of member ``m``'s initial ``state`` rows;
        returns (params, exp_avg, exp_avg_sq, grads, losses)."""
        from garage_amd import _lib
        from garage_amd.engine import reduction_workspace
        net, d = self.net, self.members[m]
        n_flat = net.n_flat
        bufs = [s[m + 1, :n_flat].clone() for s in state]
        rows = d['S'] if d['perm'] is None else min(d['S'], self.case[6])
        net._workspace(rows)
        part = net.train_partials(rows)
        losses = torch.zeros(d['n_steps'], device=net.device)
        scratch = torch.zeros(1, device=net.device)
        a = _lib.UpdateArgs()
        a.desc = C.pointer(net._desc)
        a.params, a.exp_avg, a.exp_avg_sq, a.grads = (b.data_ptr() for b in bufs)
        a.n_flat = n_flat
        a.acts, a.dacts = net._acts.data_ptr(), net._dacts.data_ptr()
        a.out, a.dout, a.ldo = net._out.data_ptr(), net._dout.data_ptr(), net.ld_out
        a.slabs, a.max_splits = net._slabs.data_ptr(), int(net._splits)
        self._shared(a)
        a.step0, a.lr = d['step0'], d['lr']
        a.X, a.ldx, a.S = d['X'].data_ptr(), d['X'].stride(0), d['S']
        a.perm = None if d['perm'] is None else d['perm'].data_ptr()
        a.actions, a.lda = d['actions'].data_ptr(), d['actions'].stride(0)
        a.old_ll, a.adv = d['old_ll'].data_ptr(), d['adv'].data_ptr()
        a.returns = d['returns'].data_ptr()
        a.clip, a.ent_coeff = d['clip'], d['ent_coeff']
        a.losses, a.loss_scratch = losses.data_ptr(), scratch.data_ptr()
        a.workspace = reduction_workspace(net.device, 0).data_ptr()
        a.partials, a.partials_floats = part.data_ptr(), part.numel()
        _lib.call('ga_update_epoch', C.byref(a), _lib.stream_ptr())
        torch.cuda.synchronize()
        return bufs + [losses]


@pytest.fixture
def narrow_path():
    """The lone runs take ``narrow_train_kernel``: small step off, narrow step on."""
    from garage_amd import _lib
    lib = _lib.load()
    lib.ga_set_small_step(0)
    lib.ga_set_narrow_step(1)
    try:
        yield lib
    finally:
        lib.ga_set_small_step(1)
        lib.ga_set_narrow_step(1)


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_each_member_equals_a_lone_pass_bit_for_bit(case, narrow_path):
    lib = narrow_path
    pop = _Population(case)
    state = [t.clone() for t in (pop.params, pop.exp_avg, pop.exp_avg_sq,
                                 pop.grads)]
    pop.run_members()
    assert pop.surroundings_intact()
    n_flat = pop.net.n_flat
    for m, d in enumerate(pop.members):
        before = lib.ga_launch_count(GA_PROF_NARROW_STEP)
        want = pop.run_lone(m, state)
        # the switches did select narrow_train_kernel for the lone pass
        assert lib.ga_launch_count(GA_PROF_NARROW_STEP) - before == d['n_steps']
        got = [pop.params[m + 1, :n_flat], pop.exp_avg[m + 1, :n_flat],
               pop.exp_avg_sq[m + 1, :n_flat], pop.grads[m + 1, :n_flat],
               d['losses'][1:-1]]
        for name, x, y in zip(('params', 'exp_avg', 'exp_avg_sq', 'grads',
                               'losses'), got, want):
            assert bool(torch.isfinite(y).all()), (m, name)
            assert torch.equal(_bits(x), _bits(y)), (m, name)
        # the pass moved this member
        assert not torch.equal(want[0], state[0][m + 1, :n_flat])


@pytest.mark.parametrize('case', [CASES[0], CASES[1], CASES[13], CASES[20],
                                  CASES[30], CASES[33]], ids=_case_id)
def test_nothing_outside_the_members_buffers_is_written(case):
    """``partials`` at exactly the size ``ga_update_members_partials_floats`` returns
    inside a larger tensor, every member row padded to the stride, the per-step
    losses at exactly their count: the sentinels around all of them survive."""
    pop = _Population(case, seed=3)
    assert pop.surroundings_intact()
    pop.run_members()
    assert pop.surroundings_intact()
    assert bool((pop.partials[PAD:PAD + pop.need] != SENTINEL).any())


@pytest.mark.parametrize('case', [CASES[0], CASES[4], CASES[23]], ids=_case_id)
def test_a_pass_takes_the_members_kernel(case):
    from garage_amd import _lib
    lib = _lib.load()
    pop = _Population(case, seed=5)
    lone, joint = (lib.ga_launch_count(GA_PROF_NARROW_STEP),
                   lib.ga_launch_count(GA_PROF_MEMBERS_STEP))
    pop.run_members()
    assert lib.ga_launch_count(GA_PROF_MEMBERS_STEP) - joint == pop.n_steps
    assert lib.ga_launch_count(GA_PROF_NARROW_STEP) == lone


# -- the algorithm: PopulationPPO against lone PPOs ------------------------------
def _make_members(head, permutation):
    """(env, members): 3 categorical MLP(32, 32) PPOs on CartPole or 2 Gaussian
    MLP(64, 64) PPOs on Pendulum, 16 envs each, with their own learning rate,
    clip range and permutation seeds."""
    from garage_amd.algos import PPO
    from garage_amd.envs import CartPoleVecEnv, PendulumVecEnv
    from garage_amd.optimizers import OptimizerWrapper
    from garage_amd.policies import (CategoricalMLPPolicy, GaussianMLPPolicy,
                                     GaussianMLPValueFunction)
    if head == 'categorical':
        M, hidden = 3, (32, 32)
        env = CartPoleVecEnv(M * 16, max_episode_length=20, seed=3)
    else:
        M, hidden = 2, (64, 64)
        env = PendulumVecEnv(M * 16, max_episode_length=20, seed=3)
    members = []
    for m in range(M):
        torch.manual_seed(10 + m)
        if head == 'categorical':
            pol = CategoricalMLPPolicy(env.spec, hidden_sizes=hidden)
        else:
            pol = GaussianMLPPolicy(env.spec, hidden_sizes=hidden)
        vf = GaussianMLPValueFunction(env.spec, hidden_sizes=hidden)
        opt = (torch.optim.Adam, dict(lr=1e-3 * (m + 1)))
        members.append(PPO(
            env_spec=env.spec, policy=pol, value_function=vf, sampler=None,
            policy_optimizer=OptimizerWrapper(opt, pol, 2, 64,
                                              permutation=permutation, seed=m),
            vf_optimizer=OptimizerWrapper(opt, vf, 2, 64,
                                          permutation=permutation,
                                          seed=100 + m),
            lr_clip_range=0.1 + 0.05 * m))
    return env, members


def _network_state(algo):
    out = []
    for mod in (algo.policy, algo._value_function):
        out += [mod.net.params.clone(), mod.net.exp_avg.clone(),
                mod.net.exp_avg_sq.clone()]
    return out


def _population(head, permutation):
    from garage_amd.algos import PopulationPPO
    from garage_amd.sampler import GpuPopulationSampler
    env, members = _make_members(head, permutation)
    pop = PopulationPPO(members)
    sampler = GpuPopulationSampler(members[0].policy, env,
                                   n_members=len(members),
                                   max_episode_length=20, seed=5)
    return pop, sampler


@pytest.mark.parametrize('permutation', ['device', 'numpy'])
@pytest.mark.parametrize('head', ['categorical', 'gaussian'])
def test_population_ppo_equals_lone_ppos_bit_for_bit(head, permutation,
                                                     narrow_path):
    lib = narrow_path
    pop, sampler = _population(head, permutation)
    _, lones = _make_members(head, permutation)
    M = len(lones)
    for a, b in zip(pop.members, lones):  # the same initial state
        for x, y in zip(_network_state(a), _network_state(b)):
            assert torch.equal(x, y)
    assert pop.member_params.shape == (M, lones[0].policy.net.n_flat)
    np.random.seed(7)
    batches, joint = [], []
    taken = lib.ga_launch_count(GA_PROF_MEMBERS_STEP)
    for itr in range(2):
        batches.append(sampler.obtain_samples(itr, 64, pop.member_params))
        returns = pop.train_once(itr, batches[-1])
        assert len(returns) == M
        joint.append([(_network_state(a), dict(a.last_tabular),
                       a.policy.net.adam_steps,
                       a._value_function.net.adam_steps) for a in pop.members])
    assert lib.ga_launch_count(GA_PROF_MEMBERS_STEP) > taken
    np.random.seed(7)  # the lone runs draw in member order, as the joint run did
    for itr in range(2):
        for m, lone in enumerate(lones):
            lone._train_once(itr, batches[itr][m])
            state, tabular, p_steps, v_steps = joint[itr][m]
            for x, y in zip(state, _network_state(lone)):
                assert torch.equal(_bits(x), _bits(y)), (itr, m)
            assert tabular == lone.last_tabular, (itr, m)
            assert (p_steps, v_steps) == (
                lone.policy.net.adam_steps,
                lone._value_function.net.adam_steps)
    # the members differ from each other and moved
    assert not torch.equal(joint[1][0][0][0], joint[1][1][0][0])
    assert not torch.equal(joint[1][0][0][0], joint[0][0][0][0])


def test_population_ppo_pickle_round_trip():
    """After one iteration, the unpickled copy trains the second iteration to the
    bits of the original: the row views are re-established."""
    pop, sampler = _population('categorical', 'device')
    pop.train_once(0, sampler.obtain_samples(0, 64, pop.member_params))
    copy = pickle.loads(pickle.dumps(pop))
    assert copy.member_params.data_ptr() != pop.member_params.data_ptr()
    for a, b in zip(pop.members, copy.members):
        assert b.policy.net.params.data_ptr() != a.policy.net.params.data_ptr()
    batches = sampler.obtain_samples(1, 64, pop.member_params)
    pop.train_once(1, batches)
    copy.train_once(1, batches)
    for m, (a, b) in enumerate(zip(pop.members, copy.members)):
        for x, y in zip(_network_state(a), _network_state(b)):
            assert torch.equal(_bits(x), _bits(y)), m
        assert a.last_tabular == b.last_tabular
        # a member's parameters ARE its row of the tensor that rolls out
        assert b.policy.net.params.data_ptr() == copy.member_params[m].data_ptr()
    assert torch.equal(pop.member_params, copy.member_params)


def test_population_ppo_train_drives_the_population_sampler():
    """``train``: per epoch one rollout of every member with its own row and one
    joint iteration, logged per member."""
    import types
    from garage_amd import logger
    from garage_amd.algos import PopulationPPO
    pop, sampler = _population('categorical', 'device')
    pop = PopulationPPO(pop.members, sampler=sampler)
    calls, real = [], sampler.obtain_samples

    def obtain_samples(itr, num_samples, member_params, env_update=None):
        calls.append((itr, num_samples, member_params.data_ptr()))
        return real(itr, num_samples, member_params, env_update)

    sampler.obtain_samples = obtain_samples
    trainer = types.SimpleNamespace(
        step_epochs=lambda: iter(range(2)), step_itr=0, total_env_steps=0,
        _train_args=types.SimpleNamespace(batch_size=64))
    start = pop.member_params.clone()
    returns = pop.train(trainer)
    assert len(returns) == 3 and all(np.isfinite(r) for r in returns)
    assert trainer.step_itr == 2
    assert calls == [(0, 64, pop.member_params.data_ptr()),
                     (1, 64, pop.member_params.data_ptr())]
    assert trainer.total_env_steps == sampler.total_env_steps >= 2 * 3 * 64
    assert not torch.equal(start, pop.member_params)
    logged = logger.tabular.as_dict
    for m in range(3):
        assert 'member{}/Evaluation/AverageReturn'.format(m) in logged
        assert 'member{}/{}/LossAfter'.format(
            m, pop.members[m].policy.name) in logged
