"""The forward + loss launch and the data-gradient launch of a fused optimizer step as
ONE launch (``ga_set_fused_fwd_dgrad``, fused_train.hip: ``fwd_dgrad_kernel``).

Every workgroup runs ``fwd_head_loss_body`` and then the data-gradient body on the same
64 rows; the last hidden layer's data gradient dZ2 stays in LDS between the two as the
k-contiguous A operand of a k-loop that takes its MFMAs in ``gemm_mainloop``'s order,
and the middle layer's split-K slabs are summed by the optimizer launch in the order
the data-gradient launch summed them.  Per element the arithmetic and its order are
those of the two launches, so a whole iteration must give the same BITS with the switch
on and off (for 256 units ``splits = ceil(M / 256)``, ``tiles = ceil(M / 64)``):

====  ======  =====  ============================================================
M     splits  tiles  what it exercises
====  ======  =====  ============================================================
64    1       1      one tile
65    1       2      a second tile of ONE live row: the masked dZ2 rows in LDS
300   2       5      a ragged tile of 44 rows
1300  6       21     runs that are not groups of four in the optimizer launch's sum
4096  16      64     whole tiles, the bench's dispatch
====  ======  =====  ============================================================

Every case trains a policy and a value function (head width 1).  The fused forward has
tanh hidden layers only, so there is no case with another activation.  Which steps take
the fused launch is pinned on the CPU (tests/host/update_loop_harness.cpp, suite fwd-dgrad).
"""
import numpy as np
import pytest
import torch

from test_fused_train_gpu import SHAPES, _algo, _problem

pytestmark = pytest.mark.gpu

# O, A, hidden, minibatch, discrete, algo keywords
for _m in (64, 65, 300, 1300, 4096):
    SHAPES['fwd_dgrad_m%d' % _m] = (17, 6, (256, 256), _m, False, {})
SHAPES['fwd_dgrad_obs1'] = (1, 6, (256, 256), 300, False, {})      # plain k-loop
SHAPES['fwd_dgrad_obs16'] = (16, 6, (256, 256), 300, False, {})    # plain k-loop
SHAPES['fwd_dgrad_obs20'] = (20, 6, (256, 256), 300, False, {})    # largest first layer
SHAPES['fwd_dgrad_categorical'] = (17, 2, (256, 256), 300, True, {})
SHAPES['fwd_dgrad_128_obs32'] = (32, 6, (128, 128), 300, False, {})
SHAPES['fwd_dgrad_128_obs17'] = (17, 6, (128, 128), 300, False, {})
SHAPES['fwd_dgrad_64'] = (17, 6, (64, 64), 300, False, {})  # (with the narrow step off)

_BATCHES = {}


def _batch(case):
    """One fixed batch per case, shared by the runs that compare on it."""
    if case not in _BATCHES:
        _BATCHES[case] = _problem(case)
    return _BATCHES[case]


def _run(case, on, overlap=None):
    from garage_amd import _lib
    lib = _lib.load()
    spec, batch = _batch(case)
    opt = (torch.optim.Adam, dict(lr=1e-3))
    lib.ga_set_fused_fwd_dgrad(on)
    algo, pol, vf = _algo(case, spec, opt, epochs=2)
    if overlap is not None:
        algo.overlap_updates = overlap
    np.random.seed(11)
    n0 = [int(lib.ga_launch_count(k)) for k in (9, 2, 10)]
    algo._train_once(0, batch)
    torch.cuda.synchronize()
    launches = tuple(int(lib.ga_launch_count(k)) - n for k, n in zip((9, 2, 10), n0))
    state = [t.clone() for net in (pol.net, vf.net)
             for t in (net.params, net.exp_avg, net.exp_avg_sq)]
    return state, dict(algo.last_tabular), launches


def _same_bits(case):
    from garage_amd import _lib
    lib = _lib.load()
    try:
        got = [_run(case, on) for on in (1, 0)]
    finally:
        lib.ga_set_fused_fwd_dgrad(1)
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert got[0][1] == got[1][1]
    for t in got[0][0]:
        assert bool(torch.isfinite(t).all())
    return got


@pytest.mark.parametrize('m', [64, 65, 300, 1300, 4096])
def test_fused_fwd_dgrad_is_bit_identical_to_the_two_launches(m):
    """Two epochs of ``PPO._train_once`` on one fixed batch, MLP(256, 256), obs 17
    (the pipelined k-loop), Gaussian policy (6 outputs) and value function (1):
    parameters, both Adam moments of both networks and the logged values, switch on
    against off."""
    case = 'fwd_dgrad_m%d' % m
    got = _same_bits(case)
    if m == 4096:
        # the counters count network steps, not dispatches: fused forward (9),
        # weight-gradient GEMM (2) and data gradient (10) advance once per step of each
        # of the two networks, in both modes
        S = int(_batch(case)[1].lengths.sum())
        steps = 2 * 2 * ((S + m - 1) // m)
        print('launch counts on / off:', got[0][2], got[1][2], 'steps', steps)
        assert got[0][2] == (steps, steps, steps), (got[0][2], steps)
        assert got[1][2] == (steps, steps, steps), (got[1][2], steps)


@pytest.mark.parametrize('case', ['obs1', 'obs16', 'obs20', 'categorical', '128_obs32',
                                  '128_obs17'])
def test_fused_fwd_dgrad_same_bits_at_other_shapes(case):
    """M = 300: first layers of 1, 16 (the plain k-loop, ``KSC = 0``) and 20 inputs (the
    largest one the 256-unit kernel holds), a categorical policy (2 outputs), and 128
    units (``fwd_dgrad_kernel<128,1,4,0>``) with 17 and with 32 inputs."""
    _same_bits('fwd_dgrad_' + case)


def test_fused_fwd_dgrad_same_bits_without_the_pipelined_kloop():
    """obs 17 with ``ga_set_pipelined_kloop(0)``: ``fwd_dgrad_kernel<256,1,8,0>`` at five
    first-layer k groups."""
    from garage_amd import _lib
    lib = _lib.load()
    try:
        lib.ga_set_pipelined_kloop(0)
        _same_bits('fwd_dgrad_m300')
    finally:
        lib.ga_set_pipelined_kloop(1)


def test_fused_fwd_dgrad_same_bits_at_64_units():
    """MLP(64, 64) with the narrow one-launch step switched off:
    ``fwd_dgrad_kernel<64,2,2,0>`` (two waves along the rows)."""
    from garage_amd import _lib
    lib = _lib.load()
    try:
        lib.ga_set_narrow_step(0)
        got = _same_bits('fwd_dgrad_64')
    finally:
        lib.ga_set_narrow_step(1)
    # the wide step's launches were taken (kinds 9 and 10), and as often either way
    assert got[0][2][0] > 0 and got[0][2][2] > 0 and got[0][2] == got[1][2], got


def test_fused_fwd_dgrad_two_streams_and_one_stream_are_the_same_bits():
    """The switch on: the two-stream schedule (``overlap_updates=True``, each network's
    fused launches on its own stream) against the serial one."""
    from garage_amd import _lib
    lib = _lib.load()
    try:
        got = [_run('fwd_dgrad_m1300', 1, overlap=o) for o in (True, False)]
    finally:
        lib.ga_set_fused_fwd_dgrad(1)
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert got[0][1] == got[1][1]
