"""The middle layer's split-K weight-gradient slabs summed inside the data-gradient
launch (``ga_set_slab_sum_in_dgrad``, fused_train.hip: ``FtSlabSummer``).

``dgrad_wgrad0_kernel`` runs, on the side, the summation tree that
``reduce_regions_adam_kernel`` runs for a region of up to 128 partials -- four shares
of contiguous runs, groups of four, ``(a0 + a1) + (a2 + a3)`` -- writes every sum over
partial 0, and the optimizer launch then reads that one partial.  The order of
additions per element is the same, so a whole iteration must give the same BITS with
the switch on and off, at every minibatch size that takes another branch of the sum
(for 256 units ``splits = ceil(M / 256)``, ``tiles = ceil(M / 64)``):

====  ======  =====  ==========================================================
M     splits  tiles  what it exercises
====  ======  =====  ==========================================================
64    1       1      nothing folded: the guard
300   2       5      fewer partials than shares; ragged last tile of 44 rows
1300  6       21     not a multiple of four: runs of 2, 2, 2, 0; ragged tile
4096  16      64     whole tiles, a group of four per share (the bench's path)
====  ======  =====  ==========================================================

That the ranges are handed over at all (and only then) is pinned on the CPU
(tests/host/update_loop_harness.cpp, suite slab-sum).
"""
import numpy as np
import pytest
import torch

from test_fused_train_gpu import SHAPES, _algo, _problem

pytestmark = pytest.mark.gpu

# O, A, hidden, minibatch, discrete, algo keywords (the bench's networks: obs 17, act 6,
# tanh MLP(256, 256))
for _m in (64, 300, 1300, 4096):
    SHAPES['slab_sum_m%d' % _m] = (17, 6, (256, 256), _m, False, {})
SHAPES['slab_sum_128_m1300'] = (17, 6, (128, 128), 1300, False, {})
SHAPES['slab_sum_uneven'] = (17, 6, (256, 256), 700, False, {})

_BATCHES = {}


def _batch(case, lens=None):
    """One fixed batch per case, shared by the tests that need it."""
    if case not in _BATCHES:
        _BATCHES[case] = _problem(case, lens=lens)
    return _BATCHES[case]


def _run(case, on, merged=0, lens=None, count=False):
    from garage_amd import _lib
    lib = _lib.load()
    spec, batch = _batch(case, lens)
    opt = (torch.optim.Adam, dict(lr=1e-3))
    lib.ga_set_slab_sum_in_dgrad(on)
    lib.ga_set_merged_pair(merged)
    algo, pol, vf = _algo(case, spec, opt, epochs=2)
    np.random.seed(11)
    n0 = [int(lib.ga_launch_count(k)) for k in (9, 2, 10)]
    algo._train_once(0, batch)
    torch.cuda.synchronize()
    launches = tuple(int(lib.ga_launch_count(k)) - n for k, n in zip((9, 2, 10), n0))
    state = [t.clone() for net in (pol.net, vf.net)
             for t in (net.params, net.exp_avg, net.exp_avg_sq)]
    return state, dict(algo.last_tabular), launches


def _same_bits(case, merged=0, lens=None):
    from garage_amd import _lib
    lib = _lib.load()
    try:
        got = [_run(case, on, merged=merged, lens=lens) for on in (1, 0)]
    finally:
        lib.ga_set_slab_sum_in_dgrad(1)
        lib.ga_set_merged_pair(0)
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert got[0][1] == got[1][1]
    return got


@pytest.mark.parametrize('m', [64, 300, 1300, 4096])
def test_slab_sum_in_dgrad_is_bit_identical_to_the_optimizer_launch_sum(m):
    """Two epochs of ``PPO._train_once`` on one fixed batch, MLP(256, 256): parameters,
    both Adam moments of both networks and the logged values, switch on against off."""
    got = _same_bits('slab_sum_m%d' % m)
    if m == 4096:
        # the launches are the same four: fused forward (9), weight-gradient GEMM (2),
        # data gradient (10)
        assert got[0][2] == got[1][2], (got[0][2], got[1][2])
        assert all(n > 0 for n in got[0][2]), got[0][2]


def test_slab_sum_in_dgrad_same_bits_when_minibatches_differ_in_size():
    """1640 samples in minibatches of 700, 700 and 240 rows: the number of partials
    (3, 3, 1 -- the last step folds nothing) and the number of workgroups that share
    the quads (11, 11, 4) change from step to step."""
    _same_bits('slab_sum_uneven', lens=[40] * 41)


def test_slab_sum_in_dgrad_same_bits_at_128_units():
    """MLP(128, 128) at M = 1300: ``dgrad_wgrad0_kernel<128,1,4>`` (four waves, four
    k-steps)."""
    _same_bits('slab_sum_128_m1300')


def test_slab_sum_in_dgrad_same_bits_in_the_merged_pair_schedule():
    """``ga_set_merged_pair(1)`` at M = 1300: the pair kernels sum both networks'
    slabs in one grid."""
    _same_bits('slab_sum_m1300', merged=1)
