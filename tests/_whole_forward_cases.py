"""Case table and forward-only fp64 reference of the whole-network forwards that run in
one launch: ``mlp_eval_forward_kernel`` (fused_train.hip; ``ga_mlp_forward_f32`` with
``acts = NULL``) and ``mlp_train_fwd_fused_kernel`` (policy_fused.hip;
``ga_mlp_forward_fused_f32``).

Shared by ``test_whole_forward_cases_cpu.py`` (is fp32 itself close enough to fp64 on
these cases, and is the table what it claims?) and ``test_whole_forward_fp64_gpu.py``
(are the kernels?).

The draw, the reference and the tolerance are ``_mlp_option_cases``': parameters and
inputs that fp32 represents exactly, ``oracle.networks.mlp_mean`` on float64 copies of
them, ``TOL_FORWARD`` times ``max(1, max |ref|)``.  Nothing is differentiated: these
kernels have no backward.  Hidden layers are tanh, the output is linear, there is no
LayerNorm -- the kernels take nothing else.  For a case ``build`` yields

  out        the network outputs
  hidden.l   the output of hidden layer l

in fp64 (``ref``), and the largest deviation of the same quantities evaluated in fp32 on
the CPU (``dev32``).

The evaluation forward also has a width-64 instantiation (``<64, 2, 2>``).  No case
reaches it: ``ga_mlp_forward_eval_supported`` asks for both hidden widths >= 128 (the
per-layer kernels' 64 x 64 tiles are faster there), and the entry refuses what that
rule refuses.  It is left alone.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

from _mlp_option_cases import (PREFIX, TOL_FORWARD, _draw, _forward,  # noqa: F401
                               _rng, tolerance)

FT_ROWS = 64          # rows of a workgroup tile, both kernels
FT_W1_FLOATS = 5120   # shape_rules.h: LDS floats of the first layer's weights


def round4(v):
    return (int(v) + 3) // 4 * 4


# ---- the evaluation forward: (in_w, (K, width), A) and why the shape is in the table
EVAL_SHAPES = OrderedDict([
    # the C3 policy; KS = 5: the pipelined <256,1,8,5>; one lane of the last input quad live
    ('E1', (17, (256, 256), 6)),
    # KS = 5 with all four lanes live; A = 8, the most heads; K * ld0 = 5120, the LDS
    # bound exactly
    ('E2', (20, (256, 256), 8)),
    # KS = 4: the plain <256,1,8> at 256 units; A = 1, the value function
    ('E3', (16, (256, 256), 1)),
    # one input (min(k, in_w - 1) clamps every load), <128,1,4>
    ('E4', (1, (128, 128), 1)),
    # the widest input, KS = 8
    ('E5', (32, (128, 128), 3)),
    # five k-steps, an odd count: the other parity of the double-buffered operand; K > width
    ('E6', (9, (160, 128), 5)),
    # K * ld0 = 4608, the last ld0 the rule admits at K = 192; plain loop, KS = 6, K < width
    ('E7', (24, (192, 256), 2)),
    # the pipelined loop with four k-steps only; A = 7
    ('E8', (19, (128, 256), 7)),
    # K = 2 * width at 128 units
    ('E9', (5, (256, 128), 4)),
])
# the shapes whose first layer has five input quads: the pipelined instantiation
PIPELINED = ('E1', 'E2', 'E8')

# ---- the fused training forward: (in_w, hidden, A)
TRAIN_SHAPES = OrderedDict([
    # everything narrower than one k chunk or one column wave
    ('F1', (5, (16, 40), 3)),
    # K = 33: one element into a second 32-chunk; N = 100: ragged against 64-column
    # waves; one hidden layer
    ('F2', (33, (100, ), 2)),
    # the widest input and layer the rule admits (PS_HMAX); five layers; an 8-wide layer
    # between wide ones (the in-place tile must zero columns 8 .. 31); K = 130; the
    # widest head (32)
    ('F3', (256, (256, 64, 8, 130), 32)),
    # C3
    ('F4', (17, (256, 256), 6)),
    # no hidden layer: the head alone, called with acts = NULL
    ('F0', (3, (), 2)),
])
SHAPES = OrderedDict(list(EVAL_SHAPES.items()) + list(TRAIN_SHAPES.items()))

# (rows, gathered): 1; 64, one full tile; 65, a full tile and a tile with one live row;
# 191, two full tiles and one of 63 rows; 130 gathered WITH repeats out of 300
GATHER_M, GATHER_POOL = 130, 300
EVAL_ROWS = ((1, False), (64, False), (65, False), (191, False), (GATHER_M, True))
TRAIN_ROWS = ((1, False), (64, False), (65, False), (GATHER_M, True))

# one case = (shape, rows, gathered)
EVAL_CASES = [(s, ) + r for s in EVAL_SHAPES for r in EVAL_ROWS]
TRAIN_CASES = [(s, ) + r for s in ('F1', 'F2', 'F3', 'F4') for r in TRAIN_ROWS] + [
    ('F0', 65, False)]
# the one case at FlatMLP.EVAL_MIN_ROWS: ``forward(keep_acts=False)`` with the
# evaluation forward switched off and on
SWITCH_CASE = ('E1', 4096, False)
CASES = EVAL_CASES + TRAIN_CASES + [SWITCH_CASE]


def case_id(case):
    shape, M, gather = case
    return '{}-M{}{}'.format(shape, M, 'g' if gather else '')


def dims_of(case):
    in_w, hidden, A = SHAPES[case[0]]
    return (in_w, ) + tuple(hidden) + (A, )


def _acts(case):
    """What ``oc._forward`` reads of a case: (shape, hidden act, output act)."""
    return (case[0], 'tanh', 'none')


@functools.lru_cache(maxsize=None)
def _network(shape):
    """The parameters of a shape: shared by its row counts."""
    return _draw(_rng('whole-forward net', shape), dims_of((shape, )), False, False)


def _evaluate(case, params, rows, dtype):
    with torch.no_grad():
        p = OrderedDict((k, v.to(dtype)) for k, v in params.items())
        y, hidden, _ = _forward(_acts(case), p, rows.to(dtype))
    res = OrderedDict(out=y)
    for l, h in enumerate(hidden):
        res['hidden.%d' % l] = h
    return OrderedDict((k, t.to(torch.float64).numpy()) for k, t in res.items())


@functools.lru_cache(maxsize=4)
def build(case):
    """The inputs of ``case`` (fp32 tensors), its fp64 reference and its fp32 deviation.
    Results are shared: treat them as read-only.

    -> dict(params: state dict; X: the row pool; row_idx: int32 rows of the pool, repeats
    included, or None; ref: {name: float64 numpy}; dev32: {name: float})."""
    shape, M, gather = case
    dims = dims_of(case)
    params = _network(shape)
    rng = _rng('whole-forward rows', case)
    pool = GATHER_POOL if gather else M
    X = torch.from_numpy(rng.randn(pool, dims[0]).astype(np.float32))
    row_idx = rng.randint(0, pool, size=M).astype(np.int32) if gather else None
    rows = X if row_idx is None else X[torch.from_numpy(row_idx).long()]
    ref = _evaluate(case, params, rows, torch.float64)
    f32 = _evaluate(case, params, rows, torch.float32)
    dev32 = OrderedDict((k, float(np.abs(f32[k] - ref[k]).max())) for k in ref)
    return dict(params=params, X=X, row_idx=row_idx, ref=ref, dev32=dev32)
