"""Case table and fp64 reference of the MLP-option sweep.

Shared by ``test_mlp_option_cases_cpu.py`` (is fp32 itself close enough to fp64 on
these cases?) and ``test_mlp_options_fp64_gpu.py`` (are the per-layer HIP kernels?).

One reference: ``oracle.networks.mlp_mean`` -- dtype-agnostic, pinned to the real
reference's goldens -- on float64 copies of fp32-representable parameters and
inputs, differentiated by torch autograd.  For a case it yields

  out        the network outputs
  hidden.l   the output of hidden layer l
  grad.KEY   d sum(out * G) / d KEY for every tensor of the state dict
  jv         the forward-mode tangent J v of the outputs for a parameter tangent v

The same quantities evaluated in fp32 on the CPU give ``dev32``, the deviation
that fp32 arithmetic alone causes; the tolerances below are the suite's usual
figures, and the CPU test asserts that ``dev32`` stays under half of them.
"""
import functools
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import networks as nets

PREFIX = nets.POLICY_PREFIX

# FlatMLP.HIDDEN_ACTS / OUTPUT_ACTS in code order (the CPU test checks both)
HIDDEN_ACTS = ('tanh', 'relu', 'none', 'sigmoid', 'elu', 'leaky_relu', 'softplus')
OUTPUT_ACTS = ('none', 'tanh', 'relu', 'sigmoid', 'elu', 'leaky_relu', 'softplus')
TORCH_ACT = {'tanh': torch.tanh, 'relu': torch.relu, 'none': None,
             'sigmoid': torch.sigmoid, 'elu': F.elu, 'leaky_relu': F.leaky_relu,
             'softplus': F.softplus}
KINKED = ('relu', 'leaky_relu')

# (obs, hidden, act) and what the shape is for
SHAPES = OrderedDict([
    # every width below 4, one hidden layer, N <= 32 tiles only
    ('S1', (3, (5, ), 2)),
    # the FVP test's shape: the 33..64 tile, the streaming first layer, narrow-output
    # weight gradients
    ('S2', (11, (64, 32), 3)),
    # the 64x64x128 small-M tile against the 128x128 one, the fused head at 256, the
    # staged epilogue
    ('S3', (17, (256, 256), 6)),
    # three hidden layers, widths ragged against 32 / 64 / 128; K = 130: a ragged
    # second 128-deep k-step; LayerNorm at D = 40, 512, 96
    ('S4', (40, (512, 96, 130), 3)),
    # LayerNorm at its widest row (1024) and at 1000; 65: one lane past a wave;
    # K = 1024
    ('S5', (1024, (1000, 65), 3)),
    # no LayerNorm; first-layer K >= 128: the split-operand arm at M >= 1024 when the
    # suite runs in that mode
    ('S6', (376, (512, 512), 17)),
])

# rows per case: 1; 65; 128 (M % 64 == 0: the fused head); 333 gathered with repeats
# out of 500; 1101 (one active wave in the last LayerNorm block, a ragged row tile,
# M >= 1024)
ROWS = (1, 65, 128, 333, 1101)
GATHER_M, GATHER_POOL = 333, 500

KINK_MARGIN = 2e-5   # |fp64 pre-activation| of a kinked layer below this: resample
KINK_ROUNDS = 10

# per tensor, times max(1, max |ref|)
TOL_FORWARD = 5e-6   # fp32 results that differ in summation order only
TOL_GRAD = 1e-5      # test_mlp_forward_backward_vs_autograd's bound
TOL_JV = 1e-5


def tolerance(name, ref):
    """The absolute bound for the tensor ``name`` of a result dict."""
    rel = TOL_FORWARD if name == 'out' or name.startswith('hidden.') else (
        TOL_JV if name == 'jv' else TOL_GRAD)
    return rel * max(1.0, float(np.abs(ref).max()))


def _options():
    """[(shape, hidden_act, output_act, layer_norm)]."""
    out = []
    # S2, S3, S4: every hidden activation without and with LayerNorm; the output
    # activation walks through its codes, shifted per shape, so that every code occurs
    # once without and once with LayerNorm at each of these shapes
    for si, shape in enumerate(('S2', 'S3', 'S4')):
        for hi, h in enumerate(HIDDEN_ACTS):
            for ln in (False, True):
                out.append((shape, h, OUTPUT_ACTS[(hi + si) % len(OUTPUT_ACTS)], ln))
    # S1, S5 (LayerNorm on) and S6 (off): tanh, relu, softplus
    k = 0
    for shape, ln in (('S1', True), ('S5', True), ('S6', False)):
        for h in ('tanh', 'relu', 'softplus'):
            out.append((shape, h, OUTPUT_ACTS[k % len(OUTPUT_ACTS)], ln))
            k += 1
    return out


OPTIONS = _options()
# one case = one (shape, options, M)
CASES = [opt + (M, ) for opt in OPTIONS for M in ROWS]
# ga_mlp_backward_f32 called directly with more splits than the rows fill
ABI_CASE = ('S2', 'tanh', 'none', True, 100)


def case_id(case):
    shape, h, o, ln, M = case
    return '{}-{}-{}-{}-M{}'.format(shape, h, o, 'ln' if ln else 'noln', M)


def dims_of(case):
    O, hidden, A = SHAPES[case[0]]
    return (O, ) + tuple(hidden) + (A, )


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _draw(rng, dims, layer_norm, tangent):
    """A state dict (without the log-std slot) in the reference's key order:
    weights ~ N(0, 1 / fan_in), biases ~ 0.1 N(0, 1), gamma ~ 1 + 0.3 N(0, 1),
    beta ~ 0.3 N(0, 1); ``tangent``: the same scales around zero."""
    p = OrderedDict()
    nl = len(dims) - 1
    for l in range(nl):
        fan_in, fan_out = dims[l], dims[l + 1]
        if l < nl - 1:
            base = '{}_mean_module._layers.{}.linear.'.format(PREFIX, l)
            if layer_norm:
                ln = '{}_mean_module._layers.{}.layer_normalization.'.format(PREFIX, l)
                p[ln + 'weight'] = _f32((0.0 if tangent else 1.0) +
                                        0.3 * rng.randn(fan_in))
                p[ln + 'bias'] = _f32(0.3 * rng.randn(fan_in))
        else:
            base = PREFIX + '_mean_module._output_layers.0.linear.'
        p[base + 'weight'] = _f32(rng.randn(fan_out, fan_in) / np.sqrt(fan_in))
        p[base + 'bias'] = _f32(0.1 * rng.randn(fan_out))
    return p


class _Recorder:
    """A nonlinearity that keeps what went in and what came out."""

    def __init__(self, name):
        self.fn = TORCH_ACT[name]
        self.on = True
        self.pre, self.post = [], []

    def __call__(self, z):
        h = z if self.fn is None else self.fn(z)
        if self.on:
            self.pre.append(z)
            self.post.append(h)
        return h


def _forward(case, params, x, record=True):
    """-> (outputs, hidden outputs, pre-activations of hidden layers + output)."""
    hid, out = _Recorder(case[1]), _Recorder(case[2])
    hid.on = out.on = record
    with nets.hidden_nonlinearity(policy=hid), nets.output_nonlinearity(policy=out):
        y = nets.mlp_mean(params, PREFIX, x)
    return y, hid.post, hid.pre + out.pre


def _kinked_rows(case, params, x):
    """Rows of ``x`` (float64) with a pre-activation of a kinked layer inside the
    margin."""
    with torch.no_grad():
        _, _, pre = _forward(case, params, x)
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    n_hidden = len(pre) - 1
    for l, z in enumerate(pre):
        if case[1 if l < n_hidden else 2] in KINKED:
            bad |= (z.abs() < KINK_MARGIN).any(dim=1)
    return bad


def evaluate(case, params, tangent, x, G, dtype):
    """Every compared quantity of ``case`` in ``dtype`` -> {name: float64 numpy}."""
    p = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_(True))
                    for k, v in params.items())
    v = OrderedDict((k, t.to(dtype)) for k, t in tangent.items())
    x, G = x.to(dtype), G.to(dtype)
    y, hidden, _ = _forward(case, p, x)
    res = OrderedDict(out=y)
    for l, h in enumerate(hidden):
        res['hidden.%d' % l] = h
    grads = torch.autograd.grad((y * G).sum(), list(p.values()))
    for k, g in zip(p, grads):
        res['grad.' + k[len(PREFIX):]] = g
    frozen = OrderedDict((k, t.detach()) for k, t in p.items())
    _, res['jv'] = torch.func.jvp(
        lambda q: _forward(case, q, x, record=False)[0], (frozen, ), (v, ))
    return OrderedDict((k, t.detach().to(torch.float64).numpy())
                       for k, t in res.items())


@functools.lru_cache(maxsize=4)
def _network(shape, h, o, ln):
    """Parameters and the parameter tangent of one (shape, options): shared by its
    row counts."""
    dims = dims_of((shape, ))
    rng = _rng('net', shape, h, o, ln)
    return _draw(rng, dims, ln, False), _draw(rng, dims, ln, True)


@functools.lru_cache(maxsize=2)
def build(case):
    """The inputs of ``case`` (fp32 tensors), its fp64 reference and its fp32
    deviation.  Results are shared: treat them as read-only.

    -> dict(params, tangent: state dicts; X: the row pool; row_idx: int32 rows of the
    pool or None; G; ref, dev32: {name: ...}; kink_rounds: resampling rounds used)."""
    shape, h, o, ln, M = case
    dims = dims_of(case)
    params, tangent = _network(shape, h, o, ln)
    rng = _rng('rows', case)
    gather = M == GATHER_M
    pool = GATHER_POOL if gather else M
    X = rng.randn(pool, dims[0]).astype(np.float32)
    row_idx = rng.randint(0, pool, size=M).astype(np.int32) if gather else None
    zero_row = None
    if ln:
        # one row of all zeros: variance 0, rstd = 1 / sqrt(eps)
        zero_row = int(row_idx[rng.randint(M)]) if gather else int(rng.randint(M))
        X[zero_row] = 0.0
    G = _f32(rng.randn(M, dims[-1]))

    # no fp32 pre-activation of a kinked layer may fall on the other side of 0 from
    # the fp64 one: resample the rows that come close (all rows stay in the case)
    p64 = OrderedDict((k, t.double()) for k, t in params.items())
    rounds = 0
    while True:
        bad = _kinked_rows(case, p64, torch.from_numpy(X).double()).numpy()
        if not bad.any():
            break
        assert zero_row is None or not bad[zero_row], \
            'the all-zero row of %s lies on a kink' % case_id(case)
        rounds += 1
        if rounds > KINK_ROUNDS:
            break
        X[bad] = rng.randn(int(bad.sum()), dims[0]).astype(np.float32)
    Xt = torch.from_numpy(X)
    rows = Xt if row_idx is None else Xt[torch.from_numpy(row_idx).long()]
    ref = evaluate(case, params, tangent, rows, G, torch.float64)
    f32 = evaluate(case, params, tangent, rows, G, torch.float32)
    dev32 = OrderedDict((k, float(np.abs(f32[k] - ref[k]).max())) for k in ref)
    return dict(params=params, tangent=tangent, X=Xt, row_idx=row_idx, G=G, ref=ref,
                dev32=dev32, kink_rounds=rounds)
