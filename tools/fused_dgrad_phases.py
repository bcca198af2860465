"""Phase timestamps and launch skew of the data-gradient body (fused_train.hip): of
dgrad_wgrad0_kernel, or -- with the fused forward + data-gradient launch on, the default --
of the second half of fwd_dgrad_kernel, whose stamps 5 and 6 split two of the phases.
    python tools/fused_dgrad_phases.py [config [minibatches per epoch]]
(GA_VARIANT_LIB: another build of the library; 64 minibatches: 256 tiles, one workgroup
per CU)"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from garage_amd import _lib
if os.environ.get('GA_VARIANT_LIB'):
    _lib.LIB_PATH = os.path.abspath(os.environ['GA_VARIANT_LIB'])
lib = _lib.load()
cfg = dict(bench.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else 'c3'])
if len(sys.argv) > 2:
    cfg['minibatches'] = int(sys.argv[2])
algo, sampler, pol, S = bench.build_engine(cfg, None)
algo.overlap_updates = False
eps = sampler.obtain_samples(0, S, None)
algo._train_once(0, eps)
buf = (C.c_longlong * 16)()
assert lib.ga_fused_dgrad_debug(buf, 0, 0) == 1
algo._train_once(1, eps)
assert lib.ga_fused_dgrad_debug(buf, 0, 0) == 0
s = np.array(list(buf), dtype=np.int64)
if s[5] and s[6]:  # fwd_dgrad_kernel of a build that has stamps 5 and 6
    t = s[[0, 5, 1, 6, 2, 3, 4]]
    names = ['X loads, zero accumulators, barrier', 'k-loop (dZ2 W2, dZ2 staged)',
             'fences, barrier, issue of the H1 loads', 'stage accumulators, X rows, barrier',
             'dZ1 = . (1 - H1^2): waits for H1', 'first-layer grad shares']
else:
    t = s[:5]
    names = ['k-loop (dZ2 W2)', 'stage accumulators, X rows',
             'dZ1 = . (1 - H1^2), H1 from memory', 'first-layer grad shares']
for n, d in zip(names, np.diff(t)):
    print('%-40s %6.2f us' % (n, d / 100.0))
print('total                                    %6.2f us' % ((t[-1] - t[0]) / 100.0))
n = min(512, (S // bench.n_minibatches(cfg) + 63) // 64)
sk = (C.c_longlong * (3 * n))()
assert lib.ga_fused_dgrad_debug(sk, 1, n) == 0
a = np.array(list(sk), dtype=np.int64).reshape(n, 3) / 100.0
t0 = a[:, 0].min()
for name, col in (('workgroup starts', 0), ('k-loop ends', 1), ('workgroup ends', 2)):
    print('%-18s: min %.2f  median %.2f  max %.2f us' % (
        name, a[:, col].min() - t0, np.median(a[:, col]) - t0, a[:, col].max() - t0))
