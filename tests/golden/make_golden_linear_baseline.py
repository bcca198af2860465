"""Generate ``linear_feature_baseline.npz`` by running the REAL reference
``garage.np.baselines.LinearFeatureBaseline``.

Run in the build container only (needs the reference checkout that
``_ref_harness.py`` imports)::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_linear_baseline.py

For every case of ``tests/_linear_baseline_cases.py`` the real class is handed
float64 copies of the case's fp32 observations and returns as ``paths``.  Written
per case (plain arrays only): ``<case>/features`` (``_features`` of every path,
concatenated; of the rows ``<case>/feature_rows`` only -- every k-th and the last
three -- where the whole matrix would be large), ``<case>/coeffs`` after ``fit``, ``<case>/predictions``
(``predict`` of every path, concatenated) and ``<case>/before`` (``predict`` of
the first path before any fit).  ``--check DIR`` writes into DIR instead.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_harness as ref  # noqa: E402

ref.install()

from garage.np.baselines import LinearFeatureBaseline  # noqa: E402

import _linear_baseline_cases as cases  # noqa: E402

OUT = HERE


def gen():
    out = {}
    for name in cases.CASE_NAMES:
        obs, returns, lengths = cases.make_inputs(name)
        paths = cases.paths_of(obs, returns, lengths)
        baseline = LinearFeatureBaseline(None, reg_coeff=cases.REG_COEFF)
        out[name + '/before'] = np.asarray(baseline.predict(paths[0]))
        feats = np.concatenate([baseline._features(p) for p in paths])
        rows = cases.golden_feature_rows(*feats.shape)
        out[name + '/feature_rows'] = rows
        out[name + '/features'] = feats[rows]
        baseline.fit(paths)
        out[name + '/coeffs'] = np.asarray(baseline.get_param_values())
        out[name + '/predictions'] = np.concatenate(
            [baseline.predict(p) for p in paths])
    path = os.path.join(OUT, 'linear_feature_baseline.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--check':
        OUT = sys.argv[2]
    gen()
