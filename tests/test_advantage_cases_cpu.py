"""The tolerance of ``_advantage_cases.py`` against an fp32 restatement of the lone
arithmetic: the restatement stays within HALF of the bound on every case (CPU)."""
import numpy as np

import _advantage_cases as cases


def test_the_fp32_restatement_stays_within_half_of_the_bound():
    worst = 0.0
    for name, (P, members) in cases.CASES.items():
        for m, member in enumerate(members):
            rew, val = cases.inputs(name, m)
            for center, positive in cases.OPTIONS[1:]:
                raw, _, adv, _, _, scale = cases.reference(
                    rew, val, cases.lengths(member), P, member[2], member[3], center,
                    positive)
                got = cases.restate_f32(raw, center, positive)
                assert (np.isnan(got) == np.isnan(adv)).all(), (name, m)
                if np.isnan(adv).all():  # the one-sample batch: 0 / 0
                    assert len(adv) == 1 and center
                    continue
                ratio = np.abs(got - adv).max() / cases.bound(scale, center, positive)
                worst = max(worst, float(ratio))
    print('worst ratio', worst)
    assert 0.0 < worst <= 0.5

