"""tools/sim_bisect_rounds.py: the round counts behind the paired launch of bisect3_kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rounds_of_channel_0_of_the_bench_spectra():
    """Channel 0 of tests/golden/c4_4096_l127.npz, lock-step + tail rounds of the four workgroups as DESIGN.md 4.3 tabulates them: the
    quarter next to zero (x = 3) costs the most, and the pairs (0, 2) and (1, 3) are closer to each other than (3, 3) is to (1, 1)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sim_bisect_rounds as sb
    finally:
        sys.path.pop(0)
    lam = sb.spectrum("c4_4096_l127", 0)
    r = [sb.workgroup_rounds(lam, wg) for wg in range(4)]
    assert r == [(12, 8), (12, 4), (13, 4), (17, 7)]


def test_tail_model_on_one_bracket():
    """One bracket of width 1 around one eigenvalue, 1024 points a round: every round shrinks it 1025-fold until it is final."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sim_bisect_rounds as sb
    finally:
        sys.path.pop(0)
    lam = np.array([-1.0, 0.3, 1.0])
    rounds = sb.tail_rounds(lam, np.array([0.0]), np.array([1.0]), np.array([1]))
    assert rounds == 6          # 1025^-5 = 8.8e-16 is not yet below 2 eps |x| = 1.3e-16; the sixth round's bracket is
