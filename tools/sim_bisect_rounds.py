#!/usr/bin/env python3
"""sim_bisect_rounds.py -- how many evaluation rounds each workgroup of csrc/tridiag.hip::bisect3_kernel runs on a golden case's
spectra, in the exact-arithmetic model of tools/sim_grid.py (the spectrum stands in for the matrix): the lock-step rounds in `share`
mode up to the kernel's hand-over (at most NG / 8 brackets unfinished), then the kernel's multisection tail on the brackets handed over
(P = NG / K points inside each of the K brackets left, every round).  A round costs the same whoever runs it -- NG Sturm counts over
the whole matrix -- so the rounds are the workgroup's run time in units of one round; the first-level grid round (one more for every
workgroup) is not in the figures.  Prints one line per channel, `lock-step + tail` per workgroup x (eigenvalues 1024 x .. 1024 x + 1023),
and what the pairs (x, x + ceil(nw / 2)) of launch_bisect's paired launch add up to.
usage: python tools/sim_bisect_rounds.py [golden case [channel ...]]   (default: c4_4096_l127, channels 0 1 8 32 64 127)"""
import sys
import numpy as np
from sim_grid import NG, final, simulate, spectrum


def tail_rounds(lam, lo, hi, m):
    """rounds of the multisection tail on the brackets [lo, hi] of eigenvalues m (0-based numbers into lam, ascending)"""
    rounds = 0
    while len(m) and rounds < 128:
        K = len(m); P = NG // K
        w = hi - lo
        pts = lo[:, None] + w[:, None] * ((np.arange(P) + 1.0) / (P + 1.0))[None, :]
        cnt = np.searchsorted(lam, pts.ravel(), side="left").reshape(K, P)
        R = np.sum(cnt <= m[:, None], axis=1)               # first point with count > m (the counts of a bracket ascend); P: none
        nlo = np.where(R > 0, pts[np.arange(K), np.maximum(R - 1, 0)], lo)
        nhi = np.where(R < P, pts[np.arange(K), np.minimum(R, P - 1)], hi)
        keep = ~(final(nlo, nhi) | ~(nhi - nlo < w))
        lo, hi, m = nlo[keep], nhi[keep], m[keep]
        rounds += 1
    return rounds


def workgroup_rounds(lam, wg):
    _, left, (lams, lo, hi, m) = simulate(lam, "share", wg, stop=NG // 8)
    return len(left) - 1, tail_rounds(lams, lo, hi, m)


if __name__ == "__main__":
    case = sys.argv[1] if len(sys.argv) > 1 else "c4_4096_l127"
    chans = [int(a) for a in sys.argv[2:]] or [0, 1, 8, 32, 64, 127]
    for l in chans:
        lam = spectrum(case, l)
        nw = (len(lam) + NG - 1) // NG
        r = [workgroup_rounds(lam, wg) for wg in range(nw)]
        tot = [a + b for a, b in r]
        ps = (nw + 1) // 2
        pairs = [tot[x] + (tot[x + ps] if x + ps < nw else 0) for x in range(ps)]
        print("%s l %3d: lock-step + tail rounds by x: %s   totals %s   pairs (x, x + %d): %s" % (
            case, l, "  ".join("%d+%d" % ab for ab in r), tot, ps, pairs), flush=True)
