"""What test_tdse_spline_wide_cpu.py and test_gpu_tdse_spline_wide.py share: the shapes of the GPU test, the launch-length rule of
bspatom_tdse_spline_wide restated in Python, and the Hermitian 17-channel system of the norm test with its evaluation on the dense
restatement tests/tdse_spline_ref.py."""
import numpy as np

import tdse_spline_ref as sref

EPS = np.finfo(np.float64).eps
DT = 0.05
NSCAN = 5
# (fixture, nch, nsteps, k, nfun): narrower than a panel; just past the old limit; N < 2 bw + 1; candidates over three waves; the limit
SHAPES = [("n65_k4", 3, 7, 4, 65), ("n65_k4", 17, 7, 4, 65), ("k16_n20", 5, 7, 16, 20), ("k16_n40", 9, 3, 16, 40), ("k16_n40", 16, 2, 16, 40)]
LAUNCH_FLOP = 27.6e9                       # two seconds at 13.8 Gflop/s per CU (include/bspatom_tdse_spline.h)


def launch_group(N, bw, nscan, slots):
    """the steps per launch of the wide call when tdse_spline_group is unset: the largest g in 1 .. 64 with
    g * ceil(nscan / slots) * 16 N bw^2 <= 27.6e9"""
    per_step = float(-(-nscan // slots)) * 16.0 * float(N) * float(bw) * float(bw)
    g = 64
    while g > 1 and g * per_step > LAUNCH_FLOP:
        g -= 1
    return g


# ---- the norm test: n65_k4, nch = 17 (bw = 67), every neighbour pair coupled in both directions on the bands of r and d/dr, the second
# direction as the transposed entry with the conjugate coefficient: block (c+1, c) is the conjugate transpose of block (c, c+1)
NORM_NCH, NORM_STEPS = 17, 5


def hermitian_system(nch=NORM_NCH, nsteps=NORM_STEPS):
    """(l, couplings, coef (nsteps, ncoup, 2)): channels l = c % 2; the pair (c, c+1) has a_c = 0.3 (1 + 0.3 i (-1)^c) on r and 0.02 i on
    d/dr, times a real pulse value per step"""
    l = [c % 2 for c in range(nch)]
    cp, a = [], []
    for c in range(nch - 1):
        ac = np.array([0.3 * (1.0 + 0.3j * (-1) ** c), 0.02j])
        cp += [(c, c + 1, 0), (c + 1, c, 1)]
        a += [ac, np.conj(ac)]
    F = 0.2 + 0.8 * np.sin(np.pi * (np.arange(nsteps) + 0.5) / nsteps) ** 2
    return l, cp, np.ascontiguousarray(F[:, None, None] * np.array(a)[None])


def norm_packet(n, nch=NORM_NCH):
    """one complex packet (nch, n) of unit scale, seeded"""
    rng = np.random.default_rng(1717)
    return (rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))) / np.sqrt(nch * n)


def norm_drift(rows, nch=NORM_NCH):
    """(max_j |sum_ch N_ch(j) - sum_ch N_ch(0)|, sum_ch N_ch(0)) of rows (nobs, >= nch)"""
    tot = np.asarray(rows)[:, :nch].sum(-1)
    return float(np.max(np.abs(tot - tot[0]))), float(tot[0])


def norm_drift_dense(SB, HB, G2, nch=NORM_NCH, nsteps=NORM_STEPS):
    """norm_drift of the dense restatement (tdse_spline_ref.propagate, numpy.linalg.solve) on the system above; G2: the full bands of r
    and d/dr, (2, 2k-1, n)"""
    l, cp, coef = hermitian_system(nch, nsteps)
    _, _, rows = sref.propagate(SB, HB, l, DT, norm_packet(SB.shape[1], nch), coef, cp, G2)
    return norm_drift(rows, nch)
