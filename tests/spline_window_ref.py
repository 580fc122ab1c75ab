"""Restatements of bspatom_spline_window (csrc/spline_window.hip, include/bspatom_spline_window.h) for the tests:

    N = x_m^H S x_m,   x_0 = c,   x_{j+1} = (H - z_j S)^-1 S x_j,   P_m(E) = gamma^(2m) N with z = host.window_shifts(E, gamma, m)

norm_f64: the header's norm rule in float64 NumPy -- y = S x by rule 1, the lane-strided partial sums, the wave's tree; element-wise
IEEE operations, no FMA, no reassociation --, what the GPU returns bit for bit on a given x (W3, W5).  chain_dense, chain_banded and
spectral: three float64 CPU evaluations of N on dense (n, n) matrices, by numpy.linalg.solve, by scipy.linalg.solve_banded and by the
spectral sum over scipy.linalg.eigh's pairs: their largest pairwise difference is the reference noise delta_ref of the accuracy
criterion.  Plain NumPy / SciPy, importable without a GPU."""
import numpy as np
import scipy.linalg as sl

from spline_expect_ref import _lane_sums, wave_sum

EPS = float(np.finfo(np.float64).eps)


def overlap_f64(SF, x):
    """(y_re, y_im) of y = S x by rule 1: from +0.0, S(i, i + d) x(i + d) added for d ascending, columns outside the matrix skipped,
    multiply then add, the two components independently.  SF: the full band (2k-1, n) of S (host.band_symmetric(SB))."""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[0]
    b = (SF.shape[0] - 1) // 2
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    yr, yi = np.zeros(n), np.zeros(n)
    for d in range(-b, b + 1):
        lo, hi = max(0, -d), min(n, n - d)
        if hi <= lo:
            continue
        g = SF[d + b, lo:hi]
        yr[lo:hi] = yr[lo:hi] + g * xr[lo + d:hi + d]
        yi[lo:hi] = yi[lo:hi] + g * xi[lo + d:hi + d]
    return yr, yi


def norm_f64(SF, x):
    """x^H S x in the header's order: the N_ch of the spline rows on the vector x (n,) complex"""
    x = np.asarray(x, dtype=np.complex128)
    yr, yi = overlap_f64(SF, x)
    return float(wave_sum(_lane_sums(x.real * yr + x.imag * yi)))


def _band(M, b):
    """the (2b+1, n) LAPACK band of a dense matrix of half-width b: ab[b + i - j, j] = M[i, j]"""
    n = M.shape[0]
    ab = np.zeros((2 * b + 1, n), dtype=M.dtype)
    for d in range(-b, b + 1):
        i = np.arange(max(0, d), min(n, n + d))
        ab[b + d, i - d] = M[i, i - d]
    return ab


def chain_dense(H, S, c, z):
    """N for one packet c (n,) and the stages z (m,) by numpy.linalg.solve on the dense complex matrices"""
    x = np.asarray(c, dtype=np.complex128)
    for zj in np.asarray(z, dtype=np.complex128).reshape(-1):
        x = np.linalg.solve(H - zj * S, S @ x)
    return float(np.real(np.vdot(x, S @ x)))


def chain_banded(H, S, c, z, b):
    """the same by scipy.linalg.solve_banded on the band of half-width b"""
    x = np.asarray(c, dtype=np.complex128)
    for zj in np.asarray(z, dtype=np.complex128).reshape(-1):
        x = sl.solve_banded((b, b), _band(H - zj * S, b), S @ x)
    return float(np.real(np.vdot(x, S @ x)))


def eigen(H, S):
    """(w, X) of scipy.linalg.eigh(H, S): X^T S X = 1"""
    return sl.eigh(H, S)


def spectral(w, X, S, c, z):
    """N by the spectral sum: sum_n |x_n^T S c|^2 / prod_j |E_n - z_j|^2 -- with window_shifts' z this is
    sum_n |a_n|^2 / ((E_n - E)^(2m) + gamma^(2m))"""
    a = X.T @ (S @ np.asarray(c, dtype=np.complex128))
    den = np.ones_like(w)
    for zj in np.asarray(z, dtype=np.complex128).reshape(-1):
        den = den * np.abs(w - zj) ** 2
    return float(np.sum(np.abs(a) ** 2 / den))


def window_integral(m):
    """I_m = pi / (m sin(pi / 2m))"""
    return np.pi / (m * np.sin(np.pi / (2 * m)))
