"""A plain NumPy banded LU with partial pivoting in the rule of the device solvers (csrc/resolvent_shared.h: the largest |Re| + |Im|
among the rows j .. j + bw of column j, ties to the smallest row), with two fault knobs that restate what a wrong kernel would do:

  max_pivot_distance = d   the search sees the rows j .. j + d only (a truncated pivot search: a wave, a half of the window or a panel's
                           tail left out);
  fill_width = f           of the pivot row, U(j, j + 1 .. j + f) is kept and what lies beyond is dropped (the outer columns of the
                           window, the second register set of the backward pass, the second chunk of the trailing update left out).

Unmutated it is LU with partial pivoting of the dense matrix, as LAPACK's; the mutants are the evidence that a test would notice such a
kernel (test_resolvent_pivots_cpu.py, test_tdse_split_pivots_cpu.py).  No zero-pivot replacement: the matrices it solves with are
regular; factor() alone also takes a matrix with exactly zero columns (a zero pivot over a zero column is left where it is, its
multipliers are zero), so that the other pivots of such a matrix can be looked at."""
import numpy as np


def factor(M, bw, max_pivot_distance=None, fill_width=None):
    """(LU, piv, widest): M (N, N) complex, banded with half-width <= bw, in the ordering that is factored.  LU holds U on and above
    the diagonal and the multipliers below (row-interchanged as LAPACK's), piv[j] the row that came to j, widest the largest
    c - j over the nonzero U(j, c)."""
    A = np.array(M, dtype=np.complex128)
    N = A.shape[0]
    piv = np.zeros(N, dtype=np.int64)
    widest = 0
    for j in range(N):
        hi = min(N, j + bw + 1)
        cand = min(hi, j + (bw if max_pivot_distance is None else max_pivot_distance) + 1)
        col = A[j:cand, j]
        p = j + int(np.argmax(np.abs(col.real) + np.abs(col.imag)))   # argmax: the first of equal maxima
        piv[j] = p
        ce = min(N, j + 2 * bw + 1)
        if p != j:
            A[[j, p], j:ce] = A[[p, j], j:ce]
        if fill_width is not None:
            A[j, min(N, j + fill_width + 1):ce] = 0.0
        nz = np.nonzero(A[j, j:ce])[0]
        widest = max(widest, int(nz[-1]) if nz.size else 0)
        if hi > j + 1 and (A[j, j] != 0.0 or np.any(A[j + 1:hi, j] != 0.0)):
            lm = A[j + 1:hi, j] / A[j, j]
            A[j + 1:hi, j] = lm
            A[j + 1:hi, j + 1:ce] -= lm[:, None] * A[j, j + 1:ce][None, :]
    return A, piv, widest


def solve(M, b, bw, max_pivot_distance=None, fill_width=None):
    """x with M x = b by factor() and the two substitutions; b (N,) or (nrhs, N), x alike"""
    LU, piv, _ = factor(M, bw, max_pivot_distance, fill_width)
    return substitute(LU, piv, b, bw)


def substitute(LU, piv, b, bw):
    """the two substitutions of solve() on what factor() returned: a matrix factored once solves many right-hand sides"""
    N = LU.shape[0]
    y = np.array(np.asarray(b, dtype=np.complex128).reshape(-1, N).T)
    for j in range(N):
        p = piv[j]
        if p != j:
            y[[j, p]] = y[[p, j]]
        hi = min(N, j + bw + 1)
        y[j + 1:hi] -= LU[j + 1:hi, j][:, None] * y[j][None, :]
    for j in range(N - 1, -1, -1):
        ce = min(N, j + 2 * bw + 1)
        y[j] = (y[j] - LU[j, j + 1:ce] @ y[j + 1:ce]) / LU[j, j]
    return y.T.reshape(np.shape(b))


def lapack_profile(M):
    """(largest pivot distance, distances (N,), widest row of U, exact zeros on U's diagonal) of LAPACK's zgetrf on M: piv[j] - j where
    piv[j] is the row interchanged with j at step j (the rows a banded matrix offers at step j end at j + bw), and the largest
    c - j over the nonzero U(j, c) -- zeros outside the fill stay exact zeros in any order of the updates"""
    import scipy.linalg
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            LU, piv = scipy.linalg.lu_factor(np.asarray(M, dtype=np.complex128), check_finite=False)
    N = LU.shape[0]
    dist = piv - np.arange(N)
    U = np.triu(LU)
    cols = np.where(U != 0.0, np.arange(N)[None, :], -1).max(axis=1)
    widest = int(np.max(cols - np.arange(N)))
    return int(np.max(dist)), dist, widest, int(np.sum(np.diag(LU) == 0.0))
