"""NumPy restatement of the resolvent solve (csrc/resolvent.hip, bspatom_resolvent) for the tests: the dense complex matrix
M = H_l - i W - z S from the bands the caller sees, numpy.linalg.solve (LAPACK zgesv: partial pivoting), and the backward error in
clongdouble.  Also the CPU route to a band of g(r) on the assembly's quadrature (Cox-de Boor in NumPy), so that the physics of the
host helpers can be pinned without a GPU."""
import numpy as np

EPS = np.finfo(np.float64).eps
C_AU = 137.035999


def upper_to_dense(UB, dtype=np.float64):
    """symmetric (n, n) from the upper band UB[d, i] = A(i, i + d)"""
    k, n = UB.shape
    A = np.zeros((n, n), dtype=dtype)
    for d in range(k):
        i = np.arange(n - d)
        A[i, i + d] = UB[d, :n - d]
        A[i + d, i] = UB[d, :n - d]
    return A


def full_to_dense(FB, dtype=np.float64):
    """(n, n) from the full band FB[d + k - 1, i] = A(i, i + d), both triangles as given"""
    k, n = (FB.shape[0] + 1) // 2, FB.shape[1]
    A = np.zeros((n, n), dtype=dtype)
    for d in range(-(k - 1), k):
        i = np.arange(max(0, -d), min(n, n - d))
        A[i, i + d] = FB[d + k - 1, i]
    return A


def band_apply(A, X):
    """Y[j] = A x_j for the rows x_j of X (m, n); A (2k-1, n) with A[d + k - 1][i] = A(i, i + d)"""
    k, n = (A.shape[0] + 1) // 2, A.shape[1]
    Y = np.zeros_like(X)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)
        Y[:, lo:hi] += A[d + k - 1, lo:hi] * X[:, lo + d:hi + d]
    return Y


def dense_matrix(SB, HB, z, WB=None, dtype=np.complex128):
    """M = H - i W - z S; SB, HB upper bands (k, n), WB a full band (2k-1, n) or None.  dtype clongdouble: every entry formed in
    extended precision from the float64 bands (the matrix the backward error is measured against)."""
    real = np.longdouble if dtype == np.clongdouble else np.float64
    M = upper_to_dense(HB, real).astype(dtype) - dtype(z) * upper_to_dense(SB, real).astype(dtype)
    if WB is not None:
        M = M - dtype(1j) * full_to_dense(WB, real).astype(dtype)
    return M


def solve(SB, HB, z, B, WB=None):
    """X (nrhs, n): numpy.linalg.solve on the dense float64-complex matrix"""
    B = np.asarray(B, dtype=np.complex128).reshape(-1, SB.shape[1])
    return np.linalg.solve(dense_matrix(SB, HB, z, WB), B.T).T


def backward_error(SB, HB, z, x, b, WB=None):
    """omega = ||b - M x||_inf / (||M||_inf ||x||_inf + ||b||_inf) in clongdouble, M from the caller-visible bands"""
    M = dense_matrix(SB, HB, z, WB, np.clongdouble)
    x, b = np.asarray(x, dtype=np.clongdouble), np.asarray(b, dtype=np.clongdouble)
    r = b - M @ x
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(M), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))))


def norm_inverse(SB, HB, z, WB=None):
    """||M^-1||_inf of the dense reference"""
    return float(np.max(np.sum(np.abs(np.linalg.inv(dense_matrix(SB, HB, z, WB))), axis=1)))


# ---- the CPU route to the band of g(r): quadrature of the assembly, B-splines by Cox-de Boor ---------------------------------
def quadrature(rt, xg, wg):
    """points and weights of the assembly's Gauss-Legendre rule on the knot intervals of positive width (bspatom_quadrature)"""
    lo, hi = rt[:-1], rt[1:]
    keep = hi > lo
    f1, f2 = (hi[keep] + lo[keep]) / 2, (hi[keep] - lo[keep]) / 2
    return (f1[:, None] + xg[None, :] * f2[:, None]).ravel(), (f2[:, None] * wg[None, :]).ravel()


def bspline_table(rt, k, r):
    """B[j, q] = B_j(r_q), j < len(rt) - k, order k on the knots rt (points strictly inside the knot range)"""
    rt, r = np.asarray(rt, dtype=np.float64), np.asarray(r, dtype=np.float64)
    nk = rt.size
    B = np.array([(rt[j] <= r) & (r < rt[j + 1]) for j in range(nk - 1)], dtype=np.float64)
    for o in range(2, k + 1):
        Bn = np.zeros((nk - o, r.size))
        for j in range(nk - o):
            d1, d2 = rt[j + o - 1] - rt[j], rt[j + o] - rt[j + 1]
            if d1 > 0:
                Bn[j] += (r - rt[j]) / d1 * B[j]
            if d2 > 0:
                Bn[j] += (rt[j + o] - r) / d2 * B[j + 1]
        B = Bn
    return B


def operator_band(rt, k, xg, wg, g):
    """full band (2k-1, n) of G(i, j) = sum_q B_i(r_q) g(r_q) B_j(r_q) w_q; g a callable of the points"""
    r, w = quadrature(rt, xg, wg)
    B = bspline_table(rt, k, r)
    G = (B * (g(r) * w)) @ B.T
    n = B.shape[0]
    FB = np.zeros((2 * k - 1, n))
    for d in range(-(k - 1), k):
        i = np.arange(max(0, -d), min(n, n - d))
        FB[d + k - 1, i] = G[i, i + d]
    return FB


def cap_profile(r, r0, eta, power=2):
    return float(eta) * np.where(r > r0, r - r0, 0.0) ** power


def response(SB, HB_fin, z, b, p=None, WB=None):
    """p^T (H - i W - z S)^-1 b, bilinear"""
    x = solve(SB, HB_fin, z, b, WB)[0]
    return complex(np.sum((b if p is None else p) * x))


def sigma_h1s(omega):
    """photoionisation cross section of H(1s) in atomic units, closed form"""
    kap = np.sqrt(2.0 * omega - 1.0)
    return (2.0 ** 9 * np.pi ** 2 / (3.0 * C_AU)) * (2.0 * omega) ** -4 * np.exp(-4.0 * np.arctan(kap) / kap) / (1.0 - np.exp(-2.0 * np.pi / kap))
