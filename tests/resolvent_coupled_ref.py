"""NumPy restatement of the coupled-channel resolvent (csrc/resolvent_coupled.hip, bspatom_resolvent_coupled) for the tests: the
dense complex matrix of nch coupled channels from the bands the caller sees (resolvent_ref.dense_matrix for the diagonal blocks,
resolvent_ref.full_to_dense for the operator bands), numpy.linalg.solve on it IN THE DOCUMENTED ORDERING (unknown (i, c) at position
i nch + c: LAPACK's partial pivoting then meets the band the kernel factors), and the backward error in clongdouble.  Matrices here
are channel-major (block (c, c') in rows c n .., columns c' n ..) unless a name says interleaved."""
import numpy as np

import resolvent_ref as ref

EPS = ref.EPS


def interleave_index(nch, n):
    """idx[i * nch + c] = c * n + i: the channel-major index of the unknown at position i nch + c"""
    i, c = np.divmod(np.arange(nch * n), nch)
    return c * n + i


def dense_matrix(SB, HB, l, z, couplings=(), G=None, a=None, WB=None, w=None, dtype=np.complex128):
    """Channel-major (nch n, nch n): diagonal block c = H_l[c] - i W_w[c] - z[c] S (w None: WB[0] on every channel if WB is given;
    w[c] = -1: none), and entry p = (cr, cc, ctr) of couplings adds sum_o a[p, o] G[o], transposed where ctr, to block (cr, cc).
    HB[l] is channel l; WB (nabs, 2k-1, n), G (nop, 2k-1, n) full bands; a (ncoup, nop) complex."""
    real = np.longdouble if dtype == np.clongdouble else np.float64
    n, nch = SB.shape[1], len(l)
    M = np.zeros((nch * n, nch * n), dtype=dtype)
    for c in range(nch):
        wc = (0 if WB is not None else -1) if w is None else int(w[c])
        M[c * n:(c + 1) * n, c * n:(c + 1) * n] = ref.dense_matrix(SB, HB[l[c]], complex(z[c]), WB[wc] if wc >= 0 else None, dtype)
    if len(couplings):
        Gd = [ref.full_to_dense(g, real) for g in G]
        a = np.asarray(a, dtype=np.complex128).reshape(len(couplings), len(Gd))
        for p, (cr, cc, ctr) in enumerate(couplings):
            blk = M[cr * n:(cr + 1) * n, cc * n:(cc + 1) * n]
            for o, g in enumerate(Gd):
                blk += dtype(a[p, o]) * (g.T if ctr else g).astype(dtype)
    return M


def solve(M, B, nch):
    """X (nrhs, nch, n): numpy.linalg.solve on the float64-complex matrix in the interleaved ordering; M channel-major, B (nrhs, nch, n)"""
    n = M.shape[0] // nch
    idx = interleave_index(nch, n)
    Bf = np.asarray(B, dtype=np.complex128).reshape(-1, nch * n)
    Xi = np.linalg.solve(M[np.ix_(idx, idx)], Bf[:, idx].T).T
    X = np.zeros_like(Bf)
    X[:, idx] = Xi
    return X.reshape(-1, nch, n)


def backward_error(Ml, x, b):
    """omega = ||b - M x||_inf / (||M||_inf ||x||_inf + ||b||_inf) in clongdouble; Ml the clongdouble channel-major matrix"""
    x, b = np.asarray(x, dtype=np.clongdouble).ravel(), np.asarray(b, dtype=np.clongdouble).ravel()
    r = b - Ml @ x
    return float(np.max(np.abs(r)) / (np.max(np.sum(np.abs(Ml), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))))


def half_width(M, nch):
    """max |row - column| over the nonzero entries of the interleaved matrix"""
    n = M.shape[0] // nch
    idx = interleave_index(nch, n)
    r, c = np.nonzero(M[np.ix_(idx, idx)])
    return int(np.max(np.abs(r - c)))


def stark_series(E1s, F):
    """E_1s - (9/4) F^2 - (3555/64) F^4 - (2512779/512) F^6: hydrogen's ground level in a static field, atomic units"""
    return E1s - 2.25 * F ** 2 - (3555.0 / 64.0) * F ** 4 - (2512779.0 / 512.0) * F ** 6
