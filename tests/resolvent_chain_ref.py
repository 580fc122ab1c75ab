"""NumPy restatement of the resolvent chain (csrc/resolvent.hip: resolvent_chain_kernel, bspatom_resolvent_chain) for the tests:
the band apply between two stages in exactly the arithmetic include/bspatom.h fixes -- real operations on separate Re and Im
arrays, one NumPy ufunc call per operation, in the stated order; no complex multiply, no `@`, nothing NumPy could fuse or
reassociate -- and the chain composed of it and resolvent_ref.solve (dense LAPACK)."""
import numpy as np

import resolvent_ref as ref


def band_combine_apply(GB, a, X):
    """Y[j] = A x_j for the rows x_j of X (m, n) complex (or real), A = sum_o a[o] G_o, GB (nop, 2k-1, n) full bands with
    GB[o, d + k - 1, i] = G_o(i, i + d).  An entry is t = a[0] * G_0(i, i + d), then t = t + a[o] * G_o(i, i + d) for o ascending;
    y_re(i) starts at +0.0 and adds t * x_re(i + d) for d = -(k-1) .. k-1 ascending, columns outside 0 .. n-1 skipped; y_im likewise
    from x_im.  Returns complex128 (m, n)."""
    GB = np.asarray(GB, dtype=np.float64)
    GB = GB.reshape((-1,) + GB.shape[-2:])
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    assert a.shape == (GB.shape[0],), (a.shape, GB.shape)
    X = np.asarray(X)
    X = X.reshape(-1, X.shape[-1])
    xr = np.ascontiguousarray(X.real, dtype=np.float64)
    xi = np.ascontiguousarray(X.imag, dtype=np.float64) if np.iscomplexobj(X) else np.zeros_like(xr)
    k, n = (GB.shape[1] + 1) // 2, GB.shape[2]
    yr, yi = np.zeros_like(xr), np.zeros_like(xr)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)                     # rows i with 0 <= i + d < n
        if hi <= lo:
            continue
        t = np.multiply(a[0], GB[0, d + k - 1, lo:hi])
        for o in range(1, GB.shape[0]):
            t = np.add(t, np.multiply(a[o], GB[o, d + k - 1, lo:hi]))
        yr[:, lo:hi] = np.add(yr[:, lo:hi], np.multiply(t, xr[:, lo + d:hi + d]))
        yi[:, lo:hi] = np.add(yi[:, lo:hi], np.multiply(t, xi[:, lo + d:hi + d]))
    Y = np.empty(xr.shape, dtype=np.complex128)
    Y.real, Y.imag = yr, yi
    return Y


def chain(SB, HB, l, z, B, GB=None, a=None, WB=None, w=None):
    """One chain on the CPU: the list of the stages' solutions x_s (nrhs, n), x_0 = M_0^-1 B, x_s = M_s^-1 (A_s x_{s-1}) with
    M_s = HB[l[s]] - i W - z[s] S by resolvent_ref.solve and A_s = sum_o a[s-1, o] GB[o] by band_combine_apply.  HB (nl, k, n) upper
    bands indexed by l[s]; WB one full band or None; w[s] = -1 switches it off for stage s (None: on everywhere)."""
    l, z = np.atleast_1d(l), np.atleast_1d(z)
    xs = []
    y = np.asarray(B, dtype=np.complex128).reshape(-1, SB.shape[1])
    for s in range(len(z)):
        if s:
            y = band_combine_apply(GB, np.asarray(a, dtype=np.float64).reshape(len(z) - 1, -1)[s - 1], xs[-1])
        Ws = WB if (WB is not None and (w is None or w[s] >= 0)) else None
        xs.append(ref.solve(SB, HB[l[s]], z[s], y, Ws))
    return xs
