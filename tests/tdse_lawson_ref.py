"""NumPy restatement of bspatom_tdse_lawson (include/bspatom.h): the integrating-factor form of tdse_ref.propagate's tableau, in a
real / complex dtype of the caller's choice.
    theta_s = E * (c_s * dt)   always in fp64 (c_s the double nearest the fraction), then cos / sin in the working dtype
    R_s = cos theta_s - i sin theta_s,  R_0 = 1
    w_s = a + dt sum_j A_sj kappa_j,  y_s = R_s w_s,  kappa_s = conj(R_s) (-i g_s),  g_s the coupling terms alone (no E y)
    a <- R_4 (a + dt sum_s d_s kappa_s),  err = max dt |sum_s (d_s - b_s) kappa_s|
Everything else follows tdse_ref.propagate, whose tableau and system() it uses.  Nothing here calls the library."""
import numpy as np

import tdse_ref
from tdse_ref import A, B, C, D5, _num


def propagate(E, pairs, D, a0, field, dt, rdtype=np.float64, cdtype=np.complex128, snap_every=0):
    """The arguments of tdse_ref.propagate: (a, err) or (a, err, snaps)."""
    E64 = np.asarray(E).astype(np.float64)
    D = np.asarray(D).astype(rdtype).reshape(len(pairs), E64.shape[1], E64.shape[1])
    a = np.asarray(a0).astype(cdtype)
    fld = np.asarray(field).astype(cdtype)
    dt64 = np.float64(dt)
    dt = rdtype(dt)
    mi, im = cdtype(-1j), cdtype(1j)
    nscan = a.shape[0]
    tabA = [[_num(x, rdtype) for x in row] for row in A]
    tabD = [_num(x, rdtype) for x in D5]
    tabE = [_num(x - y, rdtype) for x, y in zip(D5, B)]
    R = [None]
    for s in range(1, 6):
        theta = (E64 * (np.float64(C[s].numerator) / np.float64(C[s].denominator) * dt64)).astype(rdtype)
        R.append((np.cos(theta) - im * np.sin(theta)).astype(cdtype)[None])
    err = np.zeros(nscan, dtype=rdtype)
    snaps = []

    def coupling(y, f):
        g = np.zeros_like(y)
        for p, (i, j) in enumerate(pairs):
            g[:, j] += f[:, None] * (y[:, i] @ D[p])                     # (D_p^T a)[f] = sum_i D_p[i][f] a[i]
            g[:, i] += np.conj(f)[:, None] * (y[:, j] @ D[p].T)          # (D_p a)[i]   = sum_f D_p[i][f] a[f]
        return g

    for n in range(fld.shape[0]):
        k = []
        for s in range(6):
            y = a.copy()
            if s:
                y = R[s] * (a + dt * sum(tabA[s][j] * k[j] for j in range(s)))
            ks = mi * coupling(y, fld[n, s])
            k.append(np.conj(R[s]) * ks if s else ks)
        a = R[4] * (a + dt * sum(tabD[s] * k[s] for s in range(6)))
        e = dt * np.abs(sum(tabE[s] * k[s] for s in range(6)))
        err = np.maximum(err, e.reshape(nscan, -1).max(axis=1))
        if snap_every and (n + 1) % snap_every == 0:
            snaps.append(a.copy())
    return (a, err, np.array(snaps)) if snap_every else (a, err)


def both(E, pairs, D, a0, field, dt, **kw):
    """(complex128 result, long-double result) of propagate"""
    assert np.finfo(np.longdouble).eps < 2e-19
    return (propagate(E, pairs, D, a0, field, dt, np.float64, np.complex128, **kw),
            propagate(E, pairs, D, a0, field, dt, np.longdouble, np.clongdouble, **kw))


def stiff_system():
    """tdse_ref.system(3, 17, 2, 40) with the five highest states of every channel moved to 100 .. 400: dt max|E| = 20 at dt = 0.05"""
    E, pairs, D, a0, field = tdse_ref.system(3, 17, 2, 40)
    E = E.copy()
    E[:, 12:] = np.linspace(100.0, 400.0, 5)
    return E, pairs, D, a0, field
