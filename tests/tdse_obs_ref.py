"""NumPy restatement of the observables of bspatom_tdse_observe (include/bspatom.h), straight from their definitions, in a real /
complex dtype of the caller's choice, and the magnitudes that bound the rounding error of any summation order.  Nothing here calls
the library.

    pop_c = sum_n |a_c[n]|^2,  sum_n E_c[n] |a_c[n]|^2,  z_c = sum_{p: cf[p] = c} sum_{i,f} conj(a_cf[f]) D_p[i][f] a_ci[i]
"""
import numpy as np


def _args(E, pairs, D, a, rdtype, cdtype):
    E = np.asarray(E).astype(rdtype)
    nch, count = E.shape
    D = np.asarray(D).astype(rdtype).reshape(len(pairs), count, count)
    a = np.asarray(a).astype(cdtype)
    lead = a.shape[:-2]
    assert a.shape[-2:] == (nch, count), (a.shape, E.shape)
    return E, D, a.reshape((-1, nch, count)), lead, nch


def observables(E, pairs, D, a, rdtype=np.float64, cdtype=np.complex128):
    """E (nch, count), pairs [(ci, cf)], D (npairs, count, count), a (..., nch, count): (..., nch, 4) = pop, sum E |a|^2, Re z_c, Im z_c"""
    E, D, a, lead, nch = _args(E, pairs, D, a, rdtype, cdtype)
    out = np.zeros((a.shape[0], nch, 4), dtype=rdtype)
    p2 = a.real * a.real + a.imag * a.imag
    out[:, :, 0] = p2.sum(axis=-1)
    out[:, :, 1] = (E[None] * p2).sum(axis=-1)
    for p, (i, f) in enumerate(pairs):
        z = np.sum(np.conj(a[:, f]) * (a[:, i] @ D[p]), axis=-1)          # (a_i @ D_p)[f] = sum_i D_p[i][f] a_i[i]
        out[:, f, 2] += z.real
        out[:, f, 3] += z.imag
    return out.reshape(lead + (nch, 4))


def magnitudes(E, pairs, D, a):
    """M_k, k = 0 .. 3, in long double: the largest over the rows (leading index of a, channel) of the sum of the moduli of the real
    terms of component k -- a_re^2, a_im^2; E a_re^2, E a_im^2; a_re[f] D a_re[i], a_im[f] D a_im[i]; a_re[f] D a_im[i], a_im[f] D a_re[i].
    Any summation order over at most n chained additions is within n eps M_k of the exact sum (to first order in eps)."""
    E, D, a, _, nch = _args(E, pairs, D, a, np.longdouble, np.clongdouble)
    m = np.zeros((a.shape[0], nch, 4), dtype=np.longdouble)
    ar, ai, aD = np.abs(a.real), np.abs(a.imag), np.abs(D)
    p2 = ar * ar + ai * ai
    m[:, :, 0] = p2.sum(axis=-1)
    m[:, :, 1] = (np.abs(E)[None] * p2).sum(axis=-1)
    for p, (i, f) in enumerate(pairs):
        ur, ui = ar[:, i] @ aD[p], ai[:, i] @ aD[p]
        m[:, f, 2] += np.sum(ar[:, f] * ur + ai[:, f] * ui, axis=-1)
        m[:, f, 3] += np.sum(ar[:, f] * ui + ai[:, f] * ur, axis=-1)
    return m.reshape(-1, 4).max(axis=0)
