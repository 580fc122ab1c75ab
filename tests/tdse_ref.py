"""NumPy restatement of bspatom_tdse_propagate (include/bspatom.h): the equation, the six-stage embedded Runge-Kutta pair and the
field table, in a real / complex dtype of the caller's choice.  The tests run it twice, in complex128 and in long double (64-bit
mantissa), and bound the library's distance from the long-double result by 8 times the complex128 restatement's own:
    max|a_gpu - a_long| <= 8 max(max|a_128 - a_long|, eps)
(a different but equally stable summation order: MFMA K order and FMA against NumPy's sums).  Nothing here calls the library."""
import numpy as np
from fractions import Fraction as F

EPS = float(np.finfo(np.float64).eps)

A = ((), (F(2, 9),), (F(1, 12), F(1, 4)), (F(69, 128), F(-243, 128), F(135, 64)), (F(-17, 12), F(27, 4), F(-27, 5), F(16, 15)),
     (F(65, 432), F(-5, 16), F(13, 16), F(4, 27), F(5, 144)))
B = (F(1, 9), F(0), F(9, 20), F(16, 45), F(1, 12), F(0))
C = (F(0), F(2, 9), F(1, 3), F(3, 4), F(1), F(5, 6))
D5 = (F(47, 450), F(0), F(12, 25), F(32, 225), F(1, 30), F(6, 25))


def _num(x, rdtype):
    return rdtype(x.numerator) / rdtype(x.denominator)


def propagate(E, pairs, D, a0, field, dt, rdtype=np.float64, cdtype=np.complex128, snap_every=0):
    """E (nch, count), pairs [(ci, cf)], D (npairs, count, count), a0 (nscan, nch, count), field (nsteps, 6, nscan):
    (a, err) or (a, err, snaps)."""
    E = np.asarray(E).astype(rdtype)
    D = np.asarray(D).astype(rdtype).reshape(len(pairs), E.shape[1], E.shape[1])
    a = np.asarray(a0).astype(cdtype)
    fld = np.asarray(field).astype(cdtype)
    dt = rdtype(dt)
    mi = cdtype(-1j)
    nscan = a.shape[0]
    tabA = [[_num(x, rdtype) for x in row] for row in A]
    tabD = [_num(x, rdtype) for x in D5]
    tabE = [_num(x - y, rdtype) for x, y in zip(D5, B)]
    err = np.zeros(nscan, dtype=rdtype)
    snaps = []

    def rhs(y, f):
        h = E[None] * y
        for p, (i, j) in enumerate(pairs):
            h[:, j] += f[:, None] * (y[:, i] @ D[p])                     # (D_p^T a)[f] = sum_i D_p[i][f] a[i]
            h[:, i] += np.conj(f)[:, None] * (y[:, j] @ D[p].T)          # (D_p a)[i]   = sum_f D_p[i][f] a[f]
        return mi * h

    for n in range(fld.shape[0]):
        k = []
        for s in range(6):
            y = a.copy()
            if s:
                y = a + dt * sum(tabA[s][j] * k[j] for j in range(s))
            k.append(rhs(y, fld[n, s]))
        a = a + dt * sum(tabD[s] * k[s] for s in range(6))
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


def amp_bound(a128, along):
    return 8.0 * max(float(np.max(np.abs(a128.astype(np.clongdouble) - along))), EPS)


def err_bound(e128, elong, dt):
    return 8.0 * max(float(np.max(np.abs(e128.astype(np.longdouble) - elong))), EPS * dt)


def system(nch, count, nscan, nsteps, pairs=None, seed=0, dt=0.05, phase=0.0):
    """The test problem of the GPU tests: random E sorted in (-0.5, 2), D standard normal / sqrt(count) on a chain of channels
    (or `pairs`), a0 random of norm 1 per scan, a sin^2-enveloped carrier with per-scan amplitudes (times exp(i phase))."""
    rng = np.random.default_rng(1000 * nch + 10 * count + nscan + seed)
    E = np.sort(rng.uniform(-0.5, 2.0, size=(nch, count)), axis=1)
    if pairs is None:
        pairs = [(c, c + 1) for c in range(nch - 1)]
    D = rng.standard_normal((len(pairs), count, count)) / np.sqrt(count)
    a0 = rng.standard_normal((nscan, nch, count)) + 1j * rng.standard_normal((nscan, nch, count))
    a0 /= np.sqrt(np.sum(np.abs(a0) ** 2, axis=(1, 2)))[:, None, None]
    T = nsteps * dt
    c = np.array([float(x) for x in C])
    t = (np.arange(nsteps)[:, None] + c[None, :]) * dt
    amp = 0.3 + 0.1 * np.arange(nscan)
    field = (amp[None, None, :] * (np.sin(np.pi * t / T) ** 2 * np.cos(1.1 * t))[:, :, None]) * np.exp(1j * phase)
    return E, pairs, D, a0, np.ascontiguousarray(field.astype(np.complex128))


def two_by_two(nsteps, T=8.0):
    """The 2 x 2 constant-field problem: two channels of one state, E = (-0.5, 0.3), coupling 0.4, f = 1 + 0.5i; the closed form
    from eigh of the Hermitian 2 x 2 matrix.  The accumulated error (5th-order weights, grows with T) and the largest per-step estimate
    (the 4th-order formula's local error) both scale as dt^5, so their ratio is a property of T alone; T = 8 is a run of a few
    Rabi periods.  Returns (E, pairs, D, a0, field, dt, exact a(T))."""
    E = np.array([[-0.5], [0.3]])
    D = np.array([[[0.4]]])
    f = 1.0 + 0.5j
    H = np.array([[E[0, 0], np.conj(f) * 0.4], [f * 0.4, E[1, 0]]])           # row of channel cf = 1: f D^T a_0
    w, V = np.linalg.eigh(H)
    a0 = np.array([[[0.6], [0.8j]]])
    exact = (V @ (np.exp(-1j * w * T) * (V.conj().T @ a0.reshape(2)))).reshape(1, 2, 1)
    field = np.full((nsteps, 6, 1), f, dtype=np.complex128)
    return E, [(0, 1)], D, a0, field, T / nsteps, exact
