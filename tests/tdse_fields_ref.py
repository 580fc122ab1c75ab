"""NumPy restatement of bspatom_tdse_fields (include/bspatom.h): tdse_static_ref.propagate with a field per driven pair, and the rows of
4 + 2 nfield entries, in a real / complex dtype of the caller's choice.

    fidx[p] in 0 .. nfield-1: the field of pair p;  field (nsteps, 6, nfield, nscan), [n, s, g, q] = f_{g,q} at stage s of step n
    i da_c/dt = E_c a_c + sum_{p: cf[p] = c} f_{fidx[p]} D_p^T a_ci[p] + sum_{p: ci[p] = c} conj(f_{fidx[p]}) D_p a_cf[p] + S_c(a)
    rows: k = 0, 1 population and sum E |a|^2; k = 2, 3 = Re, Im of z_{c,0}; k = 4, 5 of s_c; k = 4 + 2g, 5 + 2g of z_{c,g}, g >= 1,
          z_{c,g} = sum over the pairs p with cf[p] = c and fidx[p] = g of conj(a_cf) . D_p^T a_ci

The step loop is tdse_static_ref.propagate's, statement for statement, with f[fidx[p]] in the place of f: with one field the results are
its results bit for bit (tests/test_tdse_fields_cpu.py).  The rows come from the definitions (tdse_obs_ref, tdse_static_ref).  The tests
use it as the project uses the other restatements: run in complex128 and in long double, the library within 8 times the complex128 run's
own distance from the long-double run.  Nothing here calls the library."""
import numpy as np

import tdse_obs_ref
import tdse_ref
import tdse_static_ref
from tdse_ref import A, B, C, D5, _num
from tdse_static_ref import _static


def propagate(E, pairs, D, fidx, a0, field, dt, static=None, scheme=1, rdtype=np.float64, cdtype=np.complex128, snap_every=0, obs_every=0):
    """The arguments of tdse_static_ref.propagate with fidx (one entry per pair) and field (nsteps, 6, nfield, nscan):
    (a, err[, obs][, snaps]), obs (nobs, nscan, nch, 4 + 2 nfield)."""
    assert scheme in (0, 1)
    E64 = np.asarray(E).astype(np.float64)
    Er = np.asarray(E).astype(rdtype)
    count = E64.shape[1]
    D = np.asarray(D).astype(rdtype).reshape(len(pairs), count, count)
    st = _static(static, count, rdtype)
    a = np.asarray(a0).astype(cdtype)
    fld = np.asarray(field).astype(cdtype)
    assert fld.ndim == 4 and fld.shape[1] == 6 and fld.shape[3] == a.shape[0], fld.shape
    nfield = fld.shape[2]
    fidx = [int(g) for g in fidx]
    assert len(fidx) == len(pairs) and all(0 <= g < nfield for g in fidx)
    dt64 = np.float64(dt)
    dt = rdtype(dt)
    mi, im = cdtype(-1j), cdtype(1j)
    nscan = a.shape[0]
    tabA = [[_num(x, rdtype) for x in row] for row in A]
    tabD = [_num(x, rdtype) for x in D5]
    tabE = [_num(x - y, rdtype) for x, y in zip(D5, B)]
    R = [None]
    if scheme == 1:
        for s in range(1, 6):
            theta = (E64 * (np.float64(C[s].numerator) / np.float64(C[s].denominator) * dt64)).astype(rdtype)
            R.append((np.cos(theta) - im * np.sin(theta)).astype(cdtype)[None])
    err = np.zeros(nscan, dtype=rdtype)
    snaps, rows = [], []
    nsteps = fld.shape[0]

    def add_static(h, y):
        for j, (i, f) in enumerate(st[0]):
            t = y[:, i] @ st[2][j]
            h[:, f] += mi * t if st[1][j] else t

    def rhs(y, f):                                                        # f (nfield, nscan)
        h = Er[None] * y
        for p, (i, j) in enumerate(pairs):
            h[:, j] += f[fidx[p]][:, None] * (y[:, i] @ D[p])
            h[:, i] += np.conj(f[fidx[p]])[:, None] * (y[:, j] @ D[p].T)
        add_static(h, y)
        return mi * h

    def coupling(y, f):
        g = np.zeros_like(y)
        for p, (i, j) in enumerate(pairs):
            g[:, j] += f[fidx[p]][:, None] * (y[:, i] @ D[p])
            g[:, i] += np.conj(f[fidx[p]])[:, None] * (y[:, j] @ D[p].T)
        add_static(g, y)
        return g

    for n in range(nsteps):
        if obs_every and n % obs_every == 0:
            rows.append(observables(E, pairs, D, fidx, nfield, st, a, rdtype, cdtype))
        k = []
        for s in range(6):
            y = a.copy()
            if scheme == 0:
                if s:
                    y = a + dt * sum(tabA[s][j] * k[j] for j in range(s))
                k.append(rhs(y, fld[n, s]))
            else:
                if s:
                    y = R[s] * (a + dt * sum(tabA[s][j] * k[j] for j in range(s)))
                ks = mi * coupling(y, fld[n, s])
                k.append(np.conj(R[s]) * ks if s else ks)
        if scheme == 0:
            a = a + dt * sum(tabD[s] * k[s] for s in range(6))
        else:
            a = R[4] * (a + dt * sum(tabD[s] * k[s] for s in range(6)))
        e = dt * np.abs(sum(tabE[s] * k[s] for s in range(6)))
        err = np.maximum(err, e.reshape(nscan, -1).max(axis=1))
        if snap_every and (n + 1) % snap_every == 0:
            snaps.append(a.copy())
    out = (a, err)
    if obs_every:
        rows.append(observables(E, pairs, D, fidx, nfield, st, a, rdtype, cdtype))
        out += (np.array(rows),)
    if snap_every:
        out += (np.array(snaps),)
    return out


def both(E, pairs, D, fidx, a0, field, dt, **kw):
    """(complex128 result, long-double result) of propagate"""
    assert np.finfo(np.longdouble).eps < 2e-19
    return (propagate(E, pairs, D, fidx, a0, field, dt, rdtype=np.float64, cdtype=np.complex128, **kw),
            propagate(E, pairs, D, fidx, a0, field, dt, rdtype=np.longdouble, cdtype=np.clongdouble, **kw))


def sublist(pairs, D, fidx, g):
    """the pairs of field g, in their order, and their blocks"""
    sel = [p for p, x in enumerate(fidx) if int(x) == g]
    D = np.asarray(D)
    return [pairs[p] for p in sel], (D[sel] if sel else np.zeros((0,) + D.shape[1:], dtype=D.dtype))


def observables(E, pairs, D, fidx, nfield, static, a, rdtype=np.float64, cdtype=np.complex128):
    """a (..., nch, count): (..., nch, 4 + 2 nfield) from the definitions: tdse_static_ref.observables on the pairs of field 0, then
    Re, Im of z_{c,g} (tdse_obs_ref.observables on the pairs of field g) for g = 1 .. nfield-1"""
    count = np.asarray(E).shape[1]
    D = np.asarray(D).reshape(len(pairs), count, count)
    p0, D0 = sublist(pairs, D, fidx, 0)
    out = [tdse_static_ref.observables(E, p0, D0, static, a, rdtype, cdtype)]
    for g in range(1, nfield):
        pg, Dg = sublist(pairs, D, fidx, g)
        out.append(tdse_obs_ref.observables(E, pg, Dg, a, rdtype, cdtype)[..., 2:])
    return np.concatenate(out, axis=-1)


CARRIER = (1.1, 0.7, 1.6)
PHASE = (0.0, 0.9, -0.5)


def system(nch, count, nscan, nsteps, nfield, dt=0.05, phase=0.0):
    """The test problem of the GPU tests: (E, pairs, D, fidx, a0, field, static).  tdse_ref.system's E, chain of pairs, D and a0 and
    tdse_static_ref.static_system's static blocks; every second pair on field 1 and, with three fields, every third on field 2; one
    more pair that doubles pair 0 (the same two channels, half its block) on the last field; field g = tdse_ref.system's envelope and
    per-scan amplitudes on a carrier and a phase of its own (times exp(i phase))."""
    assert nfield in (1, 2, 3)
    E, pairs, D, a0, _ = tdse_ref.system(nch, count, nscan, nsteps, dt=dt)
    fidx = []
    for p in range(len(pairs)):
        g = 0
        if nfield >= 2 and p % 2 == 1:
            g = 1
        if nfield >= 3 and p % 3 == 2:
            g = 2
        fidx.append(g)
    pairs = list(pairs) + [pairs[0]]
    D = np.ascontiguousarray(np.concatenate([D, 0.5 * D[:1]]))
    fidx.append(nfield - 1)
    T = nsteps * dt
    c = np.array([float(x) for x in C])
    t = (np.arange(nsteps)[:, None] + c[None, :]) * dt
    amp = 0.3 + 0.1 * np.arange(nscan)
    field = np.zeros((nsteps, 6, nfield, nscan), dtype=np.complex128)
    for g in range(nfield):
        field[:, :, g, :] = (amp[None, None, :] * (np.sin(np.pi * t / T) ** 2 * np.cos(CARRIER[g] * t))[:, :, None]) * np.exp(1j * (PHASE[g] + phase))
    return E, pairs, D, fidx, a0, field, tdse_static_ref.static_system(nch, count)
