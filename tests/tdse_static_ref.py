"""NumPy restatement of bspatom_tdse_static (include/bspatom.h): both schemes of the tableau with static blocks beside the driven
couplings, and the six entries of a row, in a real / complex dtype of the caller's choice.

    static = (spairs, skind, W): block j adds to the right-hand side of i da/dt of channel sf[j] alone
        skind[j] = 0:  + W_j^T a_si[j]          skind[j] = 1:  - i W_j^T a_si[j],          (W^T a)[f] = sum_i W[i][f] a[i]
    scheme 0: tdse_ref.propagate's steps with h += S(y);  scheme 1: tdse_lawson_ref.propagate's with g += S(y)
    rows: k = 0 .. 3 tdse_obs_ref.observables, k = 4, 5 = Re, Im of s_c = sum_f conj(a_c[f]) S_c[f] on a(t_n)

The step loops are those of tdse_ref.propagate and tdse_lawson_ref.propagate, statement for statement, with the static terms added
behind the pairs' loop: without static blocks the results are theirs bit for bit (tests/test_tdse_static_cpu.py).  The tests use it as
the project uses those two: run in complex128 and in long double, the library within 8 times the complex128 run's own distance from
the long-double run.  Nothing here calls the library."""
import numpy as np

import tdse_lawson_ref
import tdse_obs_ref
import tdse_ref
from tdse_ref import A, B, C, D5, _num

NONE = ((), (), np.zeros((0, 1, 1)))


def _static(static, count, rdtype):
    spairs, skind, W = NONE if static is None else static
    spairs = [(int(i), int(f)) for i, f in spairs]
    skind = [int(k) for k in skind]
    assert len(spairs) == len(skind) and all(k in (0, 1) for k in skind)
    W = np.asarray(W).astype(rdtype).reshape(len(spairs), count, count) if spairs else np.zeros((0, count, count), dtype=rdtype)
    return spairs, skind, W


def static_rhs(static, y, cdtype=np.complex128):
    """S(y) (y: (..., nch, count)) of the static blocks, channel by channel in ascending j"""
    spairs, skind, W = static
    mi = cdtype(-1j)
    S = np.zeros_like(y)
    for j, (i, f) in enumerate(spairs):
        t = y[..., i, :] @ W[j]                                           # (W_j^T a)[f] = sum_i W_j[i][f] a[i]
        S[..., f, :] += mi * t if skind[j] else t
    return S


def propagate(E, pairs, D, a0, field, dt, static=None, scheme=1, rdtype=np.float64, cdtype=np.complex128, snap_every=0, obs_every=0):
    """The arguments of tdse_ref.propagate, static = (spairs, skind, W) or None, scheme 0 (plain) or 1 (Lawson), obs_every as in
    bspatom_tdse_observe: (a, err[, obs][, snaps]), obs (nobs, nscan, nch, 6)."""
    assert scheme in (0, 1)
    E64 = np.asarray(E).astype(np.float64)
    Er = np.asarray(E).astype(rdtype)
    count = E64.shape[1]
    D = np.asarray(D).astype(rdtype).reshape(len(pairs), count, count)
    st = _static(static, count, rdtype)
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

    def rhs(y, f):                                                        # tdse_ref.propagate's, then the static terms
        h = Er[None] * y
        for p, (i, j) in enumerate(pairs):
            h[:, j] += f[:, None] * (y[:, i] @ D[p])
            h[:, i] += np.conj(f)[:, None] * (y[:, j] @ D[p].T)
        add_static(h, y)
        return mi * h

    def coupling(y, f):                                                   # tdse_lawson_ref.propagate's, then the static terms
        g = np.zeros_like(y)
        for p, (i, j) in enumerate(pairs):
            g[:, j] += f[:, None] * (y[:, i] @ D[p])
            g[:, i] += np.conj(f)[:, None] * (y[:, j] @ D[p].T)
        add_static(g, y)
        return g

    for n in range(nsteps):
        if obs_every and n % obs_every == 0:
            rows.append(observables(E, pairs, D, st, a, rdtype, cdtype))
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
        rows.append(observables(E, pairs, D, st, a, rdtype, cdtype))
        out += (np.array(rows),)
    if snap_every:
        out += (np.array(snaps),)
    return out


def both(E, pairs, D, a0, field, dt, **kw):
    """(complex128 result, long-double result) of propagate"""
    assert np.finfo(np.longdouble).eps < 2e-19
    return (propagate(E, pairs, D, a0, field, dt, rdtype=np.float64, cdtype=np.complex128, **kw),
            propagate(E, pairs, D, a0, field, dt, rdtype=np.longdouble, cdtype=np.clongdouble, **kw))


def observables(E, pairs, D, static, a, rdtype=np.float64, cdtype=np.complex128):
    """a (..., nch, count): (..., nch, 6) = tdse_obs_ref.observables and Re, Im of s_c = sum_f conj(a_c[f]) S_c[f]"""
    count = np.asarray(E).shape[1]
    st = _static(static, count, rdtype)
    o4 = tdse_obs_ref.observables(E, pairs, D, a, rdtype, cdtype)
    a = np.asarray(a).astype(cdtype)
    s = np.sum(np.conj(a) * static_rhs(st, a, cdtype), axis=-1)
    return np.concatenate([o4, s.real[..., None], s.imag[..., None]], axis=-1)


def static_magnitudes(static, a):
    """M_4, M_5 in long double, as tdse_obs_ref.magnitudes gives M_0 .. M_3: the largest over the rows (leading index of a, channel) of
    the sum of the moduli of the real terms of Re s_c and of Im s_c.  With u = |W|^T |a_si|: a kind-0 block gives Re s the terms a_re[f]
    W a_re[i], a_im[f] W a_im[i] and Im s the terms a_re[f] W a_im[i], a_im[f] W a_re[i]; a kind-1 block the other way round."""
    a = np.asarray(a).astype(np.clongdouble)
    nch, count = a.shape[-2:]
    a = a.reshape(-1, nch, count)
    spairs, skind, W = _static(static, count, np.longdouble)
    m = np.zeros((a.shape[0], nch, 2), dtype=np.longdouble)
    ar, ai, aW = np.abs(a.real), np.abs(a.imag), np.abs(W)
    for j, (i, f) in enumerate(spairs):
        ur, ui = ar[:, i] @ aW[j], ai[:, i] @ aW[j]
        same = np.sum(ar[:, f] * ur + ai[:, f] * ui, axis=-1)
        cross = np.sum(ar[:, f] * ui + ai[:, f] * ur, axis=-1)
        m[:, f, 0] += cross if skind[j] else same
        m[:, f, 1] += same if skind[j] else cross
    return m.reshape(-1, 2).max(axis=0)


def absorbers(nch, count, channels, seed=0, norm=0.5):
    """Symmetric positive definite blocks of spectral norm `norm`, one per entry of `channels`: (count, count) each"""
    rng = np.random.default_rng(77 + 1000 * nch + 10 * count + seed)
    out = []
    for _ in channels:
        G = rng.standard_normal((count, count))
        P = G @ G.T + 0.1 * np.eye(count)
        out.append(P * (norm / np.linalg.norm(P, 2)))
    return out


def static_system(nch, count, seed=0):
    """The static lists of the GPU tests on tdse_ref.system(nch, count, ..).  Kind-1 blocks P: symmetric positive, norm 0.5; the kind-0
    in-channel block H symmetric, the cross-channel block X general, norm 0.3 each; X enters as the Hermitian pair X, X^T.
        nch = 2: channel 0 no static block; channel 1 a kind-0 and a kind-1 block
        nch = 3: channel 0 one kind-1 block; channel 1 X^T from channel 2; channel 2 X from channel 1, then H and a kind-1 block
        nch = 4: channel 0 none; channel 1 one kind-1 block; channel 2 H, a kind-1 block and X^T from channel 3; channel 3 X from 2"""
    assert nch in (2, 3, 4)
    rng = np.random.default_rng(4242 + 1000 * nch + 10 * count + seed)
    P = absorbers(nch, count, range(2), seed)
    H = rng.standard_normal((count, count))
    H = H + H.T
    H *= 0.3 / float(np.linalg.norm(H, 2))
    X = rng.standard_normal((count, count))
    X *= 0.3 / float(np.linalg.norm(X, 2))
    if nch == 2:
        spairs, skind, W = [(1, 1), (1, 1)], [0, 1], [H, P[0]]
    elif nch == 3:
        spairs, skind, W = [(0, 0), (2, 1), (1, 2), (2, 2), (2, 2)], [1, 0, 0, 0, 1], [P[0], X.T, X, H, P[1]]
    else:
        spairs, skind, W = [(1, 1), (2, 2), (2, 2), (3, 2), (2, 3)], [1, 0, 1, 0, 0], [P[0], H, P[1], X.T, X]
    return spairs, skind, np.ascontiguousarray(np.stack(W))
