"""NumPy restatement of the split Crank-Nicolson steps in the spline basis (csrc/tdse_split.hip, bspatom_tdse_split) for the tests:
the three substeps of a step in complex128 with per-channel DENSE matrices built from the bands a caller sees,

    atomic half step, channel c:   x = M_c^-1 (S c_c),  M_c = H_lc - i W_c - (4i/dt) S,   c_c <- -(8i/dt) x - c_c
    field step, eigenchannel j:    d_j = sum_c Q(c,j) c_c,  N_j = S + i (dt/2) f lam_j G,   d_j <- 2 N_j^-1 (S d_j) - d_j
    back:                          c_c = sum_j Q(c,j) d_j, then the atomic half step again,

with the linear solves written twice: numpy.linalg.solve on the dense blocks ("dense") and scipy.linalg.solve_banded on the same
matrices in LAPACK's band storage ("banded").  The largest difference between the two in the S-norm is the fp64 noise of the scheme
on a case (delta_ref).  A third way ("lu") solves with tests/band_lu_ref.py, the plain banded LU in the device solvers' pivot rule,
and takes its two fault knobs: what a kernel with a cut pivot search or dropped fill would return (test_tdse_split_pivots_cpu.py).
Packets are (nch, n); matrices are (n, n) per channel."""
import numpy as np
import scipy.linalg

import band_lu_ref as blu
import resolvent_ref as ref
import tdse_spline_ref as sref


def to_banded(M, b):
    """LAPACK's band storage of a dense matrix of half-width b: ab[b + i - j, j] = M[i, j]"""
    n = M.shape[0]
    ab = np.zeros((2 * b + 1, n), dtype=M.dtype)
    for d in range(-b, b + 1):                                  # d = j - i
        i = np.arange(max(0, -d), min(n, n - d))
        ab[b - d, i + d] = M[i, i + d]
    return ab


class Solver:
    """x = M^-1 b for a dense banded matrix, by numpy.linalg.solve ("dense"), scipy.linalg.solve_banded ("banded") or band_lu_ref
    ("lu": factored here once, with the knobs max_pivot_distance and fill_width of band_lu_ref.factor where given)"""
    def __init__(self, M, b, how, **knobs):
        assert how in ("dense", "banded", "lu") and (how == "lu" or not knobs)
        self.M, self.b, self.how = M, b, how
        self.ab = to_banded(M, b) if how == "banded" else None
        if how == "lu":
            with np.errstate(all="ignore"):                    # a mutant may divide by a pivot that is zero
                self.LU, self.piv, _ = blu.factor(M, b, **knobs)

    def __call__(self, rhs):
        if self.how == "dense":
            return np.linalg.solve(self.M, rhs)
        if self.how == "lu":
            with np.errstate(all="ignore"):
                return blu.substitute(self.LU, self.piv, rhs, self.b)
        return scipy.linalg.solve_banded((self.b, self.b), self.ab, rhs)


def absorber_of(WB, w, nch):
    """the library's rule: w None with absorbers given means absorber 0 on every channel; -1 none"""
    if WB is None:
        return [-1] * nch
    return [0] * nch if w is None else [int(v) for v in np.broadcast_to(np.asarray(w), (nch,))]


def atomic_matrices(SB, HB, l, dt, WB=None, w=None):
    """M_c = H_lc - i W_c - (4i/dt) S per channel, dense complex128; HB[l] upper bands, WB (nabs, 2k-1, n) full bands or None"""
    ws = absorber_of(WB, w, len(l))
    WB = None if WB is None else np.asarray(WB).reshape(-1, 2 * SB.shape[0] - 1, SB.shape[1])
    return [ref.dense_matrix(SB, HB[lc], 4j / dt, None if ws[c] < 0 else WB[ws[c]]) for c, lc in enumerate(l)]


def s_norm(S, c):
    """sqrt(sum_c Re c_c^H S c_c)"""
    c = np.asarray(c, dtype=np.complex128).reshape(-1, S.shape[0])
    return float(np.sqrt(max(sum(np.real(np.vdot(v, S @ v)) for v in c), 0.0)))


def propagate(SB, HB, l, dt, c0, G, Q, lam, f, WB=None, w=None, P=None, how="dense", knobs=None):
    """len(f) steps of ONE packet c0 (nch, n); f: the complex field value per step; G a full band (2k-1, n); Q (nch, nch), lam (nch,).
    knobs: band_lu_ref's fault knobs for how = "lu", on every solve of the run.  Returns (c, the packets after every step (nsteps, nch, n), the rows of the steps 0 .. nsteps (nsteps + 1, nch + 2 nproj))."""
    nch, b = len(l), SB.shape[0] - 1
    S = ref.upper_to_dense(SB)
    Gd = ref.full_to_dense(np.asarray(G).reshape(2 * b + 1, -1)) if G is not None else None
    Q, lam = np.asarray(Q, dtype=np.float64).reshape(nch, nch), np.asarray(lam, dtype=np.float64).reshape(nch)
    knobs = knobs or {}
    atomic = [Solver(M, b, how, **knobs) for M in atomic_matrices(SB, HB, l, dt, WB, w)]
    c = np.array(c0, dtype=np.complex128).reshape(nch, -1)
    g = 8.0 / dt

    def half(c):
        return np.stack([-1j * g * atomic[ch](S @ c[ch]) - c[ch] for ch in range(nch)])

    traj, rows = [], [sref.row(SB, c, P)]
    for fn in np.asarray(f, dtype=np.complex128).reshape(-1):
        c = half(c)
        d = Q.T @ c                                             # d_j = sum_c Q(c, j) c_c
        d = np.stack([2.0 * Solver(S + 0.5j * dt * fn * lam[j] * Gd, b, how, **knobs)(S @ d[j]) - d[j] for j in range(nch)])
        c = half(Q @ d)                                         # c_c = sum_j Q(c, j) d_j
        traj.append(c)
        rows.append(sref.row(SB, c, P))
    return c, np.array(traj).reshape((len(traj), nch, -1)), np.array(rows)


def delta_ref(SB, HB, l, dt, c0, G, Q, lam, f, WB=None, w=None):
    """(the dense-solve result, its rows, delta): delta the largest S-norm difference, over the steps, between the packets of the
    dense-solve and the banded-solve restatement of one packet, divided by max(1, ||c0||_S)"""
    S = ref.upper_to_dense(SB)
    cd, td, rows = propagate(SB, HB, l, dt, c0, G, Q, lam, f, WB, w, how="dense")
    _, tb, _ = propagate(SB, HB, l, dt, c0, G, Q, lam, f, WB, w, how="banded")
    diff = max([s_norm(S, x - y) for x, y in zip(td, tb)] + [0.0])
    return cd, rows, diff / max(1.0, s_norm(S, c0))
