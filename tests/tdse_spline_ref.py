"""NumPy restatement of the Crank-Nicolson steps in the spline basis (csrc/tdse_spline.hip, bspatom_tdse_spline) for the tests: a
complex128 dense step c' = -(4i/dt) M^-1 (S c) - c with M = A - (2i/dt) S from resolvent_coupled_ref.dense_matrix and
numpy.linalg.solve IN THE DOCUMENTED ORDERING (unknown (i, c) at position i nch + c), the direct form (S + i tau A) c' = (S - i tau A) c
it is algebraically equal to, and the rows.  Matrices are channel-major; packets are (nch, n)."""
import numpy as np

import resolvent_coupled_ref as cref
import resolvent_ref as ref


def overlap(SB, nch):
    """the channel-major block-diagonal overlap (nch n, nch n), float64"""
    S = ref.upper_to_dense(SB)
    n = S.shape[0]
    O = np.zeros((nch * n, nch * n))
    for c in range(nch):
        O[c * n:(c + 1) * n, c * n:(c + 1) * n] = S
    return O


def hamiltonian(SB, HB, l, couplings=(), G=None, a=None, WB=None, w=None):
    """A = sum_c (H_lc - i W_c) + V, channel-major: the coupled matrix at z = 0"""
    return cref.dense_matrix(SB, HB, l, np.zeros(len(l)), couplings, G, a, WB, w)


def step(SB, HB, l, dt, c, couplings=(), G=None, a=None, WB=None, w=None):
    """one step in the library's form: b = S c, x = M^-1 b with M = A - (2i/dt) S, c' = -(4i/dt) x - c"""
    nch = len(l)
    c = np.asarray(c, dtype=np.complex128).reshape(nch, -1)
    M = cref.dense_matrix(SB, HB, l, np.full(nch, 2j / dt), couplings, G, a, WB, w)
    b = (overlap(SB, nch) @ c.ravel()).reshape(c.shape)
    x = cref.solve(M, b[None], nch)[0]
    return -(4j / dt) * x - c


def direct_step(A, S, c, dt):
    """the Crank-Nicolson step as written: (S + i tau A) c' = (S - i tau A) c, tau = dt / 2; A, S channel-major dense, c flat"""
    tau = 0.5 * dt
    return np.linalg.solve(S + 1j * tau * A, (S - 1j * tau * A) @ c)


def row(SB, c, P=None):
    """(nch + 2 nproj,): N_ch = Re c_ch^H S c_ch, then Re, Im of sum P_r (S c)"""
    c = np.asarray(c, dtype=np.complex128)
    S = ref.upper_to_dense(SB)
    b = c @ S.T
    out = [float(np.real(np.vdot(c[ch], b[ch]))) for ch in range(c.shape[0])]
    for p in ([] if P is None else P):
        v = np.sum(np.asarray(p) * b)
        out += [v.real, v.imag]
    return np.array(out)


def propagate(SB, HB, l, dt, c0, coef=None, couplings=(), G=None, WB=None, w=None, P=None):
    """nsteps steps of ONE packet: coef (nsteps, ncoup, nop) or, without couplings, an integer number of steps.  Returns (c, the packets
    after every step (nsteps, nch, n), the rows of the steps 0 .. nsteps (nsteps + 1, nch + 2 nproj))"""
    nsteps = int(coef) if np.isscalar(coef) else len(coef)
    c = np.asarray(c0, dtype=np.complex128)
    traj, rows = [], [row(SB, c, P)]
    for n in range(nsteps):
        c = step(SB, HB, l, dt, c, couplings, G, None if np.isscalar(coef) else coef[n], WB, w)
        traj.append(c)
        rows.append(row(SB, c, P))
    return c, np.array(traj).reshape((nsteps,) + c.shape), np.array(rows)


# ---- the pulse of the order tests (test_tdse_spline_cpu, test_gpu_tdse_spline): a short sin^2 pulse, about one cycle
PULSE = dict(F0=0.05, omega=0.5, T=12.0)


def pulse(t, F0=PULSE["F0"], omega=PULSE["omega"], T=PULSE["T"]):
    """F0 sin^2(pi t / T) sin(omega t) on 0 <= t <= T, zero outside"""
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 0.0) & (t <= T), F0 * np.sin(np.pi * t / T) ** 2 * np.sin(omega * t), 0.0)


def populations(SB, c, V):
    """|phi_s^T S c_ch|^2 for the eigenvectors V (nch, count, n) of the channels: (nch, count)"""
    S = ref.upper_to_dense(SB)
    c = np.asarray(c, dtype=np.complex128)
    return np.abs(np.einsum("csi,ci->cs", V, c @ S.T)) ** 2
