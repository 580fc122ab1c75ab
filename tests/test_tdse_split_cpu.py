"""The host side of the split-step spline-basis TDSE (Problem.tdse_split) pinned on the CPU: the header part and its exports, the helper
host.split_angular, and the scheme itself on the dense restatement tests/tdse_split_ref.py -- S-unitarity, the loss under an absorber,
the Cayley phase of an eigenvector, and the second order of the splitting against the unsplit step of tests/tdse_spline_ref.py.  Bands
from the oracle on test_gpu_resolvent_coupled.HYD4's grid (rb = 40, k = 9, nfun = 96), l = 0 .. 3.  No GPU."""
import os
import re
import numpy as np
import pytest
import scipy.linalg

import oracle as orc
import resolvent_ref as ref
import tdse_spline_ref as sref
import tdse_split_ref as pref
from bspatom_amd import capi, host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=3, l_ini=0, n0_ini=1, zatom=1.0)       # HYD4
EPS = np.finfo(np.float64).eps
CHANS = [(0, 0), (1, 0), (2, 0), (3, 0)]
L = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def hyd():
    c = orc.make_cfg(**KW)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 4)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    S = ref.upper_to_dense(SB)
    ev = [scipy.linalg.eigh(ref.upper_to_dense(HB[l]), S) for l in range(4)]
    E, V = np.stack([e[0] for e in ev]), np.stack([e[1].T for e in ev])
    Q, lam = host.split_angular(CHANS)
    c1s = np.zeros((4, c.nfun), dtype=np.complex128)
    c1s[0] = V[0, 0]
    return dict(SB=SB, HB=HB, R=RB[0], S=S, E=E, V=V, Q=Q, lam=lam, c1s=c1s, n=c.nfun, k=c.k)


def test_header_part_is_included_and_its_symbols_are_exported():
    """include/bspatom_tdse_split.h is part of include/bspatom.h (included there, refuses to stand alone); what it declares is
    capi.SPLIT_EXPORTS, and the library exports it with the argument list the header gives (21 arguments)"""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    main = open(os.path.join(inc, "bspatom.h")).read()
    assert '#include "bspatom_tdse_split.h"' in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    part = open(os.path.join(inc, "bspatom_tdse_split.h")).read()
    assert "#ifndef BSPATOM_H\n#error" in part
    code = re.sub(r"/\*.*?\*/", "", part, flags=re.S)
    decl = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(bspatom_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", code))
    assert sorted(decl) == sorted(capi.SPLIT_EXPORTS)
    lib = capi.lib()
    for name, params in decl.items():
        assert hasattr(lib, name) and name not in capi.EXPORTS and name not in capi.SPLINE_EXPORTS
        assert len(params.split(",")) == len(getattr(lib, name).argtypes) == 21, name


def test_split_angular_reproduces_stark_system():
    """A from stark_system(channels, 1.0) -- both directions of every block, the same real factor --: Q orthogonal, lam ascending,
    Q diag(lam) Q^T = A to a few eps; for m = 0 and l = 0 .. 3 the matrix is the Jacobi matrix of the Legendre polynomials, so lam are
    the four Gauss-Legendre nodes.  With m = 1 the factors change and l = 0 drops out."""
    for chans in (CHANS, [(1, 1), (2, 1), (3, 1)], [(0, 0), (2, 0)], [(3, 0), (0, 0), (1, 0)]):
        nch = len(chans)
        A = np.zeros((nch, nch))
        couplings, a = host.stark_system(chans, 1.0)
        for (cr, cc, _t), v in zip(couplings, a):
            assert v.imag == 0.0
            A[cr, cc] = v.real
        assert np.array_equal(A, A.T)
        Q, lam = host.split_angular(chans)
        assert Q.shape == (nch, nch) and lam.shape == (nch,) and Q.flags.c_contiguous and np.all(np.diff(lam) >= 0.0)
        assert np.max(np.abs(Q @ np.diag(lam) @ Q.T - A)) <= 8 * EPS
        assert np.max(np.abs(Q.T @ Q - np.eye(nch))) <= 8 * EPS
    Q, lam = host.split_angular(CHANS)
    assert np.allclose(lam, np.polynomial.legendre.leggauss(4)[0], rtol=0, atol=8 * EPS)
    assert abs(host.stark_system(CHANS, 1.0)[1][0].real - 1.0 / np.sqrt(3.0)) <= 2 * EPS
    Q2, lam2 = host.split_angular([(0, 0), (2, 0)])            # no dipole block between them
    assert np.array_equal(lam2, np.zeros(2))


def test_unitary_without_absorber_and_absorbing_with(hyd):
    """No absorber, real f: every factor of a step is S-unitary; c^H S c keeps its value over 40 steps within nsteps n eps cond, cond
    the largest condition number of the matrices solved with.  With an absorber W = 0.05 S on every channel the norm falls at every
    step, near exp(-0.1 t)."""
    n, dt, nsteps = hyd["n"], 0.1, 40
    F = 0.1 * np.sin(0.5 * host.spline_midpoints(0.0, dt, nsteps))
    args = (hyd["SB"], hyd["HB"], L, dt, hyd["c1s"], hyd["R"], hyd["Q"], hyd["lam"], F)
    _, _, rows = pref.propagate(*args)
    norm = rows.sum(-1)
    Gd = ref.full_to_dense(hyd["R"])
    cond = max([np.linalg.cond(M) for M in pref.atomic_matrices(hyd["SB"], hyd["HB"], L, dt)] +
               [np.linalg.cond(hyd["S"] + 0.5j * dt * 0.1 * lj * Gd) for lj in hyd["lam"]])
    print("norm drift %.3e over %d steps, population moved %.3e" % (np.max(np.abs(norm - norm[0])), nsteps, rows[0, 0] - rows[-1, 0]))
    assert abs(norm[0] - 1.0) <= 64 * EPS and rows[0, 0] - rows[-1, 0] > 1e-4
    assert np.max(np.abs(norm - norm[0])) <= nsteps * 2 * n * EPS * cond
    Wb = host.band_symmetric(hyd["SB"])[None] * 0.05
    _, _, rows_w = pref.propagate(*args, WB=Wb, w=None)
    norm_w = rows_w.sum(-1)
    assert np.all(np.diff(norm_w) < 0.0)
    assert abs(norm_w[-1] / np.exp(-0.1 * nsteps * dt) - 1.0) <= 5e-4
    assert np.allclose(host.spline_yield(rows_w[:, None]), 1.0 - norm_w[:, None], rtol=0, atol=0)


def test_eigenvector_comes_back_with_its_cayley_phase(hyd):
    """f = 0: the field step is the identity (N_j = S, d <- 2 d - d) and Q Q^T = 1, so an eigenvector (E, phi) of channel c returns
    after n steps as ((1 - i E dt/4) / (1 + i E dt/4))^(2 n) phi: two atomic half steps of tau = dt/4 per step.  States 1, 4, 20 and the
    highest of l = 0 and l = 3; deviation within nsteps n eps cond(M_c) |phi|_max."""
    n, dt, nsteps = hyd["n"], 0.05, 7
    Ms = pref.atomic_matrices(hyd["SB"], hyd["HB"], L, dt)
    for ch in (0, 3):
        cond = np.linalg.cond(Ms[ch])
        for s in (0, 3, 19, n - 1):
            E = hyd["E"][ch, s]
            c0 = np.zeros((4, n), dtype=np.complex128)
            c0[ch] = hyd["V"][ch, s]
            for how in ("dense", "banded"):
                c, _, _ = pref.propagate(hyd["SB"], hyd["HB"], L, dt, c0, hyd["R"], hyd["Q"], hyd["lam"], np.zeros(nsteps), how=how)
                closed = ((1 - 0.25j * dt * E) / (1 + 0.25j * dt * E)) ** (2 * nsteps) * c0
                dev = np.max(np.abs(c - closed))
                print("channel %d state %d (E %.4g) %s: deviation %.3e" % (ch, s + 1, E, how, dev))
                assert dev <= 2 * nsteps * n * EPS * cond * np.max(np.abs(c0)), (ch, s, how, dev)
                assert np.max(np.abs(c - c0)) > 1e-3


def test_second_order_against_the_unsplit_step(hyd):
    """Hydrogen 1s, channels l = 0 .. 3 at m = 0, through F0 sin^2(pi t / T) sin(omega t) with F0 = 0.1, omega = 0.5, T = 6 (half a
    cycle under the envelope): the largest coefficient difference between the split restatement and the UNSPLIT Crank-Nicolson step of
    tests/tdse_spline_ref.py at the same dt is the splitting error, C dt^2 (1 + O(dt^2)) -- both are second-order approximations of the
    same equation --, so it falls by 4 when dt is halved.  dt = 0.2 against 0.1, window 3.8 .. 4.2.  Measured: 1.424e-03 and 3.562e-04,
    ratio 3.9990 (3.9986 at dt = 0.1 against 0.05, 3.9996 at 0.05 against 0.025; 3.9944 for F0 = 0.05, T = 12 at dt = 0.2)."""
    F0, omega, T = 0.1, 0.5, 6.0
    pat = host.stark_system(CHANS, 1.0)
    errs = []
    for dt in (0.2, 0.1):
        ns = int(round(T / dt))
        F = sref.pulse(host.spline_midpoints(0.0, dt, ns), F0, omega, T)
        coef = host.spline_coefficients(pat, F)[:, 0]
        cu, _, _ = sref.propagate(hyd["SB"], hyd["HB"], L, dt, hyd["c1s"], coef, pat[0], hyd["R"][None])
        cs, _, rows = pref.propagate(hyd["SB"], hyd["HB"], L, dt, hyd["c1s"], hyd["R"], hyd["Q"], hyd["lam"], F)
        assert rows[0, 0] - rows[-1, 0] > 1e-4                  # the pulse did move population out of l = 0
        errs.append(float(np.max(np.abs(cu - cs))))
    ratio = errs[0] / errs[1]
    print("split against unsplit: %.3e (dt 0.2), %.3e (dt 0.1), ratio %.4f" % (errs[0], errs[1], ratio))
    assert errs[1] > 1e-6
    assert 3.8 <= ratio <= 4.2, (errs, ratio)


def test_dense_and_banded_solves_agree(hyd):
    """the two ways the restatement solves its systems differ by fp64 noise alone: delta_ref of a random packet over 7 steps is below
    nsteps n eps cond and above zero"""
    rng = np.random.default_rng(3)
    n, dt, nsteps = hyd["n"], 0.05, 7
    c0 = (rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))) / np.sqrt(n)
    f = rng.uniform(0.2, 1.0, nsteps)
    _, _, delta = pref.delta_ref(hyd["SB"], hyd["HB"], L, dt, c0, hyd["R"], hyd["Q"], hyd["lam"], f)
    cond = max(np.linalg.cond(M) for M in pref.atomic_matrices(hyd["SB"], hyd["HB"], L, dt))
    print("delta_ref %.3e" % delta)
    assert 0.0 < delta <= nsteps * n * EPS * cond
