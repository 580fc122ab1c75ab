"""The host side of the spline-basis TDSE (Problem.tdse_spline) pinned on the CPU: the helpers host.band_symmetric / spline_midpoints /
spline_coefficients / spline_packet / spline_yield, and the scheme itself on the dense restatement tests/tdse_spline_ref.py -- the
library's form c' = -(4i/dt) M^-1 S c - c against the Crank-Nicolson step as written, unitarity, second order against
scipy.linalg.expm on a constant field and against a tight Runge-Kutta solution through a pulse (the measurement behind the window of
test_gpu_tdse_spline's order test).  Bands from the oracle on the n65_k4 grid (rb = 40, k = 4, nfun = 65), l = 0, 1.  No GPU."""
import types
import numpy as np
import pytest
import scipy.linalg

import oracle as orc
import resolvent_ref as ref
import tdse_spline_ref as sref
from bspatom_amd import host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=4, nfun=65, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)
EPS = np.finfo(np.float64).eps
CHANS = [(0, 0), (1, 0)]


@pytest.fixture(scope="module")
def hyd():
    c = orc.make_cfg(**KW)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 2)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    S = ref.upper_to_dense(SB)
    ev = [scipy.linalg.eigh(ref.upper_to_dense(HB[l]), S) for l in range(2)]
    E, V = np.stack([e[0] for e in ev]), np.stack([e[1].T for e in ev])
    pat = host.stark_system(CHANS, 1.0)
    A0 = sref.hamiltonian(SB, HB, [0, 1])
    A1 = sref.hamiltonian(SB, HB, [0, 1], pat[0], RB[:1], pat[1]) - A0
    c1s = np.zeros((2, c.nfun), dtype=np.complex128)
    c1s[0] = V[0, 0]
    return dict(SB=SB, HB=HB, RB=RB, S=S, Sd=sref.overlap(SB, 2), E=E, V=V, pat=pat, A0=A0, A1=A1, c1s=c1s, n=c.nfun, k=c.k)


def test_header_part_is_included_and_its_symbols_are_exported():
    """include/bspatom_tdse_spline.h is part of include/bspatom.h (included there, refuses to stand alone); what it declares is
    capi.SPLINE_EXPORTS, and the library exports it with the argument list the header gives (24 arguments)"""
    import os
    import re
    from bspatom_amd import capi
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    main = open(os.path.join(inc, "bspatom.h")).read()
    assert '#include "bspatom_tdse_spline.h"' in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    part = open(os.path.join(inc, "bspatom_tdse_spline.h")).read()
    assert "#ifndef BSPATOM_H\n#error" in part
    code = re.sub(r"/\*.*?\*/", "", part, flags=re.S)
    decl = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(bspatom_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", code))
    assert sorted(decl) == sorted(capi.SPLINE_EXPORTS)
    L = capi.lib()
    for name, params in decl.items():
        assert hasattr(L, name) and name not in capi.EXPORTS
        assert len(params.split(",")) == len(getattr(L, name).argtypes) == 24, name


def test_band_symmetric_and_the_right_hand_side(hyd):
    SBf = host.band_symmetric(hyd["SB"])
    assert SBf.shape == (2 * hyd["k"] - 1, hyd["n"])
    assert np.array_equal(ref.full_to_dense(SBf), hyd["S"])
    x = np.random.default_rng(1).standard_normal((3, hyd["n"]))
    assert np.allclose(host.band_apply(SBf, x), x @ hyd["S"].T, rtol=0, atol=8 * EPS * np.max(np.abs(x)))


def test_midpoints_packet_and_yield():
    t = host.spline_midpoints(1.0, 0.25, 4)
    assert np.array_equal(t, np.array([1.125, 1.375, 1.625, 1.875]))
    assert host.spline_midpoints(0.0, 0.1, 0).shape == (0,)
    prob = types.SimpleNamespace(nfun=5)
    c = host.spline_packet(prob, [(0, 0), (1, 0), (2, 0)], 1, np.arange(5.0))
    assert c.shape == (3, 5) and c.dtype == np.complex128
    assert np.array_equal(c[1], np.arange(5.0)) and not np.any(c[0]) and not np.any(c[2])
    obs = np.array([[[0.75, 0.25, 9.0, 9.0]], [[0.5, 0.25, 9.0, 9.0]]])              # (nobs, nscan, nch + 2): one projection behind
    assert np.array_equal(host.spline_yield(obs, nch=2), np.array([[0.0], [0.25]]))
    assert np.array_equal(host.spline_yield(obs[..., :2]), np.array([[0.0], [0.25]]))


def test_spline_coefficients():
    """entry p gets a[p] F, a transposed partner a[p] conj(F); one-dimensional F is one scan; the table is Hermitian step by step"""
    couplings = [(0, 1, 0), (1, 0, 1), (0, 0, 0)]
    a = np.array([[0.5 + 0.1j, 2.0], [0.5 - 0.1j, 2.0], [1.0, 0.0]])
    F = np.array([[1.0 + 1.0j, 2.0], [0.5j, -1.0]])                                 # (nsteps, nscan)
    tab = host.spline_coefficients((couplings, a), F)
    assert tab.shape == (2, 2, 3, 2) and tab.dtype == np.complex128 and tab.flags.c_contiguous
    for n in range(2):
        for q in range(2):
            assert np.array_equal(tab[n, q, 0], a[0] * F[n, q]) and np.array_equal(tab[n, q, 2], a[2] * F[n, q])
            assert np.array_equal(tab[n, q, 1], a[1] * np.conj(F[n, q]))
    assert np.array_equal(tab[:, :, 1, 0], np.conj(tab[:, :, 0, 0]))               # the partner of a conjugate pattern stays the conjugate
    one = host.spline_coefficients(host.stark_system(CHANS, 1.0), np.array([0.1, 0.2, 0.3]))
    assert one.shape == (3, 1, 2, 1) and np.array_equal(one[:, 0, 0, 0], one[:, 0, 1, 0])


def test_library_form_equals_crank_nicolson(hyd):
    """c' = -(4i/dt) M^-1 (S c) - c, M = A - (2i/dt) S, against (S + i tau A) c' = (S - i tau A) c solved directly: the same vector
    up to the two solves' rounding, N eps (cond(M) + cond(S + i tau A)) |c|, with a Hermitian field, and with an absorber on top."""
    rng = np.random.default_rng(2)
    n, dt = hyd["n"], 0.05
    c = (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) / np.sqrt(n)
    Wb = 1e-2 * np.abs(hyd["RB"][0])
    a = 0.3 * hyd["pat"][1]
    for WB, w in ((None, None), (Wb[None], [0, -1])):
        new = sref.step(hyd["SB"], hyd["HB"], [0, 1], dt, c, hyd["pat"][0], hyd["RB"][:1], a, WB, w)
        A = sref.hamiltonian(hyd["SB"], hyd["HB"], [0, 1], hyd["pat"][0], hyd["RB"][:1], a, WB, w)
        direct = sref.direct_step(A, hyd["Sd"], c.ravel(), dt).reshape(2, n)
        conds = np.linalg.cond(A - (2j / dt) * hyd["Sd"]) + np.linalg.cond(hyd["Sd"] + 0.5j * dt * A)
        bound = 2 * n * EPS * conds * np.max(np.abs(c))
        diff = np.max(np.abs(new - direct))
        print("absorber %s: difference %.3e  bound %.3e" % (WB is not None, diff, bound))
        assert diff <= bound and np.max(np.abs(new - c)) > 1e-3


def test_unitary_without_absorber_and_absorbing_with(hyd):
    """Hermitian problem: c^H S c keeps its value over 40 steps within nsteps N eps cond(M); with an absorber W >= 0 on both channels
    it falls at every step"""
    n, dt, nsteps = hyd["n"], 0.1, 40
    F = 0.1 * np.sin(0.5 * host.spline_midpoints(0.0, dt, nsteps))
    coef = host.spline_coefficients(hyd["pat"], F)[:, 0]
    args = (hyd["SB"], hyd["HB"], [0, 1], dt, hyd["c1s"], coef, hyd["pat"][0], hyd["RB"][:1])
    _, _, rows = sref.propagate(*args)
    norm = rows.sum(-1)
    cond = np.linalg.cond(hyd["A0"] - (2j / dt) * hyd["Sd"])
    print("norm drift %.3e over %d steps, population moved %.3e" % (np.max(np.abs(norm - norm[0])), nsteps, rows[0, 0] - rows[-1, 0]))
    assert abs(norm[0] - 1.0) <= 64 * EPS and rows[0, 0] - rows[-1, 0] > 1e-4
    assert np.max(np.abs(norm - norm[0])) <= nsteps * 2 * n * EPS * cond
    Wb = host.band_symmetric(hyd["SB"])[None] * 0.05                               # W = 0.05 S: every state decays at the rate 0.1
    _, _, rows_w = sref.propagate(*args, WB=Wb, w=None)
    norm_w = rows_w.sum(-1)
    assert np.all(np.diff(norm_w) < 0.0)
    # Cayley's factor of a mode of energy h, |1 - i tau (h - 0.05 i)|^2 / |1 + i tau (h - 0.05 i)|^2, leaves exp(-0.1 dt) by a relative
    # 0.2 tau (tau h)^2 + O(dt^3) per step: 6e-6 at |h| = 0.5, 2.5e-4 over the run
    assert abs(norm_w[-1] / np.exp(-0.1 * nsteps * dt) - 1.0) <= 5e-4
    assert np.allclose(host.spline_yield(rows_w[:, None]), 1.0 - norm_w[:, None], rtol=0, atol=0)


def test_second_order_against_expm_on_a_constant_field(hyd):
    """F = 0.05 constant, T = 4 from 1s: the largest coefficient error against exp(-i S^-1 A T) c0 at dt = 0.1, 0.05, 0.025 falls by 4
    per halving; window 3.9 .. 4.1 as in the pulse test below"""
    n, T = hyd["n"], 4.0
    A = hyd["A0"] + 0.05 * hyd["A1"]
    exact = scipy.linalg.expm(-1j * T * np.linalg.solve(hyd["Sd"], A)) @ hyd["c1s"].ravel()
    coef1 = 0.05 * hyd["pat"][1][:, None]
    errs = []
    for dt in (0.1, 0.05, 0.025):
        ns = int(round(T / dt))
        c, _, _ = sref.propagate(hyd["SB"], hyd["HB"], [0, 1], dt, hyd["c1s"], np.broadcast_to(coef1, (ns, 2, 1)), hyd["pat"][0], hyd["RB"][:1])
        errs.append(np.max(np.abs(c.ravel() - exact)))
    print("errors %s ratios %.4f %.4f" % (errs, errs[0] / errs[1], errs[1] / errs[2]))
    assert errs[0] > 1e-7
    assert 3.9 <= errs[0] / errs[1] <= 4.1 and 3.9 <= errs[1] / errs[2] <= 4.1


def test_second_order_through_a_pulse(hyd):
    """The measurement behind test_gpu_tdse_spline's order test, with the dense restatement in place of the GPU call: from 1s through
    tdse_spline_ref.pulse; reference DOP853 (rtol 1e-13) on i S dc/dt = A(t) c; the largest error of the populations |phi_s^T S c|^2
    over all 130 states at dt = 0.1 against dt = 0.05.  Measured: errors 1.451e-05 and 3.630e-06, ratio 3.9982 (3.9928 at dt = 0.2,
    3.9996 at dt = 0.05).  Window 3.9 .. 4.1: C dt^2 (1 + O(dt^2)) leaves 4 by a relative O(dt^2)."""
    from scipy.integrate import solve_ivp
    n, T = hyd["n"], sref.PULSE["T"]
    pat = host.stark_system(CHANS, -1.0)                       # the sign tdse_system's blocks carry; A1 was built with +1
    Si = np.linalg.inv(hyd["Sd"])
    L0, L1 = -1j * Si @ hyd["A0"], 1j * Si @ hyd["A1"]
    sol = solve_ivp(lambda t, y: (L0 + float(sref.pulse(t)) * L1) @ y, (0.0, T), hyd["c1s"].ravel(), method="DOP853", rtol=1e-13, atol=1e-15)
    assert sol.status == 0
    pref = sref.populations(hyd["SB"], sol.y[:, -1].reshape(2, n), hyd["V"])
    assert abs(pref.sum() - 1.0) <= 1e-11 and pref[1, 0] > 1e-3
    errs = []
    for dt in (0.1, 0.05):
        ns = int(round(T / dt))
        coef = host.spline_coefficients(pat, sref.pulse(host.spline_midpoints(0.0, dt, ns)))[:, 0]
        c, _, _ = sref.propagate(hyd["SB"], hyd["HB"], [0, 1], dt, hyd["c1s"], coef, pat[0], hyd["RB"][:1])
        errs.append(np.max(np.abs(sref.populations(hyd["SB"], c, hyd["V"]) - pref)))
    print("population errors %.3e %.3e ratio %.4f" % (errs[0], errs[1], errs[0] / errs[1]))
    assert 3.9 <= errs[0] / errs[1] <= 4.1
