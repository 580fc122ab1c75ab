"""The window operator on spline packets without a GPU: the header part and its exports, host.window_shifts against the polynomial
it factors, the solve chain of tests/spline_window_ref.py against the spectral sum, the normalisation of host.window_density and
host.window_yield.  The pencils are tests/pencils.py's; the GPU side is tests/test_gpu_spline_window.py."""
import os
import re
import types
import numpy as np
import pytest

import pencils
import spline_window_ref as wref
from bspatom_amd import capi, host

EPS = float(np.finfo(np.float64).eps)


def test_header_part_is_included_and_its_symbols_are_exported():
    """include/bspatom_spline_window.h is part of include/bspatom.h (included there, refuses to stand alone); what it declares is
    capi.WINDOW_EXPORTS, and the library exports it with the argument list the header gives (10 arguments); BSPATOM_WINDOW_MAX_FAC is
    capi.WINDOW_MAX_FAC; window_rhs is an option"""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    main = open(os.path.join(inc, "bspatom.h")).read()
    assert '#include "bspatom_spline_window.h"' in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    part = open(os.path.join(inc, "bspatom_spline_window.h")).read()
    assert "#ifndef BSPATOM_H\n#error" in part
    code = re.sub(r"/\*.*?\*/", "", part, flags=re.S)
    decl = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(bspatom_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", code))
    assert sorted(decl) == sorted(capi.WINDOW_EXPORTS)
    lib = capi.lib()
    for name, params in decl.items():
        assert hasattr(lib, name) and name not in capi.EXPORTS + capi.SPLINE_EXPORTS + capi.SPLIT_EXPORTS + capi.EXPECT_EXPORTS
        assert len(params.split(",")) == len(getattr(lib, name).argtypes) == 10, name
    assert int(re.search(r"#define\s+BSPATOM_WINDOW_MAX_FAC\s+(\d+)", code).group(1)) == capi.WINDOW_MAX_FAC == 8
    for name in ("spline_window", "spline_window_dev"):
        assert callable(getattr(capi.Problem, name))
    capi.set_option("window_rhs", 3)
    assert capi.get_option("window_rhs") == 3
    capi.set_option("window_rhs", 0)


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_window_shifts_factor_the_polynomial(m):
    """prod_j (lam - z_j)(lam - conj z_j) = (lam - E)^(2m) + gamma^(2m) at real and complex lam, for m = 1 .. 4: every factor and the
    polynomial are O(1) here, the product of 2m factors rounds 2m times and each z_j carries an ulp or two, so the relative deviation
    stays below 8 m eps (largest seen: 3 eps).  Every shift lies in the upper half plane at distance gamma from E."""
    E, gamma = np.array([-0.4, 0.3, 2.5]), 0.37
    z = host.window_shifts(E, gamma, m)
    assert z.shape == (3, m) and z.dtype == np.complex128 and z.flags.c_contiguous
    assert np.all(z.imag > 0.0) and np.max(np.abs(np.abs(z - E[:, None]) - gamma)) <= 4 * EPS
    worst = 0.0
    for lam in (-1.3, 0.0, 0.31, 1.7 + 0.4j, 2.5 - 0.2j):
        prod = np.prod((lam - z) * (lam - np.conj(z)), axis=1)
        poly = (lam - E) ** (2 * m) + gamma ** (2 * m)
        worst = max(worst, float(np.max(np.abs(prod - poly) / np.abs(poly))))
    print("m %d: largest relative deviation %.2e (%.1f eps)" % (m, worst, worst / EPS))
    assert worst <= 8 * m * EPS
    assert host.window_shifts(0.3, gamma, m).shape == (1, m)
    for bad in (dict(gamma=0.0, m=2), dict(gamma=-1.0, m=2), dict(gamma=0.1, m=0)):
        with pytest.raises(ValueError):
            host.window_shifts(E, **bad)


def _pencil(n=24, p=3, seed=11):
    lams = np.linspace(-1.0, 1.0, n) ** 3 + 0.1 * np.linspace(0.0, 1.0, n)      # dense near 0.05, sparse at the ends
    H, S = pencils.make_pencil(lams, p, seed)
    rng = np.random.default_rng(seed + 1)
    c = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(n)
    return H, S, c, p


@pytest.mark.parametrize("m", [1, 2, 4])
def test_solve_chain_equals_the_spectral_sum(m):
    """gamma^(2m) x_m^H S x_m from the dense and from the banded solve chain against sum_n |x_n^T S c|^2 gamma^(2m) / ((E_n - E)^(2m) +
    gamma^(2m)) from scipy.linalg.eigh, on a pencil of n = 24, half-width 3, at 41 energies across and beyond the spectrum, gamma =
    0.05.  Tolerance: a stage is a solve with M = H - z S, whose relative error is about n eps kappa(M), kappa(M) <= kappa(S) (|E_n -
    z|_max / gamma) since the generalised eigenvalues of M are E_n - z and |E_n - z| >= gamma; m stages and the quadratic form double
    it: 2 m n eps kappa(S) (spread + gamma) / gamma, relative to the largest P of the scan.  (Measured: below 1e-3 of it.)"""
    H, S, c, p = _pencil()
    n, gamma = H.shape[0], 0.05
    w, X = wref.eigen(H, S)
    E = np.linspace(w[0] - 0.1, w[-1] + 0.1, 41)
    z = host.window_shifts(E, gamma, m)
    Ps = np.array([gamma ** (2 * m) * wref.spectral(w, X, S, c, z[e]) for e in range(E.size)])
    Pd = np.array([gamma ** (2 * m) * wref.chain_dense(H, S, c, z[e]) for e in range(E.size)])
    Pb = np.array([gamma ** (2 * m) * wref.chain_banded(H, S, c, z[e], p) for e in range(E.size)])
    tol = 2 * m * n * EPS * np.linalg.cond(S) * (w[-1] - w[0] + 0.2 + gamma) / gamma * np.max(Ps)
    err = max(float(np.max(np.abs(Pd - Ps))), float(np.max(np.abs(Pb - Ps))))
    print("m %d: |chain - spectral| %.3e, tolerance %.3e, largest P %.3e" % (m, err, tol, np.max(Ps)))
    assert 0.0 < np.min(Ps) and np.max(Ps) <= float(np.real(np.vdot(c, S @ c))) * (1 + 1e-12)     # a window is at most 1
    assert err <= tol


def _fake_problem(H, S, info=0):
    """what host.window_spectrum needs of a Problem: spline_window by the dense chain, one matrix for every l"""
    def spline_window(l, c, z):
        c = np.asarray(c, dtype=np.complex128)
        one = c.ndim == 2
        c = c.reshape(-1, len(l), H.shape[0])
        N = np.array([[[wref.chain_dense(H, S, c[q, ch], z[e]) for e in range(z.shape[0])] for ch in range(len(l))] for q in range(c.shape[0])])
        return (N[0] if one else N), np.full(z.shape[0], info, dtype=np.int32)
    return types.SimpleNamespace(spline_window=spline_window)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_density_integrates_to_the_norm(m):
    """The trapezoid integral of host.window_density(host.window_spectrum(..)) over [E_min - D, E_max + D] with spacing h = gamma / 4
    gives c^H S c.  The density is sum_n |a_n|^2 g(E - E_n), g(x) = (gamma^(2m) / (x^(2m) + gamma^(2m))) / (gamma I_m) of integral 1, and
    sum_n |a_n|^2 = c^H S c; so the relative tolerance is a bound for one g, the sum of
      the two tails beyond distance D:   2 int_D^inf gamma^(2m) x^(-2m) dx / (gamma I_m) = (2 / (2m-1)) (gamma / D)^(2m-1) / I_m;
      the end points' half weights:      2 (h/2) g(D) <= (1/4) (gamma / D)^(2m) / I_m   (beyond D, g decreases: the rule's points outside
                                         the interval sum to less than the tail integral);
      the trapezoid rule on the whole line: by Poisson summation 2 sum_k |g^(2 pi k / h)|, and the transform of 1 / (x^(2m) + 1) is its
                                         m residues in a half plane, each of modulus 2 pi / (2m) times exp(-omega Im z_j) with Im z_j >=
                                         s = sin(pi / 2m): at most pi exp(-omega s); hence 2 pi q / ((1 - q) I_m), q = exp(-2 pi s gamma / h)
                                         = exp(-8 pi s);
      rounding: (number of energies) eps.
    D = 40 gamma, gamma = 0.05: m = 1: 1.6e-2 (the Lorentzian's tails), m = 2: 4.8e-6, m = 3: 1.0e-5 (the trapezoid term).  With an
    (nscan, nch) packet array in front: the same per scan and channel."""
    H, S, c, p = _pencil()
    n, gamma = H.shape[0], 0.05
    w = wref.eigen(H, S)[0]
    D, h = 40 * gamma, gamma / 4
    E = np.arange(w[0] - D, w[-1] + D + h / 2, h)
    c2 = np.stack([c, 0.5 * c[::-1]])[None]                                  # (1, 2, n): two channels of one scan
    P = host.window_spectrum(_fake_problem(H, S), [0, 0], c2, E, gamma, m)
    assert P.shape == (1, 2, E.size)
    dens = host.window_density(P, gamma, m)
    Im = wref.window_integral(m)
    q = np.exp(-8 * np.pi * np.sin(np.pi / (2 * m)))
    tol = (2.0 / (2 * m - 1)) * (gamma / D) ** (2 * m - 1) / Im + 0.25 * (gamma / D) ** (2 * m) / Im + 2 * np.pi * q / ((1 - q) * Im) + E.size * EPS
    for ch in range(2):
        norm = float(np.real(np.vdot(c2[0, ch], S @ c2[0, ch])))
        got = float(np.sum(0.5 * (dens[0, ch, 1:] + dens[0, ch, :-1]) * np.diff(E)))
        print("m %d channel %d: integral / norm - 1 = %.3e, tolerance %.3e" % (m, ch, got / norm - 1, tol))
        assert abs(got - norm) <= tol * norm
        # the whole grid lies above emin: window_yield is that integral
        assert host.window_yield(P, E, gamma, m, emin=E[0] - 1.0)[0, ch] == pytest.approx(got, rel=1e-13)
    with pytest.raises(RuntimeError):
        host.window_spectrum(_fake_problem(H, S, info=1), [0], c, E[:3], gamma, m)


def test_window_yield_integrates_the_density_above_emin():
    """window_yield(P, E, gamma, m, emin) is the trapezoid of P / (gamma I_m) over the grid points E >= emin, per scan and channel;
    the part below and the part above a grid point add up to the whole; no two points above emin: zero; a grid that does not ascend
    or does not match P: ValueError"""
    rng = np.random.default_rng(5)
    E = np.sort(rng.uniform(-1.0, 3.0, 57))
    i0 = int(np.searchsorted(E, 0.0))
    E[i0] = 0.0                                                             # a grid point at emin itself, still ascending
    P = rng.uniform(0.0, 1.0, (3, 2, E.size))
    gamma, m = 0.07, 2
    dens = P / (gamma * np.pi / (m * np.sin(np.pi / (2 * m))))
    assert np.allclose(host.window_density(P, gamma, m), dens, rtol=4 * EPS, atol=0.0)
    trap = lambda lo, hi: np.sum(0.5 * (dens[..., lo + 1:hi] + dens[..., lo:hi - 1]) * np.diff(E[lo:hi]), axis=-1)
    above = host.window_yield(P, E, gamma, m)                               # emin = 0.0: the points i0 ..
    assert above.shape == (3, 2)
    assert np.allclose(above, trap(i0, E.size), rtol=1e-13, atol=0.0)
    assert np.allclose(above + trap(0, i0 + 1), host.window_yield(P, E, gamma, m, emin=-2.0), rtol=1e-13, atol=0.0)
    assert np.allclose(host.window_yield(P, E, gamma, m, emin=0.5 * (E[i0 + 9] + E[i0 + 10])), trap(i0 + 10, E.size), rtol=1e-13, atol=0.0)
    assert np.all(host.window_yield(P, E, gamma, m, emin=E[-1]) == 0.0) and np.all(host.window_yield(P, E, gamma, m, emin=4.0) == 0.0)
    assert host.window_yield(P[0, 0], E, gamma, m).shape == ()
    with pytest.raises(ValueError):
        host.window_yield(P, E[::-1], gamma, m)
    with pytest.raises(ValueError):
        host.window_yield(P, E[:-1], gamma, m)
