"""The physics of the resolvent helpers (host.response / polarizability / photoabsorption) pinned on the CPU: the oracle's bands
(oracle.assemble_bands, oracle.dipole_bands), the absorber's band by quadrature, and the dense restatement tests/resolvent_ref.py.
Hydrogen, linear grid, rb = 40, k = 9, nfun = 96.  No GPU."""
import numpy as np
import pytest

import oracle as orc
import resolvent_ref as ref
from bspatom_amd import host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)


@pytest.fixture(scope="module")
def hydrogen():
    c = orc.make_cfg(**KW)
    E, c1s, (rt, aind, xg, wg) = orc.solve_all(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    b = ref.band_apply(RB[0], c1s[None, :])[0]                 # r |1s>
    return dict(c=c, E=E, SB=SB, HB=HB, b=b, rt=rt, xg=xg, wg=wg)


def test_c1_static_polarizability(hydrogen):
    """C1: (2/3) b^T (H_1 - E_1s S)^-1 b = 4.5 (measured 4.499999999998781); the solve equals the sum over all l = 1 states
    (measured difference 1.3e-13)."""
    h = hydrogen
    E1s = h["E"][0, 0]
    alpha = (2.0 / 3.0) * ref.response(h["SB"], h["HB"][1], E1s, h["b"])
    print("alpha(0) = %.15f + %.1e i, error %.2e" % (alpha.real, alpha.imag, alpha.real - 4.5))
    assert abs(alpha - 4.5) <= 1e-10
    # the sum over states: every eigenpair of the l = 1 pencil
    import scipy.linalg
    lam, Z = scipy.linalg.eigh(ref.upper_to_dense(h["HB"][1]), ref.upper_to_dense(h["SB"]))
    sos = (2.0 / 3.0) * np.sum((Z.T @ h["b"]) ** 2 / (lam - E1s))
    print("sum over states %.15f, difference %.2e" % (sos, alpha.real - sos))
    assert abs(alpha.real - sos) <= 1e-11


def test_c2_photoabsorption_closed_form(hydrogen):
    """C2: absorber cap_profile(r, 20, 1e-3): sigma(omega) = 4 pi omega Im alpha / c against the closed form for H(1s); measured
    relative deviations -3.6e-2, -2.5e-3, -1.2e-2, -4.9e-2 at omega = 0.55, 0.7, 1.0, 1.5 (the absorber's own reflection)."""
    h = hydrogen
    WB = ref.operator_band(h["rt"], h["c"].k, h["xg"], h["wg"], lambda r: host.cap_profile(r, 20.0, 1e-3))
    # the CPU quadrature is the assembly's: the overlap band it gives is the oracle's
    S1 = ref.operator_band(h["rt"], h["c"].k, h["xg"], h["wg"], lambda r: np.ones_like(r))
    assert np.max(np.abs(S1[h["c"].k - 1:] - h["SB"])) <= 1e-13
    E1s = h["E"][0, 0]
    for omega in (0.55, 0.7, 1.0, 1.5):
        alpha = (ref.response(h["SB"], h["HB"][1], E1s + omega, h["b"], WB=WB) + ref.response(h["SB"], h["HB"][1], E1s - omega, h["b"], WB=WB)) / 3.0
        sigma = 4.0 * np.pi * omega * alpha.imag / ref.C_AU
        dev = sigma / ref.sigma_h1s(omega) - 1.0
        print("omega %.2f: sigma %.6e, closed form %.6e, relative deviation %.2e" % (omega, sigma, ref.sigma_h1s(omega), dev))
        assert abs(dev) <= 6e-2


def test_host_band_apply_is_the_restatement():
    rng = np.random.default_rng(3)
    A, X = rng.standard_normal((7, 23)), rng.standard_normal((3, 23))
    assert np.array_equal(host.band_apply(A, X), ref.band_apply(A, X))
    Xc = X + 1j * rng.standard_normal((3, 23))
    assert np.allclose(host.band_apply(A, Xc), (ref.full_to_dense(A) @ Xc.T).T, rtol=1e-13, atol=1e-13)
