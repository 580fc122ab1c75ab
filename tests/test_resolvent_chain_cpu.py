"""The physics of the resolvent chains (host.cauchy_moments / two_photon / response_chain) pinned on the CPU: the oracle's bands, the
dense restatement tests/resolvent_ref.py and the chain's own restatement tests/resolvent_chain_ref.py (the band apply between two
stages in the arithmetic include/bspatom.h fixes).  Hydrogen, linear grid, rb = 40, k = 9, nfun = 96, channels 0 .. 2.  No GPU."""
import numpy as np
import pytest
import scipy.linalg

import oracle as orc
import resolvent_ref as ref
import resolvent_chain_ref as cref
from bspatom_amd import host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=2, l_ini=0, n0_ini=1, zatom=1.0)
EPS = np.finfo(np.float64).eps


def full_from_upper(UB):
    """the full band (2k-1, n) of the symmetric matrix with upper band UB[d, i] = A(i, i + d)"""
    k, n = UB.shape
    FB = np.zeros((2 * k - 1, n))
    for d in range(k):
        FB[k - 1 + d, :n - d] = UB[d, :n - d]
        FB[k - 1 - d, d:] = UB[d, :n - d]
    return FB


@pytest.fixture(scope="module")
def hydrogen():
    c = orc.make_cfg(**KW)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg)
    assert HB.shape[0] == 3
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    S = ref.upper_to_dense(SB)
    E, Z = [], []
    for l in range(3):
        lam, V = scipy.linalg.eigh(ref.upper_to_dense(HB[l]), S)
        V = V * np.sign(V[np.argmax(np.abs(V) > 1e-8, axis=0), np.arange(V.shape[1])])    # u(r) > 0 near the origin
        E.append(lam); Z.append(V.T.copy())
    b = ref.band_apply(RB[0], Z[0][0][None, :])[0]             # r |1s>
    return dict(SB=SB, HB=HB, RB=RB, E=E, Z=Z, b=b, SF=full_from_upper(SB))


def test_cauchy_moments_are_the_rationals(hydrogen):
    """(2/3) b^T (G S)^(m-1) G b at z = E_1s, G = (H_1 - E_1s S)^-1, from one three-stage chain with the overlap in between: 9/2, 43/4,
    319/12, each to 1e-10, and so the sums over states.  Measured with scipy's E_1s: 4.499999999998780, 10.749999999995538,
    26.583333333318556; the sums over states 4.499999999998655, 10.749999999995108, 26.583333333317476."""
    h = hydrogen
    E1s = h["E"][0][0]
    xs = cref.chain(h["SB"], h["HB"], [1, 1, 1], [E1s] * 3, h["b"], GB=h["SF"][None], a=np.ones((2, 1)))
    mom = [(2.0 / 3.0) * complex(np.sum(h["b"] * x[0])) for x in xs]
    # the sums over states: (2/3) sum_n (c_n^T b)^2 / (E_n - E_1s)^m
    ov = (h["Z"][1] @ h["b"]) ** 2
    sos = [(2.0 / 3.0) * np.sum(ov / (h["E"][1] - E1s) ** m) for m in (1, 2, 3)]
    for m, (v, s, exact) in enumerate(zip(mom, sos, (4.5, 43.0 / 4.0, 319.0 / 12.0)), 1):
        print("moment %d: chain %.15f  sum over states %.15f  exact %.15f" % (m, v.real, s, exact))
        assert abs(v - exact) <= 1e-10, m
        assert abs(s - exact) <= 1e-10, m


def test_two_photon_1s_2s(hydrogen):
    """(1/3) <2s| r G_1((E_1s + E_2s)/2) r |1s> = -7.853655422691 (the literature's -7.8537): against the sum over the l = 1 states to
    1e-10, against -7.85366 to 1e-5."""
    h = hydrogen
    E1s, E2s = h["E"][0][0], h["E"][0][1]
    p = ref.band_apply(h["RB"][0], h["Z"][0][1][None, :])[0]   # r |2s>
    z = 0.5 * (E1s + E2s)
    amp = ref.response(h["SB"], h["HB"][1], z, h["b"], p=p) / 3.0
    sos = np.sum((h["Z"][1] @ p) * (h["Z"][1] @ h["b"]) / (h["E"][1] - z)) / 3.0
    print("1s-2s: solve %.12f %+.1e i  sum over states %.12f  difference %.2e" % (amp.real, amp.imag, sos, amp.real - sos))
    assert abs(amp - sos) <= 1e-10
    assert abs(amp - (-7.85366)) <= 1e-5


@pytest.mark.parametrize("dz", [(0.3 + 0.05j, 0.6 + 0.05j)])
def test_two_stage_chain_against_double_sum(hydrogen, dz):
    """b^T G_2(z2) r G_1(z1) b, z = E_1s + dz, through l = 1 and then l = 2.  Three CPU routes: (A) dense -- numpy.linalg.solve and
    the dense r matrix with `@`; (B) the double sum over the states of both channels; (C) resolvent_chain_ref.chain, the
    restatement the GPU tests compare with.  d = |A - B| is recomputed here (measured 1.0e-10 on a value of 408, 175 eps sum |terms|);
    (C) agrees with (B) within 8 max(d, eps sum |terms|) (measured 1.02e-10)."""
    h = hydrogen
    E1s = h["E"][0][0]
    z1, z2 = E1s + dz[0], E1s + dz[1]
    b = h["b"]
    Rd = ref.full_to_dense(h["RB"][0])
    x1 = ref.solve(h["SB"], h["HB"][1], z1, b)[0]
    A = complex(np.sum(b * ref.solve(h["SB"], h["HB"][2], z2, Rd @ x1)[0]))
    Z1, Z2 = h["Z"][1], h["Z"][2]
    terms = ((Z2 @ b) / (h["E"][2] - z2))[:, None] * (Z2 @ Rd @ Z1.T) * ((Z1 @ b) / (h["E"][1] - z1))[None, :]
    Bv, mass = complex(np.sum(terms)), float(np.sum(np.abs(terms)))
    d = abs(A - Bv)
    xs = cref.chain(h["SB"], h["HB"], [1, 2], [z1, z2], b, GB=h["RB"][:1], a=np.ones((1, 1)))
    Cv = complex(np.sum(b * xs[1][0]))
    print("two-stage chain: dense %s  double sum %s  chain %s  d %.3e = %.1f eps sum|terms|  |C - B| %.3e"
          % (A, Bv, Cv, d, d / (EPS * mass), abs(Cv - Bv)))
    assert abs(Cv - Bv) <= 8.0 * max(d, EPS * mass)
    assert abs(Bv) > 1.0


def test_host_band_apply_is_the_chain_arithmetic():
    """host.band_apply on real input equals band_combine_apply with a = (1,) bit for bit; with two operators the combination is
    formed entry by entry before the product (differs from the sum of two applies in the last bits, agrees to rounding)."""
    rng = np.random.default_rng(11)
    G, X = rng.standard_normal((2, 7, 23)), rng.standard_normal((3, 23))
    Y = cref.band_combine_apply(G[:1], (1.0,), X)
    assert np.array_equal(Y.real, host.band_apply(G[0], X)) and np.all(Y.imag == 0.0) and not np.any(np.signbit(Y.imag))
    Xc = X + 1j * rng.standard_normal((3, 23))
    a = (0.75, -1.5)
    Yc = cref.band_combine_apply(G, a, Xc)
    assert np.array_equal(Yc.real, cref.band_combine_apply(G, a, Xc.real).real)           # the components are independent
    assert np.array_equal(Yc.imag, cref.band_combine_apply(G, a, Xc.imag).real)
    dense = a[0] * ref.full_to_dense(G[0]) + a[1] * ref.full_to_dense(G[1])
    assert np.allclose(Yc, (dense @ Xc.T).T, rtol=1e-13, atol=1e-13)
