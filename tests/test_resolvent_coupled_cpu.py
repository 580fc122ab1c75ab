"""The host helpers of the coupled-channel resolvent (host.band_transpose / coupled_dense / stark_system / floquet_system /
coupled_eigenpair) pinned on the CPU: the oracle's bands on test_resolvent_cpu's hydrogen grid (rb = 40, k = 9, nfun = 96), l = 0..3,
the dense restatement tests/resolvent_coupled_ref.py standing in for the GPU call.  No GPU."""
import types
import numpy as np
import pytest

import oracle as orc
import resolvent_ref as ref
import resolvent_coupled_ref as cref
from bspatom_amd import host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=3, l_ini=0, n0_ini=1, zatom=1.0)


@pytest.fixture(scope="module")
def hydrogen():
    c = orc.make_cfg(**KW)
    E, c1s, (rt, aind, xg, wg) = orc.solve_all(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 4)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    SBf = np.zeros((2 * c.k - 1, c.nfun))                       # the overlap's full band: S(i, i+d) = S(i+d, i)
    for d in range(c.k):
        SBf[c.k - 1 + d, :c.nfun - d] = SB[d, :c.nfun - d]
        SBf[c.k - 1 - d, d:] = SB[d, :c.nfun - d]
    return dict(c=c, E=E, c1s=c1s, SB=SB, HB=HB, RB=RB, SBf=SBf, n=c.nfun, k=c.k)


def _dense_solver(h, couplings, G, a):
    """(l, z, B) -> y (nch, n): the dense solve in the documented ordering, in place of Problem.resolvent_coupled"""
    def solver(l, z, B):
        M = cref.dense_matrix(h["SB"], h["HB"], list(l), z, couplings, np.asarray(G).reshape(-1, 2 * h["k"] - 1, h["n"]), a)
        return cref.solve(M, B[None], len(l))[0]
    return solver


def test_band_transpose_against_dense():
    rng = np.random.default_rng(11)
    G = rng.standard_normal((2, 7, 23))
    for d in range(-3, 4):                                      # a full band is zero where i + d leaves the matrix
        G[:, d + 3, :max(0, -d)] = 0.0
        G[:, d + 3, 23 - max(0, d):] = 0.0
    T = host.band_transpose(G)
    for o in range(2):
        assert np.array_equal(ref.full_to_dense(T[o]), ref.full_to_dense(G[o]).T)
    assert np.array_equal(host.band_transpose(T), G)
    assert np.array_equal(host.band_transpose(G[0]), T[0])      # one band, no leading axis


def test_coupled_dense_against_hand_built_blocks(hydrogen):
    """three channels l = (0, 1, 0) with their own energies, an absorber on channel 1 alone, a complex nearest-neighbour coupling with
    its transposed partner, an in-channel entry of two operators: every block against its formula; the interleaved matrix is banded
    with half-width <= nch k - 1"""
    h = hydrogen
    n, k = h["n"], h["k"]
    S, H0, H1 = ref.upper_to_dense(h["SB"]), ref.upper_to_dense(h["HB"][0]), ref.upper_to_dense(h["HB"][1])
    Wb = np.abs(h["RB"][0]) * 1e-3
    G = np.stack([h["RB"][0], h["RB"][2]])
    Rr, Dr, Wd = ref.full_to_dense(G[0]), ref.full_to_dense(G[1]), ref.full_to_dense(Wb)
    z = np.array([0.3 + 0.05j, 0.1, -0.2 - 0.01j])
    couplings = [(0, 1, 0), (1, 0, 1), (2, 2, 0), (1, 2, 1)]
    a = np.array([[0.7 + 0.2j, 0.0], [0.7 - 0.2j, 0.0], [0.25, -0.5j], [0.0, 1.5]])
    M = host.coupled_dense(h["SB"], h["HB"], [0, 1, 0], z, couplings, G, a, W=Wb, w=[-1, 0, -1])
    Z = np.zeros((n, n))
    blocks = [[H0 - z[0] * S, (0.7 + 0.2j) * Rr, Z],
              [(0.7 - 0.2j) * Rr.T, H1 - 1j * Wd - z[1] * S, 1.5 * Dr.T],
              [Z, Z, H0 - z[2] * S + 0.25 * Rr - 0.5j * Dr]]
    assert M.shape == (3 * n, 3 * n) and M.dtype == np.complex128
    assert np.allclose(M, np.block(blocks), rtol=1e-15, atol=0.0)
    assert np.array_equal(M, cref.dense_matrix(h["SB"], h["HB"], [0, 1, 0], z, couplings, G, a, Wb[None], [-1, 0, -1]))
    assert cref.half_width(M, 3) <= 3 * k - 1
    # the same without couplings, w None: the absorber on every channel
    M0 = host.coupled_dense(h["SB"], h["HB"], [1, 1], [0.1, 0.2], None, None, None, W=Wb)
    assert np.allclose(M0[:n, :n], H1 - 1j * Wd - 0.1 * S, rtol=1e-15, atol=0.0) and not np.any(M0[:n, n:])


def test_stark_system_factors():
    """m = 0: the factor between l and l + 1 is F (l+1) / sqrt((2l+1)(2l+3)); both directions, the second as the transpose"""
    F = 0.37
    couplings, a = host.stark_system([(0, 0), (1, 0), (2, 0), (3, 0)], F)
    assert couplings == [(0, 1, 0), (1, 0, 1), (1, 2, 0), (2, 1, 1), (2, 3, 0), (3, 2, 1)]
    want = [F * (l + 1) / np.sqrt((2 * l + 1) * (2 * l + 3)) for l in (0, 0, 1, 1, 2, 2)]
    assert a.dtype == np.complex128 and np.all(a.imag == 0.0)
    assert np.allclose(a.real, want, rtol=1e-15, atol=0.0)
    assert host.stark_system([(0, 0), (2, 0)], F)[0] == []      # no dipole coupling between l = 0 and l = 2


def test_floquet_system_blocks():
    blocks, zoff, couplings, a = host.floquet_system([(0, 0), (1, 0)], 1, 0.2, 0.005)
    assert blocks == [((1, 0), -1), ((0, 0), 0), ((1, 0), 1)]
    assert np.array_equal(zoff, [0.2, 0.0, -0.2])
    assert couplings == [(0, 1, 0), (1, 0, 1), (1, 2, 0), (2, 1, 1)]
    assert np.allclose(a, 0.0025 / np.sqrt(3.0), rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("F,dev_measured", [(0.005, 3e-13), (0.01, 8e-11)])
def test_stark_shift_through_coupled_eigenpair(hydrogen, F, dev_measured):
    """The level connected to 1s in a field F, l = 0..3, by coupled_eigenpair(solver = dense) at shift -0.5 from (c_1s, 0, 0, 0),
    against E_1s - (9/4) F^2 - (3555/64) F^4 - (2512779/512) F^6 within 1e-9 (the deviations measured with dense SciPy, 3e-13 and
    8e-11, are the numerical floor and the F^8 remainder); converged to 1e-13 after two solves."""
    h = hydrogen
    n = h["n"]
    couplings, a = host.stark_system([(0, 0), (1, 0), (2, 0), (3, 0)], F)
    x0 = np.zeros((4, n)); x0[0] = h["c1s"]
    prob = types.SimpleNamespace(SB_full=h["SBf"])
    lam, x, hist = host.coupled_eigenpair(prob, [0, 1, 2, 3], couplings, h["RB"][0], a, -0.5, x0, iters=3,
                                          solver=_dense_solver(h, couplings, h["RB"][0], a))
    want = cref.stark_series(h["E"][0, 0], F)
    print("F %.3f: lambda %.15f  series %.15f  deviation %.2e (measured with SciPy: %.0e)  steps %s"
          % (F, lam.real, want, lam.real - want, dev_measured, [abs(v - lam) for v in hist]))
    assert abs(lam.imag) <= 1e-15 and abs(lam.real - want) <= 1e-9
    assert abs(hist[1] - hist[2]) <= 1e-13
    assert abs(np.sum(x * ref.band_apply(h["SBf"], x)) - 1.0) <= 1e-12


def test_floquet_shift_through_coupled_eigenpair(hydrogen):
    """Three Floquet blocks (l = 0 at n = 0, l = 1 at n = +-1), omega = 0.2, F = 0.005: the quasi-energy shift against
    -alpha(omega) F^2 / 4, alpha from the dense single-channel resolvents, within 1e-3 relative (2.0e-4 measured: the F^4 term)."""
    h = hydrogen
    n, om, F = h["n"], 0.2, 0.005
    E1s = h["E"][0, 0]
    blocks, zoff, couplings, a = host.floquet_system([(0, 0), (1, 0)], 1, om, F)
    l = [b[0][0] for b in blocks]
    x0 = np.zeros((3, n)); x0[1] = h["c1s"]
    prob = types.SimpleNamespace(SB_full=h["SBf"])
    lam, _, hist = host.coupled_eigenpair(prob, l, couplings, h["RB"][0], a, -0.5, x0, zoff=zoff, iters=3,
                                          solver=_dense_solver(h, couplings, h["RB"][0], a))
    b = ref.band_apply(h["RB"][0], h["c1s"][None, :])[0]
    alpha = (ref.response(h["SB"], h["HB"][1], E1s + om, b) + ref.response(h["SB"], h["HB"][1], E1s - om, b)).real / 3.0
    shift, want = lam.real - E1s, -alpha * F * F / 4.0
    print("alpha(0.2) = %.5f  shift %.6e  -alpha F^2 / 4 = %.6e  relative difference %.2e" % (alpha, shift, want, shift / want - 1.0))
    assert abs(alpha - 5.94167) <= 1e-4
    assert abs(shift / want - 1.0) <= 1e-3
    assert abs(hist[1] - hist[2]) <= 1e-13
