"""The wide coupled-channel resolvent (bspatom_resolvent_coupled_wide, csrc/resolvent_wide.hip) on the CPU: its names in
capi.EXPORTS, and the systems its GPU tests solve -- Stark levels with 8 and 10 channels, Floquet quasi-energies with 10 and 14
blocks -- through host.coupled_eigenpair with the dense restatement tests/resolvent_coupled_ref.py on the oracle's bands, as
test_resolvent_coupled_cpu.py does for the narrow call; the half-widths of the interleaved matrices.  No GPU."""
import types
import numpy as np
import pytest

import oracle as orc
import resolvent_coupled_ref as cref
from bspatom_amd import capi, host

KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=9, l_ini=0, n0_ini=1, zatom=1.0)   # test_resolvent_cpu's grid, l = 0..9


@pytest.fixture(scope="module")
def hydrogen():
    c = orc.make_cfg(**KW)
    E, c1s, (rt, aind, xg, wg) = orc.solve_all(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 10)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    SBf = np.zeros((2 * c.k - 1, c.nfun))                       # the overlap's full band: S(i, i+d) = S(i+d, i)
    for d in range(c.k):
        SBf[c.k - 1 + d, :c.nfun - d] = SB[d, :c.nfun - d]
        SBf[c.k - 1 - d, d:] = SB[d, :c.nfun - d]
    return dict(E1s=E[0, 0], c1s=c1s, SB=SB, HB=HB, R_r=RB[0], prob=types.SimpleNamespace(SB_full=SBf), n=c.nfun, k=c.k)


def _dense_solver(h, couplings, a):
    """(l, z, B) -> y (nch, n): the dense solve in the documented ordering, in place of Problem.resolvent_coupled_wide"""
    def solver(l, z, B):
        M = cref.dense_matrix(h["SB"], h["HB"], list(l), z, couplings, h["R_r"][None], a)
        return cref.solve(M, B[None], len(l))[0]
    return solver


def test_wide_entry_points_are_exported():
    """the new names are declared (test_library_exports_every_declared_symbol then checks the library) and wrapped"""
    assert "bspatom_resolvent_coupled_wide" in capi.EXPORTS and "bspatom_resolvent_coupled_wide_dev" in capi.EXPORTS
    assert callable(capi.Problem.resolvent_coupled_wide) and callable(capi.Problem.resolvent_coupled_wide_dev)
    assert host.COUPLED_MAX_BAND == 63


@pytest.mark.parametrize("nl", [8, 10])
@pytest.mark.parametrize("F,dev_measured", [(0.005, -3.1e-13), (0.01, -8.1e-11)])
def test_stark_shift_with_many_channels(hydrogen, nl, F, dev_measured):
    """l = 0..7 (bw 71) and l = 0..9 (bw 89): the level connected to 1s against the series within 1e-9, |Im| <= 1e-15, the bounds of
    the 4-channel test; the deviation itself, -3.1e-13 and -8.1e-11 for both channel counts (the floor and the F^8 remainder), is
    pinned within 2e-12 (the floor's own size: eps times a few hundred operations on numbers of order 1)"""
    h = hydrogen
    couplings, a = host.stark_system([(l, 0) for l in range(nl)], F)
    x0 = np.zeros((nl, h["n"])); x0[0] = h["c1s"]
    lam, x, hist = host.coupled_eigenpair(h["prob"], list(range(nl)), couplings, h["R_r"], a, -0.5, x0, iters=3,
                                          solver=_dense_solver(h, couplings, a))
    dev = lam.real - cref.stark_series(h["E1s"], F)
    print("l = 0..%d F %.3f: lambda %.16f  deviation %.3e (measured: %.1e)" % (nl - 1, F, lam.real, dev, dev_measured))
    assert abs(lam.imag) <= 1e-15 and abs(dev) <= 1e-9
    assert abs(dev - dev_measured) <= 2e-12
    assert abs(hist[1] - hist[2]) <= 1e-13


@pytest.mark.parametrize("nphot,nblk,lam_measured", [(2, 10, -0.5000370831994085), (3, 14, -0.5000370799559866)])
def test_floquet_quasi_energy_with_many_blocks(hydrogen, nphot, nblk, lam_measured):
    """l = 0..3, omega = 0.2, F = 0.005, two and three photons either side: the quasi-energy next to E_1s, pinned within 1e-13 (the
    bar of the CPU tests on this iteration; two dense orderings differ by at most 5.6e-16)"""
    h = hydrogen
    blocks, zoff, couplings, a = host.floquet_system([(0, 0), (1, 0), (2, 0), (3, 0)], nphot, 0.2, 0.005)
    assert len(blocks) == nblk and nblk * h["k"] - 1 > host.COUPLED_MAX_BAND
    l = [b[0][0] for b in blocks]
    x0 = np.zeros((nblk, h["n"])); x0[blocks.index(((0, 0), 0))] = h["c1s"]
    lam, _, hist = host.coupled_eigenpair(h["prob"], l, couplings, h["R_r"], a, -0.5, x0, zoff=zoff, iters=3,
                                          solver=_dense_solver(h, couplings, a))
    print("nphot %d: lambda %.16f %+.1e i (measured: %.16f)" % (nphot, lam.real, lam.imag, lam_measured))
    assert abs(lam - lam_measured) <= 1e-13
    assert abs(hist[1] - hist[2]) <= 1e-13


def test_half_widths_of_the_wide_systems(hydrogen):
    """the interleaved matrices of the 10-, 14- and 27-block Floquet systems are banded within nch k - 1 (measured: 83, 115, 220
    against 89, 125, 242: the outermost blocks couple to one side only)"""
    h = hydrogen
    for chans, nphot, nblk, hw_measured in (([0, 1, 2, 3], 2, 10, 83), ([0, 1, 2, 3], 3, 14, 115), ([0, 1, 2, 3, 4, 5], 4, 27, 220)):
        blocks, zoff, couplings, a = host.floquet_system([(l, 0) for l in chans], nphot, 0.2, 0.005)
        assert len(blocks) == nblk
        M = cref.dense_matrix(h["SB"], h["HB"], [b[0][0] for b in blocks], -0.5 + zoff, couplings, h["R_r"][None], a)
        hw = cref.half_width(M, nblk)
        assert hw == hw_measured and hw <= nblk * h["k"] - 1 <= 255
