"""The host side of the expectation values in the spline basis (Problem.spline_expect, Problem.tdse_split_observe) pinned on the CPU: the
header part and its exports, the two restatements of tests/spline_expect_ref.py against each other on the shapes of the GPU tests'
fixtures, the helpers host.split_expect_dipole / _accel / _rows and host.hhg_spectrum, and the order check of the GPU physics test on
the dense restatement tests/tdse_split_ref.py.  Bands from the oracle; a stand-in for the problem handle gives the helpers what they
ask a Problem for.  No GPU."""
import os
import re
import types
import numpy as np
import pytest
import scipy.linalg

import oracle as orc
import resolvent_ref as ref
import spline_expect_ref as eref
import tdse_spline_ref as sref
import tdse_split_ref as pref
from bspatom_amd import capi, host

EPS = np.finfo(np.float64).eps
# the shapes of the GPU tests' fixtures (tiny8, n65_k4, lin256, k16_n40): n and k on a linear grid, with the channels of their cases
SHAPES = [(8, 4, 2), (65, 4, 3), (256, 9, 4), (40, 16, 4), (65, 4, 1), (256, 9, 29)]


def _bands(n, k, rb=40.0):
    c = orc.make_cfg(kind_grid=0, ra=0.0, rb=rb, k=k, nfun=n, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 2)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    return c, (rt, aind, xg, wg), SB, HB, RB


def _stand_in(c, g, RB, kind_pot=0, zatom=1.0):
    """what the helpers ask a Problem for: dipole_bands, quadrature, operator_bands (deriv 0), inp, nfun, k"""
    rt, aind, xg, wg = g
    r, w = ref.quadrature(rt, xg, wg)
    def operator_bands(gv, deriv):
        assert list(deriv) == [0]
        return ref.operator_band(rt, c.k, xg, wg, lambda rr: np.asarray(gv, dtype=np.float64))[None]
    return types.SimpleNamespace(nfun=c.nfun, k=c.k, dipole_bands=lambda: RB, quadrature=lambda: (r, w), operator_bands=operator_bands,
                                 inp=types.SimpleNamespace(kind_pot=kind_pot, zatom=zatom))


def test_header_part_is_included_and_its_symbols_are_exported():
    """include/bspatom_spline_expect.h is part of include/bspatom.h (included there, refuses to stand alone); what it declares is
    capi.EXPECT_EXPORTS, and the library exports it with the argument lists the header gives: 8 for the measuring call, the 21 of
    bspatom_tdse_split and three more for the observing one"""
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    main = open(os.path.join(inc, "bspatom.h")).read()
    assert '#include "bspatom_spline_expect.h"' in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    part = open(os.path.join(inc, "bspatom_spline_expect.h")).read()
    assert "#ifndef BSPATOM_H\n#error" in part
    code = re.sub(r"/\*.*?\*/", "", part, flags=re.S)
    decl = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(bspatom_[a-z_0-9]+)\s*\(([^;]*)\)\s*;", code))
    assert sorted(decl) == sorted(capi.EXPECT_EXPORTS)
    lib = capi.lib()
    for name, params in decl.items():
        assert hasattr(lib, name) and name not in capi.EXPORTS + capi.SPLINE_EXPORTS + capi.SPLIT_EXPORTS
        assert len(params.split(",")) == len(getattr(lib, name).argtypes) == (8 if "spline_expect" in name else 24), name
    for name in ("spline_expect", "spline_expect_dev", "tdse_split_observe", "tdse_split_observe_dev"):
        assert callable(getattr(capi.Problem, name))


@pytest.mark.parametrize("n,k,nch", SHAPES, ids=["n%d-k%d-nch%d" % s for s in SHAPES])
def test_the_fixed_order_lies_within_the_bound_of_the_definition(n, k, nch):
    """expect_f64, the header's order in float64, against expect_ld, the definition in long double, on random packets (one real) and
    the GPU tests' kinds of operator -- tridiagonal B with the band of r, dense B with a non-symmetric band, B = 1 with the overlap,
    a B with an all-zero row, B = 0 --: |e - e_ld| <= 2 (n + 2 nch + 2k + 4) eps sum |terms|; B = 0 gives exactly +0.0, a real packet
    Im e = +-0.0"""
    c, g, SB, HB, RB = _bands(n, k, 40.0 if n > 8 else 10.0)
    rng = np.random.default_rng(17 + nch)
    off = rng.uniform(0.3, 0.7, max(nch - 1, 0))
    tri = np.diag(rng.uniform(0.1, 0.4, nch)) + np.diag(off, 1) + np.diag(off, -1)
    holed = rng.standard_normal((nch, nch))
    holed[nch // 2] = 0.0
    B = np.stack([tri, rng.standard_normal((nch, nch)), np.eye(nch), holed, np.zeros((nch, nch))])
    GE = np.stack([RB[0], RB[2], host.band_symmetric(SB), RB[2], RB[0]])
    worst = 0.0
    for real in (False, True):
        pk = rng.standard_normal((nch, n)) / np.sqrt(n) + (0.0 if real else 1j) * rng.standard_normal((nch, n)) / np.sqrt(n)
        e = eref.expect_f64(pk, B, GE)
        eld, mag = eref.expect_ld(pk, B, GE)
        for o in range(5):
            err, bound = abs(complex(eld[o]) - e[o]), eref.bound(n, nch, k, mag[o])
            assert err <= bound, (o, err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
        assert e[4].real == 0.0 and e[4].imag == 0.0 and not np.signbit(e[4].real) and not np.signbit(e[4].imag) and mag[4] == 0.0
        if real:
            assert np.all(e.imag == 0.0)
        else:
            assert abs(e[1].imag) > 1e-6                        # a non-symmetric pair is not real
        # B = 1 with S: the norm
        S = ref.upper_to_dense(SB)
        assert abs(e[2] - sum(np.vdot(v, S @ v) for v in pk)) <= eref.bound(n, nch, k, mag[2])
    print("n %d k %d nch %d: worst |e_f64 - e_ld| / bound %.3g" % (n, k, nch, worst))
    assert 0.0 < worst


def test_helper_algebra():
    """split_expect_dipole: B the cos theta matrix of stark_system(channels, 1.0), GE the band of r, both symmetric, so e is real to
    rounding; the band of g d/dr is not symmetric and Im e != 0.  split_expect_accel: the same B, the band of zatom / r^2; another
    potential without a profile raises ValueError, a profile or a callable is taken.  split_expect_rows inverts the row layout."""
    c, g, SB, HB, RB = _bands(65, 4)
    prob = _stand_in(c, g, RB)
    chans = [(0, 0), (1, 0), (2, 0)]
    B, GE = host.split_expect_dipole(prob, chans)
    assert B.shape == (1, 3, 3) and GE.shape == (1, 7, 65) and np.array_equal(B[0], B[0].T)
    sym = lambda F: float(np.max(np.abs(ref.full_to_dense(F) - ref.full_to_dense(F).T)) / np.max(np.abs(F)))
    assert sym(GE[0]) <= 64 * EPS and np.array_equal(GE[0], RB[0])     # the two triangles are summed separately: symmetric to rounding
    assert abs(B[0, 0, 1] - 1.0 / np.sqrt(3.0)) <= 2 * EPS and abs(B[0, 1, 2] - 2.0 / np.sqrt(15.0)) <= 2 * EPS and B[0, 0, 2] == 0.0
    Q, lam = host.split_angular(chans)
    assert np.max(np.abs(Q @ np.diag(lam) @ Q.T - B[0])) <= 8 * EPS
    rng = np.random.default_rng(2)
    pk = (rng.standard_normal((3, 65)) + 1j * rng.standard_normal((3, 65))) / 8.0
    e = eref.expect_f64(pk, B, GE)
    _, mag = eref.expect_ld(pk, B, GE)
    assert abs(e[0].real) > 1e-3 and abs(e[0].imag) <= eref.bound(65, 3, 4, mag[0])
    ed = eref.expect_f64(pk, B, RB[2][None])                    # d/dr
    assert abs(ed[0].imag) > 1e-3
    Ba, Ga = host.split_expect_accel(prob, chans)
    r = prob.quadrature()[0]
    assert np.array_equal(Ba, B) and Ga.shape == (1, 7, 65) and sym(Ga[0]) <= 64 * EPS
    assert np.array_equal(Ga, prob.operator_bands(1.0 / (r * r), [0]))
    assert np.array_equal(host.split_expect_accel(_stand_in(c, g, RB, zatom=2.0), chans)[1], prob.operator_bands(2.0 / (r * r), [0]))
    with pytest.raises(ValueError):
        host.split_expect_accel(_stand_in(c, g, RB, kind_pot=1), chans)
    soft = lambda rr: rr / (rr * rr + 1.0) ** 1.5
    G1 = host.split_expect_accel(_stand_in(c, g, RB, kind_pot=1), chans, dVdr=soft)[1]
    assert np.array_equal(G1, host.split_expect_accel(prob, chans, dVdr=soft(r))[1]) and not np.array_equal(G1, Ga)
    obs = rng.standard_normal((4, 2, 3 + 2 * 2 + 2 * 3))
    rows = host.split_expect_rows(obs, 3, 2)
    assert rows.shape == (4, 2, 3) and np.array_equal(rows.real, obs[..., 7::2]) and np.array_equal(rows.imag, obs[..., 8::2])
    assert host.split_expect_rows(obs[..., :7], 3, 2).shape == (4, 2, 0)
    with pytest.raises(ValueError):
        host.split_expect_rows(obs[..., :8], 3, 2)


def test_hhg_spectrum_of_a_cosine_peaks_at_its_frequency():
    """d(t) = cos(omega0 t) sampled every 0.1 over 200 periods' worth of rows: both kinds peak at the bin next to omega0 (omega^2
    does not move a Hann peak by a bin); the dipole kind is omega^4 times the plain spectrum; a second column is treated alike; the
    zero-frequency bin of the dipole kind is zero"""
    dt, nt, w0 = 0.1, 4096, 1.3
    t = dt * np.arange(nt)
    d = np.cos(w0 * t)
    om, S = host.hhg_spectrum(d, dt, kind="accel")
    assert om.shape == S.shape == (nt // 2 + 1,) and abs(om[1] - 2 * np.pi / (nt * dt)) < 1e-15
    assert abs(om[np.argmax(S)] - w0) <= om[1]
    om2, S2 = host.hhg_spectrum(d, dt)
    assert np.array_equal(om, om2) and abs(om[np.argmax(S2)] - w0) <= om[1] and S2[0] == 0.0
    assert np.allclose(S2, om ** 4 * S, rtol=1e-12, atol=0.0)
    _, S3 = host.hhg_spectrum(np.stack([d, 2.0 * d], axis=1), dt, window=None, kind="accel")
    assert S3.shape == (nt // 2 + 1, 2) and np.allclose(S3[:, 1], 4.0 * S3[:, 0], rtol=1e-12)
    # Parseval with no window: sum |x~|^2 d omega / pi = integral of x^2 (one-sided, interior bins doubled)
    assert abs((2.0 * S3[1:-1, 0].sum() + S3[0, 0] + S3[-1, 0]) * om[1] / (2.0 * np.pi) - dt * np.sum(d * d)) < 1e-9 * nt * dt
    with pytest.raises(ValueError):
        host.hhg_spectrum(d, dt, window="blackman")
    with pytest.raises(ValueError):
        host.hhg_spectrum(d, dt, kind="velocity")


def test_dipole_of_the_restatement_is_second_order():
    """The order check of test_gpu_spline_expect.test_dipole_rows_are_second_order on the dense restatement: n65_k4's grid, l = 0, 1
    from 1s through tdse_spline_ref's pulse with f = -F; <cos theta r> of the packets at t = 0, 0.1, .. 12 at dt = 0.1 and 0.05
    against the Richardson extrapolate (4 d(h/2) - d(h)) / 3 of the same restatement at h = 0.0125 -- fourth order, its distance from
    d(h/2) is 1e-7 --: the largest deviations fall in the ratio 3.9 .. 4.1.  Measured: 2.611e-05 and 6.528e-06, ratio 4.0002 (the
    l2 norms over the rows: 4.0004): the dipole error does not cross zero near its maximum, so the GPU test takes the largest
    deviation as the issue states it."""
    c, g, SB, HB, RB = _bands(65, 4)
    S, Gd = ref.upper_to_dense(SB), ref.full_to_dense(RB[0])
    V0 = scipy.linalg.eigh(ref.upper_to_dense(HB[0]), S)[1]
    chans = [(0, 0), (1, 0)]
    Q, lam = host.split_angular(chans)
    B = host.split_expect_dipole(_stand_in(c, g, RB), chans)[0][0]
    c0 = np.zeros((2, c.nfun), dtype=np.complex128)
    c0[0] = V0[:, 0]
    T = sref.PULSE["T"]

    def dipole(dt, every):
        ns = int(round(T / dt))
        F = -sref.pulse(host.spline_midpoints(0.0, dt, ns))
        _, traj, _ = pref.propagate(SB, HB, [0, 1], dt, c0, RB[0], Q, lam, F)
        return np.array([np.sum(np.conj(p) * ((B @ p) @ Gd.T)).real for p in np.concatenate([c0[None], traj])[::every]])

    fine, finer = dipole(0.0125, 8), dipole(0.00625, 16)
    zref = (4.0 * finer - fine) / 3.0
    errs = [float(np.max(np.abs(dipole(dt, every) - zref))) for dt, every in ((0.1, 1), (0.05, 2))]
    ratio = errs[0] / errs[1]
    print("dipole of the restatement: %.3e (dt 0.1), %.3e (dt 0.05), ratio %.4f; largest |<z>| %.4e" % (errs[0], errs[1], ratio, np.max(np.abs(zref))))
    assert np.max(np.abs(zref)) > 0.1 and np.max(np.abs(finer - zref)) < 0.05 * errs[1]
    assert 3.9 <= ratio <= 4.1, (errs, ratio)
