"""The three banded LU solvers -- the one-wave factorisation of csrc/resolvent.hip (single channel and chains), the workgroup LU of
csrc/resolvent_coupled_lu.h (the coupled resolvent and the time steps of csrc/tdse_spline.hip) and the blocked panel LU of
csrc/resolvent_wide.hip -- where the physical matrices of the other tests never take them: pivots at distance bw, rows of U that are
2 bw wide, pivots that are exactly zero.  The matrices are those of tests/pivot_designs.py, given to the calls through their public
arguments; test_resolvent_pivots_cpu.py proves on the CPU that they pivot and fill as designed and that a banded LU with a cut pivot
search or dropped fill misses the criterion used here on every one of (A) and (B).  Criterion, references and helpers are the
project's own: tests/resolvent_ref.py, tests/resolvent_coupled_ref.py, test_gpu_resolvent._input / _vectors / _same."""
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import pivot_designs as pd
import resolvent_chain_ref as chref
import resolvent_coupled_ref as cref
import test_gpu_resolvent as single        # its fixtures (_input), right-hand sides (_vectors) and bit comparison (_same)
import test_gpu_resolvent_coupled as coupled
import test_gpu_resolvent_wide as wide     # its problems (k16_n20 among them)
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
same = single._same
DT = 0.05


@functools.lru_cache(maxsize=None)
def _assembled(name):
    """(problem, SB, HB[0:2], the absorber's band, the bands of r and d/dr): assembled once per grid, bands only, never changed"""
    got = wide._assembled(name)
    for v in got[1:]:
        v.setflags(write=False)
    return got


def _call(prob, WB, entry, sy, B, P, mats=None):
    """the coupled call `entry` on the matrices `mats` (a slice; None: all) of a system, with the arrays pivot_designs.dense is given"""
    sel = slice(None) if mats is None else mats
    return getattr(prob, entry)(sy["l"], sy["z"][sel], B, couplings=sy["couplings"], G=sy["G"], a=sy["a"][sel],
                                W=None if sy["w"] is None else WB, w=None if sy["w"] is None else sy["w"][sel], P=P)


def _criterion(what, nch, dense, B, P, X, R, info):
    """The project's criterion on the matrices `dense` = [(M, Ml)] (channel-major, complex128 and clongdouble) of one call: X finite,
    info == 0, omega <= 8 max(omega_ref, eps) with omega_ref numpy.linalg.solve's in the documented ordering, R against P^T x within
    (N + 2) eps sum |P| |x|.  Returns the largest omega / max(omega_ref, eps)."""
    nrhs, nproj = B.shape[0], 0 if P is None else P.shape[0]
    N = dense[0][0].shape[0]
    Bc = B.reshape(nrhs, nch, -1)
    assert X.shape[:2] == (len(dense), nrhs) and np.all(np.isfinite(X.view(np.float64))), what
    assert np.all(info == 0), (what, info)
    assert (R is None) == (nproj == 0)
    worst = 0.0
    for m, (M, Ml) in enumerate(dense):
        Xref = cref.solve(M, Bc, nch)
        for r in range(nrhs):
            om, om_ref = cref.backward_error(Ml, X[m, r], B[r]), cref.backward_error(Ml, Xref[r], B[r])
            ratio = om / max(om_ref, EPS)
            worst = max(worst, ratio)
            print("%s m %d rhs %d: omega %.3e  omega_ref %.3e  ratio %.3g" % (what, m, r, om, om_ref, ratio))
            assert om <= 8.0 * max(om_ref, EPS), (what, m, r, om, om_ref)
            for q in range(nproj):
                xl, pl = X[m, r].astype(np.clongdouble).ravel(), P[q].astype(np.clongdouble).ravel()
                bound = (N + 2) * EPS * float(np.sum(np.abs(pl) * np.abs(xl)))
                assert abs(complex(np.sum(pl * xl)) - R[m, r, q]) <= bound, (what, m, r, q)
    return worst


def _coupled_case(entry, name, nch, kinds):
    """every system of a coupled case through `entry`, nrhs / nproj = (1, 0) and (3, 2); of (C) the regular matrix alone.  Returns
    the largest ratio per design."""
    prob, SB, HB, WB, _ = _assembled(name)
    n = prob.nfun
    assert nch * prob.k - 1 <= (63 if entry == "resolvent_coupled" else 255)
    worst = {}
    for sy in pd.coupled_systems(name, nch, SB, HB, WB, kinds):
        mats = slice(0, 1) if sy["tag"] == "C" else slice(None)
        dense = [(pd.dense(sy, SB, HB, WB, m), pd.dense(sy, SB, HB, WB, m, np.clongdouble)) for m in range(len(sy["z"]))[mats]]
        for nrhs, nproj in ((1, 0), (3, 2)):
            B, P = coupled._vectors(n, nch, nrhs, nproj, 7 + nrhs)
            X, R, info = _call(prob, WB, entry, sy, B, P, mats)
            ratio = _criterion("%s %s nch %d (%s)" % (entry, name, nch, sy["tag"]), nch, dense, B, P, X, R, info)
            worst[sy["tag"]] = max(worst.get(sy["tag"], 0.0), ratio)
    note("%s pivots %s nch %d (bw %d): max omega / max(omega_ref, eps) = %s"
         % (entry, name, nch, nch * prob.k - 1, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    return worst


# ---- the one-wave factorisation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pd.SINGLE_CASES)
def test_single_channel_far_pivots(name):
    """bspatom_resolvent on design (A), which enters through W: two matrices (t = 20 on l = 0, t = 2 on l = 1), every second group of
    k - 1 columns pivots at distance b = k - 1 and U's rows are 2 b wide; b = 3 (n65_k4), 8 (lin256), 9, the instance for b <= 15 with
    rows of its register window unused (k10_n65), 15, the limit of the one-wave window (k16_n40).  The criterion of
    test_gpu_resolvent's T1.  The single-channel call cannot cancel its base (W enters as -i W alone), so it gets no exactly singular
    case.  Measured on the MI355X, maximum of omega / max(omega_ref, eps): n65_k4 0.249, lin256 1.0, k10_n65 0.135, k16_n40 0.162."""
    prob, SB, HB, _, _ = _assembled(name)
    n = prob.nfun
    sy = pd.design_a_single(SB, HB)
    dense = [(pd.dense_single(sy, SB, HB, m), pd.dense_single(sy, SB, HB, m, np.clongdouble)) for m in range(2)]
    worst = 0.0
    for nrhs, nproj in ((1, 0), (3, 2)):
        B, P = single._vectors(n, nrhs, nproj, 7 + nrhs)
        X, R, info = prob.resolvent(sy["l"], sy["z"], B, W=sy["W"], w=sy["w"], P=P)
        worst = max(worst, _criterion("resolvent %s (A)" % name, 1, dense, B, P, X, R, info))
    note("resolvent pivots %s (b %d): max omega / max(omega_ref, eps) = %.3g" % (name, prob.k - 1, worst))


def test_chain_on_far_pivot_matrices():
    """C4 and C5 bit for bit where every stage pivots at distance 15: one chain of two stages on the two (A) matrices of k16_n40, the
    band of r in between, nrhs = 2, nproj = 2.  Each stage's R and info and the last X equal bspatom_resolvent with nmat = 1 given
    A x_0 formed by resolvent_chain_ref.band_combine_apply; the two matrices as two chains of one stage equal bspatom_resolvent."""
    prob, SB, HB, _, G = _assembled("k16_n40")
    n = prob.nfun
    sy = pd.design_a_single(SB, HB)
    l, z, w, W, GB = sy["l"], sy["z"], sy["w"], sy["W"], G[:1]
    B, P = single._vectors(n, 2, 2, 9)
    X, R, info = prob.resolvent_chain(l, z, B, G=GB, W=W, w=w, P=P)
    assert X.shape == (1, 2, n) and R.shape == (1, 2, 2, 2) and np.all(info == 0) and np.max(np.abs(X)) > 0
    y = B
    for s in range(2):
        if s:
            y = chref.band_combine_apply(GB, [1.0], xs[0])
        xs, rs, infs = prob.resolvent(l[s], z[s], y, W=W, w=w[s], P=P)
        assert same(rs[0], R[0, s]) and infs[0] == info[0, s], s
    assert same(xs[0], X[0])
    col = lambda v: np.asarray(v).reshape(2, 1)
    X1, R1, info1 = prob.resolvent_chain(col(l), col(z), B, W=W, w=col(w), P=P)
    Xr, Rr, infor = prob.resolvent(l, z, B, W=W, w=w, P=P)
    assert same(X1, Xr) and same(R1[:, 0], Rr) and np.array_equal(info1[:, 0], infor)


# ---- the workgroup LU --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch", pd.NARROW_CASES, ids=["%s-nch%d" % c for c in pd.NARROW_CASES])
def test_coupled_far_pivots(name, nch):
    """bspatom_resolvent_coupled on the designs (A) (t = 20 and t = 2), (B) and (C, the regular matrix), the criterion of
    test_gpu_resolvent_coupled's T1: N < 2 bw + 1 (tiny8, nch 2), bw = 11 (n65_k4, nch 3), bw = 62 (lin256, nch 7) and bw = 63, both
    register sets of rc_solve full (k16_n40, nch 4).  (A): rc_factor swaps window rows up to the last, rs_forward reads lane p - j = bw.
    Measured on the MI355X, maximum of omega / max(omega_ref, eps) per case and design: tiny8 nch 2: A 0.735, B 0.537, C 0.204;
    n65_k4 nch 3: A 0.268, B 0.233, C 0.27; lin256 nch 7: A 1.55, B 0.328, C 0.399; k16_n40 nch 4: A 0.176, B 0.7, C 0.339."""
    _coupled_case("resolvent_coupled", name, nch, "ABC")


# ---- the blocked panel LU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch", pd.WIDE_CASES, ids=["%s-nch%d" % c for c in pd.WIDE_CASES])
def test_wide_far_pivots(name, nch):
    """bspatom_resolvent_coupled_wide on (A) and (B), and (C, regular) on the two smaller cases, the criterion of
    test_gpu_resolvent_wide's T1: bw = 67, pivots cross into wave 1 and across four panels (n65_k4, nch 17); the window never fills
    (k16_n20, nch 5, t = 6 for the condition number); bw = 143, 287 columns, no multiple of 16 (k16_n40, nch 9); bw = 255: pivots at
    distance 192 .. 255 land in wave 3 and U12 runs into the second chunk of 256 columns (k16_n40, nch 16; (B) with two bands).
    Measured on the MI355X, maximum of omega / max(omega_ref, eps) per case and design: n65_k4 nch 17: A 0.26, B 0.278, C 0.603;
    k16_n20 nch 5: A 0.233, B 0.406, C 0.306; k16_n40 nch 9: A 0.144, B 0.843; k16_n40 nch 16: A 0.164, B 0.756."""
    _coupled_case("resolvent_coupled_wide", name, nch, "ABC" if (name, nch) in pd.WIDE_C else "AB")


def test_narrow_against_wide_on_far_pivot_matrices():
    """The same designed matrices at bw = 63 (k16_n40, nch 4: (A) twice, (B)) by both coupled calls: each meets the criterion; their
    difference is printed in units of eps max |x|, not asserted -- include/bspatom.h promises no equality between the two kernels.
    Measured on the MI355X: 4.6e3 on (A), 1.8e3 on (B) (condition numbers 4e5 and 6e3); every omega / max(omega_ref, eps)
    of either call is below 1."""
    prob, SB, HB, WB, _ = _assembled("k16_n40")
    n, nch = prob.nfun, 4
    B, P = coupled._vectors(n, nch, 3, 2, 11)
    for sy in pd.coupled_systems("k16_n40", nch, SB, HB, WB, "AB"):
        dense = [(pd.dense(sy, SB, HB, WB, m), pd.dense(sy, SB, HB, WB, m, np.clongdouble)) for m in range(len(sy["z"]))]
        got = {}
        for entry in ("resolvent_coupled", "resolvent_coupled_wide"):
            X, R, info = _call(prob, WB, entry, sy, B, P)
            _criterion("%s against the other (%s)" % (entry, sy["tag"]), nch, dense, B, P, X, R, info)
            got[entry] = X
        Xn, Xw = got["resolvent_coupled"], got["resolvent_coupled_wide"]
        diff = max(float(np.max(np.abs(Xn[m, r] - Xw[m, r])) / (EPS * np.max(np.abs(Xn[m, r])))) for m in range(Xn.shape[0]) for r in range(3))
        note("narrow against wide, k16_n40 nch 4 (%s): max |x_narrow - x_wide| = %.3g eps max |x|" % (sy["tag"], diff))


# ---- pivots that are exactly zero --------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,nch", [("resolvent_coupled", 3), ("resolvent_coupled_wide", 17)], ids=["narrow-nch3", "wide-nch17"])
def test_zero_pivots_are_replaced_and_counted(entry, nch):
    """Design (C) on n65_k4, one batch of three: the regular integer matrix, the same with one column zero, the same with two separated
    columns zero (the coefficients of the batch do it; the bands are shared).  A zero column stays exactly zero under any elimination,
    so info is [0, 1, 2] exactly -- the replacement path (rs_pivot_recip, the count) with a known answer --, every X is finite, and
    the regular matrix's X and R have the bits of solving it alone (K2 next to singular neighbours).  The single-channel call cannot
    cancel its base, so it has no such case."""
    prob, SB, HB, WB, _ = _assembled("n65_k4")
    n = prob.nfun
    sy = pd.design_c(SB, HB, nch)
    B, P = coupled._vectors(n, nch, 3, 2, 13)
    X, R, info = _call(prob, WB, entry, sy, B, P)
    print("%s nch %d: info %s  max |x| %s" % (entry, nch, info, np.max(np.abs(X), axis=(1, 2, 3))))
    assert np.array_equal(info, [0, 1, 2]), info
    assert np.all(np.isfinite(X.view(np.float64))) and np.all(np.isfinite(R.view(np.float64)))
    X0, R0, info0 = _call(prob, WB, entry, sy, B, P, slice(0, 1))
    assert info0[0] == 0 and same(X0[0], X[0]) and same(R0[0], R[0])


# ---- K3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,nch", [("resolvent_coupled", 4), ("resolvent_coupled_wide", 9)], ids=["narrow-bw63", "wide-bw143"])
def test_real_far_pivot_problem_stays_real(entry, nch):
    """K3 where the rows travel: design (A) on k16_n40 with real strengths (t = 20 and 2), real z (0.3 and -1.0, Im z = 0: no eraser),
    no absorber, real B and P: every imaginary part of X and R is +-0.0, on the workgroup LU at bw = 63 and on the panel LU at
    bw = 143."""
    prob, SB, HB, WB, _ = _assembled("k16_n40")
    sy = pd.design_a(SB, HB, None, nch, phase=1.0, mats=((0.3, -1), (-1.0, -1)), y=0.0)
    assert np.all(sy["z"].imag == 0.0) and np.all(sy["a"].imag == 0.0)
    B = np.random.default_rng(3).standard_normal((2, nch, prob.nfun))
    X, R, info = getattr(prob, entry)(sy["l"], sy["z"], B, couplings=sy["couplings"], G=sy["G"], a=sy["a"], P=B)
    assert np.all(info == 0) and np.max(np.abs(X.real)) > 0
    assert np.all(X.imag == 0.0) and np.all(R.imag == 0.0)


# ---- the time steps ----------------------------------------------------------------------------------------------------
def test_time_steps_on_a_far_pivot_matrix():
    """S3 bit for bit where the step's matrix pivots at distance bw: four steps of bspatom_tdse_spline on n65_k4 with three channels,
    the static couplings design (A) at t = 2 on the step's own base (z = 2i / dt), two packets (one real).  The replay of
    test_gpu_tdse_spline.test_step_is_band_apply_coupled_solve_update with these couplings -- host.band_apply on the overlap's band,
    Problem.resolvent_coupled at z = 2i / dt, two NumPy operations -- reproduces every snapshot, c and info."""
    prob, SB, HB, WB, _ = _assembled("n65_k4")
    n, nch, nsteps = prob.nfun, 3, 4
    sy = pd.design_a(SB, HB, None, nch, strengths=(pd.T_WEAK,), mats=((0.0, -1),), y=2.0 / DT)
    l, cp, G = sy["l"], sy["couplings"], sy["G"]
    coef = np.ascontiguousarray(np.broadcast_to(sy["a"][0], (nsteps,) + sy["a"][0].shape))
    rng = np.random.default_rng(103)
    c0 = (rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real
    cend, info, snaps = prob.tdse_spline(l, c0, DT, nsteps, couplings=cp, G=G, coef=coef, snap_every=1)
    assert np.all(info == 0) and np.all(np.isfinite(cend.view(np.float64))) and np.max(np.abs(cend - c0)) > 1e-3
    SBf = host.band_symmetric(SB)
    g, z = 4.0 / DT, complex(0.0, 2.0 / DT)
    c = np.array(c0)
    count = np.zeros(2, dtype=np.int64)
    for step in range(nsteps):
        for q in range(2):
            b = host.band_apply(SBf, c[q].real) + 1j * host.band_apply(SBf, c[q].imag)
            X, _, inf = prob.resolvent_coupled(l, z, b, couplings=cp, G=G, a=coef[step])
            x = X[0, 0]
            c[q] = (g * x.imag - c[q].real) + 1j * (-(g * x.real) - c[q].imag)
            count[q] += inf[0]
        assert same(c, snaps[step]), step
    assert same(c, cend) and np.array_equal(count, info)
