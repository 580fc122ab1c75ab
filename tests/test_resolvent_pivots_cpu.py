"""The designed matrices of tests/pivot_designs.py proved on the CPU, before any kernel sees them: on LAPACK's factorisation of the
interleaved dense matrix alone they pivot as far, fill U as wide and are as regular (or as exactly singular) as designed; the physical
matrices of test_gpu_resolvent_coupled's T1 do none of this -- which is why test_gpu_resolvent_pivots.py exists; and a banded LU that
is wrong where those are blind (tests/band_lu_ref.py: a pivot search cut to bw / 2, U's fill dropped beyond 1.25 bw) misses the GPU
tests' own criterion on every matrix of the designs (A) and (B), and meets it on T1.  Bands from the oracle on the GPU cases' grids.
No GPU."""
import functools
import numpy as np
import pytest

import oracle as orc
import band_lu_ref as blu
import pivot_designs as pd
import resolvent_ref as ref
import resolvent_coupled_ref as cref

EPS = np.finfo(np.float64).eps
CASES = [("single", name, 1) for name in pd.SINGLE_CASES] + [("narrow", name, nch) for name, nch in pd.NARROW_CASES] \
    + [("wide", name, nch) for name, nch in pd.WIDE_CASES]
IDS = ["%s-%s-nch%d" % c for c in CASES]
MUTANTS = lambda bw: (dict(max_pivot_distance=bw // 2), dict(fill_width=bw + bw // 4))


@functools.lru_cache(maxsize=None)
def _bands(name):
    """(SB, HB[0:2], the absorber's band of the GPU tests, the bands of r and d/dr) of a grid, from the oracle"""
    kw = pd.GRIDS.get(name) or dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)   # "hydrogen"
    c = orc.make_cfg(**kw)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 2)
    r = ref.quadrature(rt, xg, wg)[0]
    WB = ref.operator_band(rt, c.k, xg, wg, lambda q: ref.cap_profile(q, 0.5 * r[-1], 1e-2))
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    return SB, HB, WB, np.stack([RB[0], RB[2]])


@functools.lru_cache(maxsize=1)
def _designed(group, name, nch):
    """[(label, design, the interleaved dense matrix)] of a GPU case, every matrix of every system"""
    SB, HB, WB, _ = _bands(name)
    k, n = SB.shape
    out = []
    if group == "single":
        sy = pd.design_a_single(SB, HB)
        return [("A %s" % sy["what"][m], "A", pd.dense_single(sy, SB, HB, m)) for m in range(2)]
    kinds = "ABC" if group == "narrow" or (name, nch) in pd.WIDE_C else "AB"
    for sy in pd.coupled_systems(name, nch, SB, HB, WB, kinds):
        for m in range(len(sy["z"])):
            M = pd.dense(sy, SB, HB, WB, m)
            assert cref.half_width(M, nch) <= nch * k - 1
            out.append(("%s %s" % (sy["tag"], sy["what"][m]), sy["tag"], pd.interleaved(M, nch)))
    return out


def _condition(Mi):
    """the 2-norm condition number: by SVD up to order 400, above it the bound sqrt(kappa_1 kappa_inf) from the inverse"""
    if Mi.shape[0] <= 400:
        return float(np.linalg.cond(Mi))
    inv = np.linalg.inv(Mi)
    return float(np.sqrt(np.linalg.norm(Mi, 1) * np.linalg.norm(inv, 1) * np.linalg.norm(Mi, np.inf) * np.linalg.norm(inv, np.inf)))


def _rhs(N):
    rng = np.random.default_rng(5)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


def _meets(Mi, bw, *mutants):
    """[(omega / max(omega_ref, eps), whether the GPU tests' criterion omega <= 8 max(omega_ref, eps) is met)] for band_lu_ref.solve
    unmutated and then with each dict of knobs given; omega in clongdouble, omega_ref numpy.linalg.solve's on the same matrix and
    right-hand side.  A solution that is not finite does not meet it."""
    b = _rhs(Mi.shape[0])
    Ml = Mi.astype(np.clongdouble)
    om_ref = cref.backward_error(Ml, np.linalg.solve(Mi, b), b)
    out = []
    for knobs in ({},) + mutants:
        with np.errstate(all="ignore"):
            x = blu.solve(Mi, b, bw, **knobs)
            om = cref.backward_error(Ml, x, b) if np.all(np.isfinite(x.view(np.float64))) else np.inf
        out.append((om / max(om_ref, EPS), bool(om <= 8.0 * max(om_ref, EPS))))
    return out


@pytest.mark.parametrize("check", ["conditions", "mutants"])      # the inner one: a case's matrices are built once
@pytest.mark.parametrize("group,name,nch", CASES, ids=IDS)
def test_designed_matrices(group, name, nch, check):
    """For every designed matrix of the GPU case.  conditions, on LAPACK's zgetrf of the interleaved matrix: the half-width is
    <= nch k - 1; (A): the largest pivot distance is bw exactly and at least 0.35 of the columns pivot at distance >= bw - 2 (nch-1)
    -- on k16_n20, whose 20 functions hold no complete group of 30, no more than (n - (k-1)) / n = 0.25 of the columns HAVE a row
    that far, and exactly those must pivot there --; (A), (B): U's widest row is >= 2 bw - 2 (nch-1) - 10, or N - 1 where the matrix
    is no wider (k16_n20); the condition number is <= 1e7; (C): 0, 1 and 2 exact zeros on U's diagonal.  mutants: band_lu_ref
    unmutated meets the GPU criterion on every regular matrix; cut to max_pivot_distance = bw // 2, or to fill_width = bw + bw // 4,
    it misses it on every matrix of (A) and (B)."""
    SB = _bands(name)[0]
    k, n = SB.shape
    bw, N = nch * k - 1, nch * n
    for label, design, Mi in _designed(group, name, nch):
        what = "%s %s nch %d %s" % (group, name, nch, label)
        singular = design == "C" and "column" in label
        if check == "conditions":
            far, dist, widest, zeros = blu.lapack_profile(Mi)
            frac = float(np.mean(dist >= bw - 2 * (nch - 1)))
            cond = float("inf") if singular else _condition(Mi)
            print("%s: N %d bw %d  largest pivot distance %d  far columns %.3f  widest row of U %d (2 bw = %d)  condition %.2e  zeros %d"
                  % (what, N, bw, far, frac, widest, 2 * bw, cond, zeros))
            if design == "A":
                assert far == bw, what
                if n >= 2 * (k - 1):
                    assert frac >= 0.35, what
                else:
                    assert frac == (n - (k - 1)) / n, what
            if design in "AB":
                assert widest >= min(2 * bw - 2 * (nch - 1) - 10, N - 1), what
            if design == "C":
                assert zeros == ["regular", "one column", "two columns"].index(label[2:]), what
            if not singular:
                assert cond <= 1e7, what
        elif not singular:
            res = _meets(Mi, bw, *(MUTANTS(bw) if design in "AB" else ()))
            plain, ok = res[0]
            assert ok, (what, plain)
            if design in "AB":
                (rp, okp), (rf, okf) = res[1:]
                print("%s: omega / max(omega_ref, eps) unmutated %.3g  pivot search cut %.3g  fill dropped %.3g" % (what, plain, rp, rf))
                assert not okp and not okf, (what, rp, rf)


# ---- the matrices of test_gpu_resolvent_coupled's T1, restated: its topology, coefficients and (z, absorber, strength) ------------
T1_MATS = [(0.3, -1, 0.0), (0.3, -1, 1e-2), (0.3, -1, 1.0), (0.3 + 0.05j, -1, 1.0), (0.3 - 0.05j, 0, 1e-2), (0.3 + 0.05j, 0, 0.0),
           (0.3, 0, 1.0), (0.3 - 0.05j, -1, 1e-2)]


def _t1_matrix(nch, zb, wm, s):
    SB, HB, WB, G = _bands("hydrogen")
    cp = [(0, 0, 0)] + [e for c in range(nch - 1) for e in ((c, c + 1, 0), (c + 1, c, 1))]
    a = np.zeros((2 * nch - 1, 2), dtype=np.complex128)
    a[0] = (0.5 * s, 0.05 * s)
    a[1:, 0] = s
    if nch > 1:
        a[1, 0], a[2, 0] = s * (1 + 0.3j), s * (1 - 0.3j)
    else:
        a[0, 0] = 0.5 * s * (1 + 0.3j)
    M = cref.dense_matrix(SB, HB, [c % 2 for c in range(nch)], [zb + 0.01 * c for c in range(nch)], cp, G, a, WB[None], [wm] * nch)
    return pd.interleaved(M, nch)


@pytest.mark.parametrize("nch", [1, 2, 4, 7])
def test_physical_matrices_stay_near_the_diagonal(nch):
    """Why this file exists: the eight T1 matrices on test_resolvent_cpu's hydrogen grid (k = 9, nfun = 96) pivot within bw / 2 and
    fill U within 1.3 bw (measured: distances 3, 6, 12, 21 and widths 10, 21, 41, 71 at bw 8, 17, 35, 62), so both mutants of
    band_lu_ref factor them exactly as the unmutated LU does and meet the criterion: a kernel with those faults passes T1."""
    bw = nch * 9 - 1
    far, widest = 0, 0
    for zb, wm, s in T1_MATS:
        Mi = _t1_matrix(nch, zb, wm, s)
        f, _, w_, zeros = blu.lapack_profile(Mi)
        far, widest = max(far, f), max(widest, w_)
        assert zeros == 0
        for q, (ratio, ok) in enumerate(_meets(Mi, bw, *MUTANTS(bw))):
            assert ok, (nch, zb, wm, s, q, ratio)
    print("T1 nch %d bw %d: largest pivot distance %d  widest row of U %d" % (nch, bw, far, widest))
    assert far <= bw / 2 and widest <= 1.3 * bw


def test_band_lu_ref_is_lu_with_partial_pivoting():
    """band_lu_ref against LAPACK on a designed matrix (n65_k4, nch = 3, (B)): the same pivot rows, the same widest row, a solution as
    good; and the knobs do what they say on a matrix where they bite"""
    SB, HB, WB, _ = _bands("n65_k4")
    sy = pd.design_b(SB, HB, WB, 3)
    Mi = pd.interleaved(pd.dense(sy, SB, HB, WB, 0), 3)
    bw = 3 * 4 - 1
    far, dist, widest, _ = blu.lapack_profile(Mi)
    LU, piv, w_ = blu.factor(Mi, bw)
    assert np.array_equal(piv - np.arange(len(piv)), dist) and w_ == widest
    _, piv_cut, _ = blu.factor(Mi, bw, max_pivot_distance=bw // 2)
    assert np.max(piv_cut - np.arange(len(piv))) <= bw // 2 < far
    _, _, w_cut = blu.factor(Mi, bw, fill_width=bw + bw // 4)
    assert w_cut <= bw + bw // 4 < widest
