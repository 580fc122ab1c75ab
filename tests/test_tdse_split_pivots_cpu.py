"""The split-step TDSE's own banded LU (csrc/tdse_split.hip: sp_factor, sp_solve) and what its tests can see, settled on the CPU before
any kernel runs: the physical matrices of test_gpu_tdse_split.py pivot next to the diagonal and fill U barely past the band, so a
kernel whose pivot search stops at b / 2 or which drops U's fill beyond 1.25 b passes them; the designed matrices of
tests/pivot_designs.py (split_system) pivot at distance b, fill U's rows to 2 b and are as regular, or as exactly singular, as
designed; and on every designed case the restatement tests/tdse_split_ref.py solving with tests/band_lu_ref.py meets the GPU tests'
criterion unmutated and misses it with either fault.  Bands from the oracle on the GPU cases' grids.  No GPU."""
import ast
import functools
import os
import numpy as np
import pytest

import oracle as orc
import band_lu_ref as blu
import pivot_designs as pd
import resolvent_ref as ref
import tdse_split_ref as pref

EPS = np.finfo(np.float64).eps
MUTANTS = lambda b: (dict(max_pivot_distance=b // 2), dict(fill_width=b + b // 4))
PHYS_DT, PHYS_NSCAN = 0.05, 5                                  # test_gpu_tdse_split's DT and NSCAN


def _gpu_shapes():
    """test_gpu_tdse_split.SHAPES, read from the file's text: importing it would import the GPU runtime"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_tdse_split.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "SHAPES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("SHAPES not found")


SHAPES = _gpu_shapes()


@functools.lru_cache(maxsize=None)
def _bands(name):
    """(SB, HB[0:2], the absorber's band of the GPU tests, the band of r) of a grid, from the oracle"""
    c = orc.make_cfg(**pd.GRIDS[name])
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 2)
    r = ref.quadrature(rt, xg, wg)[0]
    WB = ref.operator_band(rt, c.k, xg, wg, lambda q: ref.cap_profile(q, 0.5 * r[-1], 1e-2))
    return SB, HB, WB, orc.dipole_bands(c, rt, aind, xg, wg)[0]


def _args(SB, HB, sy, q):
    return SB, HB, sy["l"], sy["dt"], sy["c0"][q], sy["G"], sy["Q"], sy["lam"], sy["f"][:, q], sy["W"], sy["w"]


def _references(SB, HB, sy, scans=None):
    """{scan: (the dense restatement's final packet, delta_ref)}: test_gpu_tdse_split._reference"""
    return {q: pref.delta_ref(*_args(SB, HB, sy, q))[::2] for q in (range(sy["c0"].shape[0]) if scans is None else scans)}


def _accuracy(SB, HB, sy, refs, knobs=None):
    """test_gpu_tdse_split._accuracy with the restatement solving by band_lu_ref in the kernel's place: the largest, over the scans
    of refs, of ||c - c_ref||_S / (8 max(delta_ref, eps nsteps) max(1, ||c0||_S)).  A result that is not finite counts as infinity."""
    S = ref.upper_to_dense(SB)
    worst = 0.0
    for q, (cref_, delta) in refs.items():
        c, _, _ = pref.propagate(*_args(SB, HB, sy, q), how="lu", knobs=knobs)
        scale = max(1.0, pref.s_norm(S, sy["c0"][q]))
        bound = 8.0 * max(delta * scale, EPS * sy["nsteps"] * scale)
        err = pref.s_norm(S, c - cref_) if np.all(np.isfinite(c.view(np.float64))) else np.inf
        worst = max(worst, err / bound)
    return worst


# ---- 1: the physical cases are blind ---------------------------------------------------------------------------------------------
def _angular(nch, rng):
    """test_gpu_tdse_split._angular"""
    if nch == 1:
        return np.ones((1, 1)), np.array([0.7])
    off = rng.uniform(0.3, 0.7, nch - 1)
    A = np.diag(rng.uniform(-0.2, 0.2, nch)) + np.diag(off, 1) + np.diag(off, -1)
    lam, Q = np.linalg.eigh(A)
    return np.ascontiguousarray(Q), lam


def _physical(name, nch, nsteps, absorb):
    """test_gpu_tdse_split._case restated: the same seeded angular matrix, fields and packets, the oracle's bands"""
    SB, HB, WB, RB = _bands(name)
    n = SB.shape[1]
    rng = np.random.default_rng(200 + nch)
    Q, lam = _angular(nch, rng)
    f = rng.uniform(0.2, 1.0, (nsteps, PHYS_NSCAN)).astype(np.complex128)
    c0 = (rng.standard_normal((PHYS_NSCAN, nch, n)) + 1j * rng.standard_normal((PHYS_NSCAN, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real
    return dict(l=[c % 2 for c in range(nch)], w=([0] + [-1] * (nch - 1)) if absorb else None, W=WB[None] if absorb else None,
                G=np.ascontiguousarray(RB), Q=Q, lam=lam, f=f, c0=c0, dt=PHYS_DT, nsteps=nsteps)


@pytest.mark.parametrize("name,nch,nsteps", SHAPES, ids=["%s-nch%d" % s[:2] for s in SHAPES])
def test_physical_cases_are_blind(name, nch, nsteps):
    """Why test_gpu_tdse_split_pivots.py exists.  On every case of test_gpu_tdse_split.SHAPES, without and with the absorber: LAPACK's
    zgetrf of every atomic matrix and of every field matrix (every step, scan and eigenchannel) pivots within b / 2 and fills U within
    1.3 b; and the restatement solving with band_lu_ref under either fault meets that file's accuracy criterion (scans 0 and 1: the
    real packet and a complex one) -- a kernel with those faults passes there.  Measured, largest pivot distance / widest row of U:
    tiny8 (b 4) 1 / 5, n65_k4 (b 3) 0 / 3, lin256 (b 8) 2 / 10, k16_n40 (b 15) 3 / 18, k10_n65 (b 9) 2 / 11."""
    SB, HB, _, _ = _bands(name)
    b = SB.shape[0] - 1
    for absorb in (False, True):
        sy = _physical(name, nch, nsteps, absorb)
        mats = pref.atomic_matrices(SB, HB, sy["l"], sy["dt"], sy["W"], sy["w"])
        mats += [pd.split_field_matrix(sy, SB, q, j, s) for s in range(nsteps) for q in range(PHYS_NSCAN) for j in range(nch)]
        far, widest = 0, 0
        for M in mats:
            f_, _, w_, zeros = blu.lapack_profile(M)
            far, widest = max(far, f_), max(widest, w_)
            assert zeros == 0
        print("%s nch %d %s: b %d  largest pivot distance %d  widest row of U %d" % (name, nch, "cap" if absorb else "nocap", b, far, widest))
        assert far <= b / 2 and widest <= 1.3 * b, (name, absorb, far, widest)
        refs = _references(SB, HB, sy, scans=(0, 1))
        for knobs in ({},) + MUTANTS(b):
            ratio = _accuracy(SB, HB, sy, refs, knobs)
            print("    %s: err / bound %.3g" % (knobs or "unmutated", ratio))
            assert ratio <= 1.0, (name, absorb, knobs, ratio)


# ---- 2: the designs are as designed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pd.SPLIT_GRIDS)
def test_designs_are_as_designed(name):
    """On LAPACK's zgetrf: the two designed atomic matrices (l = 0 at t = 20, l = 1 at t = 2) and the field matrix S + G of the
    eigenchannel lam = +1 under f = -2i / dt, and of lam = -1 under f = +2i / dt (the same matrix), have the largest pivot distance b
    exactly, a row of U at least min(2 b, n - 1) wide and a condition number <= 1e7.  Where the singular design has a GPU case: S + G
    (the factor 1) has exactly two zeros on U's diagonal, S - G and S + G / 2 none, with column j2 alone one zero; and no other pivot
    of band_lu_ref.factor is below 1e3 eps max |diag|, so the kernel's threshold eps max |diag| counts exactly the zero columns."""
    SB, HB, _, RB = _bands(name)
    k, n = SB.shape
    b = k - 1
    sy = pd.split_system("both", SB, HB, RB)
    lam = list(sy["lam"])
    designed = [("atomic l=%d" % c, M) for c, M in enumerate(pref.atomic_matrices(SB, HB, sy["l"], sy["dt"], sy["W"], sy["w"])[:2])]
    designed += [("field f=-2i/dt lam=+1", pd.split_field_matrix(sy, SB, 0, lam.index(1.0))),
                 ("field f=+2i/dt lam=-1", pd.split_field_matrix(sy, SB, 1, lam.index(-1.0)))]
    assert np.array_equal(designed[2][1], designed[3][1])
    assert np.array_equal(designed[2][1], ref.upper_to_dense(SB) + ref.full_to_dense(sy["G"]))     # the factor is 1 exactly
    for what, M in designed:
        far, _, widest, zeros = blu.lapack_profile(M)
        cond = float(np.linalg.cond(M))
        print("%s %s: b %d  largest pivot distance %d  widest row of U %d (2 b = %d)  condition %.2e" % (name, what, b, far, widest, 2 * b, cond))
        assert far == b and widest >= min(2 * b, n - 1) and zeros == 0 and cond <= 1e7, (name, what, far, widest, cond)
    if name not in pd.SPLIT_ZERO_GRIDS:
        return
    S = ref.upper_to_dense(SB)
    for variant, nzero in (("zeros", 2), ("zero", 1)):
        sz = pd.split_system(variant, SB, HB, RB)
        Gd = ref.full_to_dense(sz["G"])
        mats = [(pd.split_field_matrix(sz, SB, q, j), factor) for q, j, factor in ((0, 2, 1.0), (0, 0, -1.0), (0, 1, 0.5), (1, 0, 1.0), (1, 2, -1.0))]
        for M, factor in mats:
            assert np.array_equal(M, S + factor * Gd)
        # regular besides: the real field of scan 2 (S + i 2^-13 lam G) and the call's atomic matrices, whose count joins info
        mats += [(pd.split_field_matrix(sz, SB, 2, j), None) for j in range(3)]
        mats += [(M, None) for M in pref.atomic_matrices(SB, HB, sz["l"], sz["dt"])]
        for M, factor in mats:
            want = nzero if factor == 1.0 else 0
            assert blu.lapack_profile(M)[3] == want, (name, variant, factor)
            with np.errstate(all="ignore"):
                LU, _, _ = blu.factor(M, b)
            piv = np.abs(np.diag(LU).real) + np.abs(np.diag(LU).imag)
            dmax = float(np.max(np.abs(np.diag(M).real) + np.abs(np.diag(M).imag)))
            assert np.all(np.isfinite(LU.view(np.float64))) and int(np.sum(piv == 0.0)) == want
            assert np.min(piv[piv != 0.0]) >= 1e3 * EPS * dmax, (name, variant, factor, np.min(piv[piv != 0.0]), dmax)


# ---- 3: the mutants would be noticed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", pd.SPLIT_VARIANTS)
@pytest.mark.parametrize("name", pd.SPLIT_GRIDS)
def test_mutants_miss_the_gpu_criterion(name, variant):
    """What keeps test_gpu_tdse_split_pivots.test_accuracy_on_designed_matrices honest: on every designed case the restatement with
    band_lu_ref unmutated meets its criterion (the largest err / bound over the three scans is <= 1), and with max_pivot_distance =
    b // 2 or with fill_width = b + b // 4 on every solve it misses it (> 1 on at least one scan, which fails the GPU test; not finite
    counts as missed).  Measured, the largest err / bound unmutated, fill dropped, search cut (inf: not finite), atomic | field | both:
    tiny8    0.18, 8.4e12, 2.5e3 | 0.15, 9.8e10, inf | 0.29, 1.2e13, inf
    n65_k4   0.17, 1.3e14, 265 | 0.14, 9.2e11, inf | 0.26, 1.4e14, inf
    lin256   0.13, 2.8e13, 83 | 0.13, 3.8e10, inf | 0.13, 3.8e13, inf
    k10_n65  0.36, 1.6e13, 580 | 0.17, 1.6e10, inf | 0.43, 1.7e13, inf
    k16_n40  0.16, 2.3e11, 47 | 0.12, 6.7e8, inf | 0.13, 1.7e11, inf
    Both faults miss the bound by at least 47 times on every case."""
    SB, HB, _, RB = _bands(name)
    b = SB.shape[0] - 1
    sy = pd.split_system(variant, SB, HB, RB)
    refs = _references(SB, HB, sy)
    plain = _accuracy(SB, HB, sy, refs)
    cut, drop = (_accuracy(SB, HB, sy, refs, knobs) for knobs in MUTANTS(b))
    print("%s %s: err / bound unmutated %.3g  fill dropped %.3g  pivot search cut %.3g" % (name, variant, plain, drop, cut))
    assert plain <= 1.0, (name, variant, plain)
    assert cut > 1.0 and drop > 1.0, (name, variant, cut, drop)
