"""bsp_dsygv_ (csrc/dsygv.hip) on synthetic pencils with prescribed spectra (tests/pencils.py; tests/test_pencils_cpu.py proves them
fair inputs): the eigenvector half of the pipeline -- inverse iteration, the cluster rule, the blocked S-orthonormalisation, the
512-vector chunks -- and the calling convention of the symbol, where the reference's own radial pencils never go.

The contract asserted for every jobz = 'V' call (`contract`):
  info = 0; w ascending; w of jobz = 'N' equal bit for bit; a second call returns the same bits of w and Z; U^T U = S to 1e-13;
  eigenvalues    |w - truth| <= 1e-13 |lambda|_max, truth = 113-bit bisection on the rounded pencil (all indices for n <= 200,
                 else 64 that hold both ends of every cluster);
  eigenvectors   orth  = max|Z^T S Z - I|                    <= max(4 n eps,  16 x LAPACK's on the same pencil)
                 resid = max|H Z - S Z w| / (|w|max |S|max)   <= max(32 n eps, 16 x LAPACK's)
                 (the standing bars 1e-12 / 1e-11 at n = 2048, restated per n);
  isolated       for every eigenvalue that is a cluster of one under the rule: 1 - |z_gpu^T S z_lapack| <=
                 max((64 n eps |lambda|_max / gap)^2, 64 eps) -- two backward-stable answers cannot differ by more; a cluster update
                 that spills into the eigenvector next to the cluster shows here.
The figures of the GPU and of LAPACK are written with `note` (tests/test_gpu_stages.py), beside those of the stage tests."""
import numpy as np
import pytest
import pencils as pc
from pencils import EPS
from test_gpu_stages import note

pytestmark = pytest.mark.gpu
from bspatom_amd import capi


class _Route:
    def __init__(self, route):
        self.route = route
    def __enter__(self):
        self.old = capi.get_option("route")
        capi.set_option("route", self.route)
    def __exit__(self, *a):
        capi.set_option("route", self.old)


def contract(name, route=0):
    """One jobz = 'V' call on the case and every common assertion; returns (w, Z)."""
    c = pc.case(name)
    n, H, S = c.n, c.H, c.S
    with _Route(route):
        w, Z, U, info = capi.dsygv(H, S, jobz="V", uplo="U")
        w2, Z2, _, info2 = capi.dsygv(H, S, jobz="V", uplo="U")
        wN, _, _, infoN = capi.dsygv(H, S, jobz="N", uplo="U")
    tag = "pencil %s n=%d p=%d route %d" % (name, n, c.p, route)
    assert info == 0 and info2 == 0 and infoN == 0, tag
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(Z)), tag
    assert np.all(np.diff(w) >= 0), tag
    assert np.array_equal(w, wN), tag
    assert np.array_equal(w, w2) and np.array_equal(Z, Z2), tag
    assert np.max(np.abs(np.triu(U).T @ np.triu(U) - S)) < 1e-13, tag
    # eigenvalues against the truth, LAPACK's beside them
    wl, Zl = pc.lapack(name)
    idx, tru, lam = pc.truth(name)
    eg = np.max(np.abs(w[idx] - tru)) / lam; el = np.max(np.abs(wl[idx] - tru)) / lam
    # eigenvectors
    orth, resid = pc.metrics(H, S, w, Z)
    orth_l, resid_l = pc.metrics(H, S, wl, Zl)
    # isolated eigenvalues: the angle to LAPACK's vector
    g = pc.gaps(w)
    iso = [c0 for c0, c1 in pc.clusters_by_rule(w) if c1 - c0 == 1]
    worst = 0.0
    if iso:
        ov = np.abs(np.sum(Z[:, iso] * (S @ Zl[:, iso]), axis=0))
        bound = np.maximum((64 * n * EPS * lam / g[iso]) ** 2, 64 * EPS)
        worst = float(np.max((1.0 - ov) / bound))
    note("%s | eig err/lmax gpu %.2e lapack %.2e | orth gpu %.2e lapack %.2e (bar %.2e) | resid gpu %.2e lapack %.2e (bar %.2e) | "
         "isolated %d, worst (1-|cos|)/bound %.2e"
         % (tag, eg, el, orth, orth_l, max(4 * n * EPS, 16 * orth_l), resid, resid_l, max(32 * n * EPS, 16 * resid_l), len(iso), worst))
    assert eg <= 1e-13, tag
    assert orth <= max(4 * n * EPS, 16 * orth_l), tag
    assert resid <= max(32 * n * EPS, 16 * resid_l), tag
    assert worst <= 1.0, tag
    if name[0] in "CE" and name != "E-unequal":                       # the cluster geometry the case is about (gaps far from the rule's threshold)
        assert [c1 - c0 for c0, c1 in pc.clusters_by_rule(w)] == list(c.sizes), tag
    return w, Z


# ---- A: sizes ------------------------------------------------------------------------------------------------------------------
# the band route takes n >= 16 (and is the default from 32 on); both routes wherever both run, each against the truth
A_PARAMS = [(n, r) for n in pc.A_SIZES for r in ((1, 2) if n >= 16 else (0,))]


@pytest.mark.parametrize("n,route", A_PARAMS)
def test_sizes(n, route):
    contract("A-n%d" % n, route)


# ---- B: half-widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", pc.B_WIDTHS)
def test_half_widths(p):
    w, Z = contract("B-p%d" % p)
    if p == 0:
        # a diagonal pencil in shuffled order: w = sorted H_ii / S_ii, Z = the unit vectors over sqrt(S_ii)
        c = pc.case("B-p0")
        h, s = np.diag(c.H), np.diag(c.S)
        o = np.argsort(h / s)
        assert np.max(np.abs(w - (h / s)[o])) <= 1e-13
        Zx = np.zeros((c.n, c.n)); Zx[o, np.arange(c.n)] = 1.0 / np.sqrt(s[o])
        assert np.max(np.abs(np.abs(Z) - Zx)) <= 4 * c.n * EPS


def test_half_width_16_is_refused():
    H, S = pc.make_pencil(pc.spectrum("uniform", 200), 16, 216)
    w, a, b, info = capi.dsygv(H, S, jobz="V", uplo="U")
    assert info == -5
    assert np.array_equal(a, H) and np.array_equal(b, S) and not w.any()


# ---- C: cluster geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C-p4", "C-p12", "C-uniform"])
def test_cluster_geometry(name):
    """C-p4 / C-p12: clusters of 1, 2, 63, 64, 65, 1, 129, 3, 272 columns in one call (band route with invit<8>, dense route with
    invit<15>): clusters that start beyond column 0, odd blocks, short blocks, foreign eigenvectors on both sides, the last one across
    the 512-vector chunk boundary.  C-uniform: no cluster at all (the branch without orthonormalisation)."""
    contract(name)


# ---- D: near-degenerate --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 8])
def test_near_degenerate(p):
    contract("D-p%d" % p)


# ---- E: exactly degenerate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E-sum2", "E-sum3", "E-diag", "E-unequal"])
def test_exactly_degenerate(name):
    """Multiplicities 2, 3 and 64: the full contract -- an S-orthonormal basis of every eigenspace --, not an error return.
    E-unequal: a simple spectrum on a pencil that splits into two blocks (zero reflectors and rotations in the reduction)."""
    w, Z = contract(name)
    if name == "E-unequal":
        c = pc.case(name)
        wN, _, _, info = capi.dsygv(c.H, c.S, jobz="N", uplo="U")
        idx, tru, lam = pc.truth(name)
        assert info == 0 and np.max(np.abs(wN[idx] - tru)) <= 1e-13 * lam


# ---- F: persymmetric double well -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F-n255", "F-n256", "F-deep128"])
def test_persymmetric_double_well(name):
    """Every eigenvector is symmetric or antisymmetric and the start vector of the inverse iteration is exactly S-orthogonal to the
    antisymmetric ones; pairs with small gaps at the bottom of the wells.  F-deep128: the pair gaps run from far below the resolution
    of double precision (a double eigenvalue for every purpose, with a generic eigenspace) through 6e-14 and 8e-12 |lambda|_max up."""
    w, Z = contract(name)
    n = len(w)
    lam = np.max(np.abs(w)); g = pc.gaps(w)
    worst = 0.0
    for i in [c0 for c0, c1 in pc.clusters_by_rule(w) if c1 - c0 == 1]:
        z = Z[:, i]
        d = min(np.max(np.abs(z[::-1] - z)), np.max(np.abs(z[::-1] + z)))
        worst = max(worst, d / (64 * n * EPS * lam / g[i] * np.max(np.abs(z))))
    note("pencil %s: worst parity defect / bound outside clusters %.2e" % (name, worst))
    assert worst <= 1.0


# ---- G: calling convention -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A-n65", "B-p9"])
@pytest.mark.parametrize("uplo", ["U", "L"])
def test_unreferenced_triangle_is_not_read(name, uplo):
    c = pc.case(name)
    n = c.n
    w0, Z0, F0, info0 = capi.dsygv(c.H, c.S, jobz="V", uplo=uplo)
    assert info0 == 0
    other = np.tril(np.ones((n, n), dtype=bool), -1) if uplo == "U" else np.triu(np.ones((n, n), dtype=bool), 1)
    Hn = c.H.copy(); Sn = c.S.copy()
    Hn[other] = np.nan; Sn[other] = np.nan
    w, Z, F, info = capi.dsygv(Hn, Sn, jobz="V", uplo=uplo)
    assert info == 0
    assert np.array_equal(w, w0) and np.array_equal(Z, Z0)
    assert np.all(np.isnan(F[other])) and np.array_equal(F[~other], F0[~other])
    T = np.triu(F0) if uplo == "U" else np.tril(F0).T
    assert np.max(np.abs(T.T @ T - c.S)) < 1e-13
    wN, A, _, infoN = capi.dsygv(Hn, Sn, jobz="N", uplo=uplo)
    assert infoN == 0 and np.array_equal(wN, w0)


@pytest.mark.parametrize("name", ["A-n65", "B-p9"])
@pytest.mark.parametrize("uplo", ["U", "L"])
def test_leading_dimensions(name, uplo):
    c = pc.case(name)
    n = c.n
    w0, Z0, F0, info0 = capi.dsygv(c.H, c.S, jobz="V", uplo=uplo)
    w, a, b, info = capi.dsygv(c.H, c.S, jobz="V", uplo=uplo, lda=n + 3, ldb=n + 5, sentinel=-777.0)
    assert info0 == 0 and info == 0
    assert a.shape == (n + 3, n) and b.shape == (n + 5, n)
    assert np.all(a[n:] == -777.0) and np.all(b[n:] == -777.0)
    assert np.array_equal(w, w0) and np.array_equal(a[:n], Z0)
    ref = np.triu(np.ones((n, n), dtype=bool)) if uplo == "U" else np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(b[:n][ref], F0[ref])


# ---- H: scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["H-up", "H-down", "H-graded"])
def test_scale(name):
    """The near-degenerate pencil with H times 2^200 and 2^-200 (every figure of the contract is relative), and a spectrum graded over
    ten decades with both signs (eigenvalues against the truth normwise)."""
    contract(name)


# ---- I: not positive definite --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("pos", [0, 16, 50, 99])
def test_not_positive_definite(pos, route):
    from scipy.linalg import lapack
    n = 100
    H, S = pc.not_positive_definite(n, 4, pos)
    _, pinfo = lapack.dpotrf(S, lower=0)
    assert pinfo == pos + 1
    with _Route(route):
        for jobz in ("N", "V"):
            w, a, b, info = capi.dsygv(H, S, jobz=jobz, uplo="U")
            assert info - n == pinfo, (jobz, info)
