"""The synthetic pencils of tests/pencils.py are fair inputs: checked here with LAPACK and the 113-bit truth alone, no GPU.

For every case that tests/test_gpu_dsygv_pencils.py hands to bsp_dsygv_: the half-width is the intended one, the persymmetric
pencils are persymmetric bit for bit, the cluster rule applied to LAPACK's eigenvalues finds exactly the intended clusters, the
repeated blocks give the intended multiplicities -- and LAPACK itself passes every bar of the GPU test with a margin:
    eigenvalues   |w - truth| <= 1e-13 |lambda|_max / 4
    orth          <= 4 n eps / 4          (the GPU bar is max(4 n eps, 16 x LAPACK's))
    resid         <= 32 n eps / 16        (the GPU bar is max(32 n eps, 16 x LAPACK's))
so a GPU result that misses a bar is the library's fault, not the input's."""
import numpy as np
import pytest
import pencils as pc
from pencils import EPS


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_case_is_a_fair_input(name):
    c = pc.case(name)
    n = c.n
    assert c.H.shape == (n, n) and c.S.shape == (n, n)
    assert np.array_equal(c.H, c.H.T) and np.array_equal(c.S, c.S.T)
    assert max(pc.half_width(c.H), pc.half_width(c.S)) == c.p
    w, Z = pc.lapack(name)
    lam = np.max(np.abs(w))
    if c.sizes is not None:
        assert [c1 - c0 for c0, c1 in pc.clusters_by_rule(w)] == list(c.sizes)
    idx, tru, tlam = pc.truth(name)
    err = np.max(np.abs(w[idx] - tru)) / lam
    orth, resid = pc.metrics(c.H, c.S, w, Z)
    print("%s n=%d p=%d: LAPACK eig err %.2e  orth %.2e = %.3f n eps  resid %.2e = %.4f n eps  cond(S) %.1e"
          % (name, n, c.p, err, orth, orth / (n * EPS), resid, resid / (n * EPS), np.linalg.cond(c.S)))
    assert err <= 1e-13 / 4
    assert orth <= 4 * n * EPS / 4
    assert resid <= 32 * n * EPS / 16


def test_prescribed_spectrum_and_eigenvectors():
    """make_pencil: eigenvalues `lams` to a few eps |lambda|_max, eigenvectors U^-1 e_i (checked through the pencil itself)."""
    for n, p in ((200, 1), (200, 8), (500, 4), (500, 15)):
        lams = pc.spectrum("uniform", n)
        H, S, U, lp = pc.make_pencil(lams, p, 7 * n + p, return_factor=True)
        assert max(pc.half_width(H), pc.half_width(S)) == p
        idx = np.arange(0, n, 7)
        from oracle import truth as tq
        hi, _ = tq.band_eigs(pc.upper_bands(S, p + 1), pc.upper_bands(H, p + 1), idx, lams[idx], 1.0, rtol=1e-20)
        assert np.max(np.abs(hi - lams[idx])) <= 32 * EPS
        X = np.linalg.solve(U, np.eye(n))                                  # column i: U^-1 e_i, eigenvalue lp[i]
        orth, resid = pc.metrics(H, S, lp, X)
        assert orth <= 64 * EPS * np.linalg.cond(U) and resid <= 64 * EPS * np.linalg.cond(U)


def test_clusters_spectrum_geometry():
    """The last cluster of `clusters` at n = 600 covers columns 328 .. 599: across the boundary of the 512-vector chunks."""
    cl = pc.clusters_by_rule(pc.spectrum("clusters", 600))
    assert [c1 - c0 for c0, c1 in cl] == [1, 2, 63, 64, 65, 1, 129, 3, 272]
    assert cl[-1] == (328, 600) and cl[2][0] == 3 and cl[6] == (196, 325)


def test_tight_and_graded_spectra():
    t = pc.spectrum("tight", 300)
    d = np.diff(t)
    assert np.sum(d < 1e-12) == pc.TIGHT_COUNT - 1 and np.all(d > 0.5e-13)
    assert np.min(d[d >= 1e-12]) > 2e-3                                    # the rest is isolated under the rule
    g = pc.spectrum("graded", 400)
    assert np.all(np.diff(g) > 0) and g[0] == -1.0 and np.min(np.abs(g)) <= 1e-10 and np.sum(g > 0) == 200


@pytest.mark.parametrize("name", ["F-n255", "F-n256", "F-deep128"])
def test_persymmetry_bit_for_bit(name):
    c = pc.case(name)
    assert np.array_equal(c.H[::-1, ::-1], c.H) and np.array_equal(c.S[::-1, ::-1], c.S)
    w, Z = pc.lapack(name)
    g = pc.gaps(w)
    lam = np.max(np.abs(w))
    # the double well: pairs with small gaps at the bottom, and LAPACK's vectors outside clusters are symmetric or antisymmetric
    assert np.min(g[:8]) < 1e-3 * lam
    if name == "F-deep128":                                                # unresolved pairs, and pairs between 64 eps and 1e-10 of the norm
        assert np.sum(g < 8 * EPS * lam) >= 4 and np.sum((g > 64 * EPS * lam) & (g < 1e-10 * lam)) >= 4
    iso = [c0 for c0, c1 in pc.clusters_by_rule(w) if c1 - c0 == 1]
    assert len(iso) >= c.n // 4
    for i in iso:
        z = Z[:, i]
        d = min(np.max(np.abs(z[::-1] - z)), np.max(np.abs(z[::-1] + z)))
        assert d <= 64 * c.n * EPS * lam / g[i] * np.max(np.abs(z)) / 16
    # the constant vector is S-orthogonal to every antisymmetric one: about half of the isolated vectors
    ov = np.abs(np.ones(c.n) @ c.S @ Z[:, iso]) / np.sqrt(np.ones(c.n) @ c.S @ np.ones(c.n))
    assert c.n // 8 <= np.sum(ov < 1e-10) <= len(iso)


@pytest.mark.parametrize("name", ["E-sum2", "E-sum3", "E-diag"])
def test_exact_multiplicities(name):
    c = pc.case(name)
    from oracle import truth as tq
    w = pc.lapack(name)[0]
    lam = float(np.max(np.abs(w)))
    k = max(c.p, 1) + 1
    tru, _ = tq.band_eigs(pc.upper_bands(c.S, k), pc.upper_bands(c.H, k), np.arange(c.n), w, lam, rtol=1e-20)
    # truth resolves 1e-20 relative: copies of one eigenvalue agree far below eps, distinct ones differ far above it
    d = np.diff(tru)
    same = d <= 1e-17 * lam
    assert not np.any((d > 1e-17 * lam) & (d < 1e-6 * lam))
    runs, m = [], 1
    for s in same:
        if s:
            m += 1
        else:
            runs.append(m); m = 1
    runs.append(m)
    assert sorted(r for r in runs if r > 1) == sorted(c.mults)


def test_unequal_blocks_split_but_the_spectrum_is_simple():
    c = pc.case("E-unequal")
    assert c.n == 128 and c.H[36, 37] == 0.0 and c.S[36, 37] == 0.0
    w = pc.lapack("E-unequal")[0]
    assert np.min(np.diff(w)) > 1e-6


def test_direct_sum_and_diagonal_pencil():
    H1, S1 = pc.make_pencil(pc.spectrum("uniform", 5), 2, 1)
    H, S = pc.direct_sum([(H1, S1), (H1, S1)])
    assert np.array_equal(H[5:, 5:], H1) and np.array_equal(S[:5, :5], S1) and not H[:5, 5:].any()
    lams = np.array([0.5, 0.5, -0.25, 0.75])
    Hd, Sd = pc.diagonal_pencil(lams, 3)
    assert sorted(np.diag(Hd) / np.diag(Sd)) == sorted(lams)


@pytest.mark.parametrize("pos", [0, 16, 50, 99])
def test_not_positive_definite_pencil(pos):
    from scipy.linalg import lapack
    H, S = pc.not_positive_definite(100, 4, pos)
    _, info = lapack.dpotrf(S, lower=0)
    assert info == pos + 1
