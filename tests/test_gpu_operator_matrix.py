"""Matrix elements of caller-given radial operators g(r), g(r) d/dr (bspatom_operator_bands / bspatom_operator_matrix and their
_dev variants, csrc/opmat.hip): the bands against bspatom_dipole_bands and against an ordered CPU restatement, bit for bit; the
matrix against its own bands, against bspatom_dipole_matrix and against the independent quadrature route host.radial_matrix;
independence of the batch, of the grouping and of the other operators; the device variants; the argument checks.

The bounds.
  Against the bands (tests 3, 4): both sides evaluate z^T A x in floating point from the same z, G_o and x, so
      |D - ref| <= 2 (n + 2k + nop + 1) eps sum_i |z_i| (|A| |x|)_i,   |A| = sum_o |a_o| |G_o|
  (per path nop roundings of an entry of A, 2k - 1 of a row of A x, n + 1 of the dot product; at nop = 3 this is the n + 2k + 4 of
  tests/test_gpu_dipole_matrix.py).
  Against host.radial_matrix (test 5): both sides evaluate the same quadrature sum in exact arithmetic from bit-identical
  eigenvectors, so |D - R| <= m eps S_abs with
      S_abs[i, f] = sum_q w_q (sum_o |a_o| |g_o(q)| X_i^o(q)) U_f(q),  U_f = |Z_f| @ B,  X_i^o = |Z_i| @ B or |Z_i| @ |B'|,
      m = npts + n + 4k + k ka + nop + 7
  the sum of the longest rounding chains of the two paths (tables plus NumPy contraction: npts + 2k + 4; band route:
  n + 2k + k ka + nop + 3); eps = 2^-52 is twice the unit roundoff, which is the margin."""
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny


def _problem(name):
    return capi.Problem(input_from_case(name))


def _solved(name, nl=None, **over):
    prob = capi.Problem(input_from_case(name, **over))
    nl = prob.lmax + 1 if nl is None else nl
    E, info = prob.solve(0, nl)
    assert np.all(info == 0)
    return prob


def band_apply(A, X):
    """Y[j] = A x_j for the rows x_j of X (m, n); A (2k-1, n) with A[d + k - 1][i] = A(i, i + d)"""
    k, n = (A.shape[0] + 1) // 2, A.shape[1]
    Y = np.zeros_like(X)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)                     # rows i with 0 <= i + d < n
        Y[:, lo:hi] += A[d + k - 1, lo:hi] * X[:, lo + d:hi + d]
    return Y


def combine(GB, a):
    return sum(a[o] * GB[o] for o in range(len(a)))


def abs_combine(GB, a):
    return sum(abs(a[o]) * np.abs(GB[o]) for o in range(len(a)))


def band_bound(prob, nop, GB, a, X, Z):
    """2 (n + 2k + nop + 1) eps sum_i |z_i| (|A| |x|)_i for the rows of X (initial) and Z (final)"""
    S = band_apply(abs_combine(GB, a), np.abs(X)) @ np.abs(Z).T
    return 2.0 * (prob.nfun + 2 * prob.k + nop + 1) * EPS * S


def check_block(tag, D, R, B):
    ratio = float(np.max(np.abs(D - R) / np.maximum(B, TINY)))
    note("operator_matrix %s: max |D - ref| / bound = %.3g (max|D| %.3g)" % (tag, ratio, np.max(np.abs(R))))
    assert np.all(np.abs(D - R) <= B), (tag, ratio)
    return ratio


class Vecs:
    """eigenvector blocks of a solved problem, cached per (channel, window)"""

    def __init__(self, prob):
        self.prob, self.Z = prob, {}

    def __call__(self, l, n0, count):
        key = (l, n0, count)
        if key not in self.Z:
            self.Z[key] = self.prob.eigvecs(l, n0, count)
        return self.Z[key]


def some_operators(r, nop, seed):
    """nop operators on the grid r: smooth profiles of either sign and random ones, derivatives among them"""
    rng = np.random.default_rng(seed)
    pool = [(r ** 2, 0), (rng.standard_normal(r.size), 1), (np.exp(-r / 5.0), 0), (np.cos(r), 1), (rng.standard_normal(r.size), 0)]
    g = np.stack([pool[o % 5][0] for o in range(nop)])
    deriv = np.array([pool[o % 5][1] for o in range(nop)], dtype=np.int32)
    return g, deriv


@pytest.fixture(scope="module")
def lin256():
    prob = _solved("lin256")
    assert prob.lmax == 3
    yield prob
    prob.close()


@pytest.fixture(scope="module")
def lin1024():
    prob = _solved("lin1024", 2)
    yield prob
    prob.close()


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "c1_exp", "ka_ra", "bc1", "bc10", "c5_1024_k11"])
def test_operator_bands_equal_dipole_bands(name):
    """g = (r, 1/r, 1), deriv = (0, 0, 1) on the r of quadrature(): the three bands are dipole_bands() bit for bit, alone and
    at positions 1, 4 and 7 of nine operators whose other six are random (nop no multiple of the register block; an operator's
    band does not depend on its company).  n below one tile, odd n, k = 4 and 11, an exponential grid, ka != k + 3 with
    ra != 0, boundary conditions that move the zero-width intervals.  On n65_k4 the _dev variant equals the host variant."""
    prob = _problem(name)
    RB = prob.dipole_bands()
    r, w = prob.quadrature()
    g3, d3 = np.stack([r, 1.0 / r, np.ones_like(r)]), np.array([0, 0, 1], dtype=np.int32)
    GB = prob.operator_bands(g3, d3)
    assert GB.shape == RB.shape == (3, 2 * prob.k - 1, prob.nfun)
    assert np.array_equal(GB, RB)
    rng = np.random.default_rng(11)
    g9, d9 = rng.standard_normal((9, r.size)), rng.integers(0, 2, size=9).astype(np.int32)
    g9[[1, 4, 7]], d9[[1, 4, 7]] = g3, d3
    GB9 = prob.operator_bands(g9, d9)
    assert np.array_equal(GB9[[1, 4, 7]], RB)
    assert np.all(np.isfinite(GB9)) and np.max(np.abs(GB9[0])) > 0 and np.max(np.abs(GB9[8])) > 0
    if name == "n65_k4":
        gd = torch.from_numpy(g9).to("cuda:0")
        out = torch.full(GB9.shape, float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        prob.operator_bands_dev(9, gd.data_ptr(), d9, out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), GB9)
    prob.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "bc1"])
def test_operator_bands_equal_ordered_cpu_restatement(name):
    """B, dB = tabulate(identity) on the quadrature grid are the point table's B_j, B_j' exactly (one nonzero coefficient: the
    documented summation of bspatom_tabulate adds zeros to it).  The restatement of an entry is the sequential sum
    np.add.accumulate(((B_i * g) * X_j) * w)[-1] over ALL points ascending: outside the common support the terms are zero and
    change nothing.  g = r^2, exp(-r/5), a random array of both signs, deriv both ways: np.array_equal on every in-range entry,
    0 where i + d is outside 0 .. nfun-1."""
    prob = _problem(name)
    n, k = prob.nfun, prob.k
    r, w = prob.quadrature()
    B, dB = prob.tabulate(np.eye(n))
    gs = [r ** 2, np.exp(-r / 5.0), np.random.default_rng(5).standard_normal(r.size)]
    g = np.stack(gs + gs)
    deriv = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    GB = prob.operator_bands(g, deriv)
    for o in range(6):
        X = dB if deriv[o] else B
        for d in range(-(k - 1), k):
            lo, hi = max(0, -d), min(n, n - d)
            T = ((B[lo:hi] * g[o]) * X[lo + d:hi + d]) * w
            ref = np.add.accumulate(T, axis=1)[:, -1]
            got = GB[o, d + k - 1]
            assert np.array_equal(got[lo:hi], ref), (name, o, d)
            assert np.all(got[:lo] == 0.0) and np.all(got[hi:] == 0.0), (name, o, d)
        assert np.max(np.abs(GB[o])) > 0
    prob.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 1), (1, 0), (1, 1), (0, 1)]
RATIOS = {}


@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "lin256", "c5_1024_k11"])
def test_operator_matrix_vs_its_own_bands(name):
    """The pairs and windows of test_dipole_matrix_vs_per_state_call, nop = 1, 3, 5: every element within the bound of
    z_f^T (sum_o a_o G_o) x_i evaluated in NumPy from operator_bands and eigvecs; the repeated pair bit-identical to its first
    occurrence."""
    prob = _solved(name, 2)
    n, vec = prob.nfun, Vecs(prob)
    r = prob.quadrature()[0]
    cf = min(37, n - 1)
    cf = cf if cf % 2 else cf - 1
    worst = 0.0
    for nop in (1, 3, 5):
        g, deriv = some_operators(r, nop, 100 + nop)
        GB = prob.operator_bands(g, deriv)
        a0 = np.random.default_rng(nop).standard_normal(nop)
        a = np.stack([a0, 1.25 * a0, -1.5 * a0, a0])
        for ci in (1, min(17, n)):
            for n0_ini, n0_fin in ((1, 2), (n - ci + 1, n - cf + 1)):
                D = prob.operator_matrix(PAIRS, g, deriv, n0_ini, ci, n0_fin, cf, a)
                assert D.shape == (4, ci, cf)
                for p in range(3):
                    li, lf = PAIRS[p]
                    X, Z = vec(li, n0_ini, ci), vec(lf, n0_fin, cf)
                    R = band_apply(combine(GB, a[p]), X) @ Z.T
                    worst = max(worst, check_block("%s nop %d pair %s ci %d n0 %d/%d" % (name, nop, PAIRS[p], ci, n0_ini, n0_fin),
                                                   D[p], R, band_bound(prob, nop, GB, a[p], X, Z)))
                assert np.array_equal(D[3], D[0])
                assert np.max(np.abs(D)) > 0
    note("operator_matrix %s vs its own bands: worst ratio %.3g" % (name, worst))
    prob.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------
GAUGES = {"length": np.array([0.75, 0.0, 0.0]), "velocity": np.array([0.0, 2.0, -1.0])}


def test_operator_matrix_vs_dipole_matrix(lin256):
    """g = (r, 1/r, 1), deriv = (0, 0, 1), both gauges: within the same bound of dipole_matrix (not bit-identical: dipole.hip
    contracts its apply into FMAs, opmat.hip does not)."""
    prob = lin256
    vec = Vecs(prob)
    r = prob.quadrature()[0]
    g, deriv = np.stack([r, 1.0 / r, np.ones_like(r)]), [0, 0, 1]
    GB = prob.operator_bands(g, deriv)
    pairs = [(0, 1), (1, 0), (1, 1), (2, 3)]
    for gname, a in GAUGES.items():
        D = prob.operator_matrix(pairs, g, deriv, 1, 17, 2, 37, a)
        R = prob.dipole_matrix(pairs, 1, 17, 2, 37, a)
        for p, (li, lf) in enumerate(pairs):
            check_block("lin256 %s pair %s vs dipole_matrix" % (gname, pairs[p]), D[p], R[p],
                        band_bound(prob, 3, GB, a, vec(li, 1, 17), vec(lf, 2, 37)))
        assert np.max(np.abs(D)) > 0.1


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lin256", "c1_exp"])
def test_operator_matrix_vs_radial_matrix(name):
    """States 1 .. 32, pairs (0, 1) and (1, 2): r^2, exp(-r/5), r d/dr alone and a three-operator combination with mixed deriv
    against host.radial_matrix (the sum of three results for the combination): |D - R| <= m eps S_abs (module docstring)."""
    prob = _solved(name, 3, l_fin=2)
    n, k, ka = prob.nfun, prob.k, prob.ka
    pairs, cnt = [(0, 1), (1, 2)], 32
    r, w = prob.quadrature()
    B, dB = prob.tabulate(np.eye(n))
    Zabs = [np.abs(prob.eigvecs(l, 1, cnt)) for l in range(3)]
    ZB, ZdB = [z @ B for z in Zabs], [z @ np.abs(dB) for z in Zabs]
    single = [("r^2", [(lambda x: x ** 2, False)], None), ("exp(-r/5)", [(lambda x: np.exp(-x / 5.0), False)], None),
              ("r d/dr", [(lambda x: x, True)], None),
              ("0.5 r^2 - 2 exp(-r/5) d/dr + 1.5 r d/dr", [(lambda x: x ** 2, False), (lambda x: np.exp(-x / 5.0), True), (lambda x: x, True)],
               [0.5, -2.0, 1.5])]
    worst = 0.0
    for tag, ops, a in single:
        nop = len(ops)
        av = np.ones(1) if a is None else np.asarray(a)
        D = host.operator_matrix(prob, pairs, ops, 1, cnt, 1, cnt, a)
        R = sum(av[o] * host.radial_matrix(prob, pairs, ops[o][0], 1, cnt, 1, cnt, deriv=ops[o][1]) for o in range(nop))
        assert D.shape == R.shape == (2, cnt, cnt)
        m = r.size + n + 4 * k + k * ka + nop + 7
        for p, (li, lf) in enumerate(pairs):
            S = sum(abs(av[o]) * ((ZdB[li] if ops[o][1] else ZB[li]) * (np.abs(ops[o][0](r)) * w)) @ ZB[lf].T for o in range(nop))
            bound = m * EPS * S
            ratio = float(np.max(np.abs(D[p] - R[p]) / np.maximum(bound, TINY)))
            worst = max(worst, ratio)
            note("operator_matrix %s %s pair %s vs radial_matrix: max |D - R| / (m eps S_abs) = %.3g (m = %d, max|D| %.3g)"
                 % (name, tag, pairs[p], ratio, m, np.max(np.abs(R[p]))))
            assert np.all(np.abs(D[p] - R[p]) <= bound), (name, tag, p, ratio)
            assert np.max(np.abs(D[p])) > 0
    note("operator_matrix %s vs radial_matrix: worst ratio %.3g" % (name, worst))
    prob.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def _independence(prob, pairs, n0_ini, ci, n0_fin, cf, g, deriv, a):
    nop = len(deriv)
    D = prob.operator_matrix(pairs, g, deriv, n0_ini, ci, n0_fin, cf, a)
    assert np.array_equal(D, prob.operator_matrix(pairs, g, deriv, n0_ini, ci, n0_fin, cf, a))          # run to run
    alone = [prob.operator_matrix([pairs[p]], g, deriv, n0_ini, ci, n0_fin, cf, a[p])[0] for p in range(len(pairs))]
    for p in range(len(pairs)):
        assert np.array_equal(alone[p], D[p]), p
    gd = torch.from_numpy(np.ascontiguousarray(g)).to("cuda:0")
    capi.set_option("dipole_stage_mb", 1)                # several groups: two pairs of these sizes do not fit into 1 MiB
    try:
        Dg = prob.operator_matrix(pairs, g, deriv, n0_ini, ci, n0_fin, cf, a)
        Dd = torch.full(D.shape, float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        prob.operator_matrix_dev(pairs, nop, gd.data_ptr(), deriv, n0_ini, ci, n0_fin, cf, a, Dd.data_ptr())
    finally:
        capi.set_option("dipole_stage_mb", 0)
    assert np.array_equal(Dg, D)
    assert np.array_equal(Dd.cpu().numpy(), D)
    Dd.fill_(float("nan"))
    torch.cuda.synchronize()
    prob.operator_matrix_dev(pairs, nop, gd.data_ptr(), deriv, n0_ini, ci, n0_fin, cf, a, Dd.data_ptr())   # one group
    assert np.array_equal(Dd.cpu().numpy(), D)
    assert np.array_equal(prob.operator_matrix(pairs, g, deriv, n0_ini, ci, n0_fin, cf, a[1]),
                          prob.operator_matrix(pairs, g, deriv, n0_ini, ci, n0_fin, cf, np.tile(a[1], (len(pairs), 1))))
    assert np.max(np.abs(D)) > 0 and np.all(np.isfinite(D))


def test_operator_matrix_independent_of_batch_and_grouping(lin256, lin1024):
    """nop = 4.  lin256, seven pairs (channels repeated in both roles, l_ini = l_fin among them, windows of 101 and 120 states):
    the same call twice is bit-identical; every pair called alone equals its block of the joint call; so does the joint call cut
    into groups by dipole_stage_mb = 1, host and device variants (g a torch tensor, D pre-filled with NaN); a of shape (nop,)
    equals its tiling.  Then three pairs at n = 1024, where the product runs in four K slices."""
    rng = np.random.default_rng(7)
    prob = lin256
    g, deriv = some_operators(prob.quadrature()[0], 4, 21)
    a = rng.standard_normal((7, 4))
    a[2, 1:] = 0.0
    _independence(prob, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (2, 2)], 2, 101, 5, 120, g, deriv, a)
    prob = lin1024
    g, deriv = some_operators(prob.quadrature()[0], 4, 22)
    _independence(prob, [(0, 1), (1, 0), (1, 1)], 3, 40, 2, 33, g, deriv, rng.standard_normal((3, 4)))


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_operator_argument_checks():
    prob = _solved("c1_lin")
    nch, n, L = prob.lmax + 1, prob.nfun, capi.lib()
    r = prob.quadrature()[0]
    nop = 2
    g = np.ascontiguousarray(np.stack([r, np.ones_like(r)]))
    deriv = np.array([0, 1], dtype=np.int32)
    gd = torch.from_numpy(g).to("cuda:0")
    Dd = torch.zeros(4 * n, dtype=torch.float64, device="cuda:0")
    GBd = torch.zeros(nop * (2 * prob.k - 1) * n, dtype=torch.float64, device="cuda:0")
    a = [1.0, 0.5]
    bad = [([], 1, 1, 1, 1),                    # npairs = 0
           ([(0, 1)], 1, 0, 1, 1),              # count_ini = 0
           ([(0, 1)], 1, 1, 1, 0),              # count_fin = 0
           ([(0, 1)], 0, 1, 1, 1),              # n0_ini = 0
           ([(0, 1)], 1, 1, 0, 1),              # n0_fin = 0
           ([(0, 1)], n, 2, 1, 1),              # initial window beyond nfun
           ([(0, 1)], 1, 1, n - 1, 3),          # final window beyond nfun
           ([(0, nch)], 1, 1, 1, 1),            # final channel outside the last solve
           ([(0, 1), (-1, 1)], 1, 1, 1, 1)]     # initial channel outside the last solve, second pair
    for args in bad:
        aa = np.zeros((0, nop)) if not args[0] else a
        with pytest.raises(capi.BspAtomError) as ei:
            prob.operator_matrix(args[0], g, deriv, *args[1:], aa)
        assert ei.value.code == -2, args
        with pytest.raises(capi.BspAtomError) as ei:
            prob.operator_matrix_dev(args[0], nop, gd.data_ptr(), deriv, *args[1:], aa, Dd.data_ptr())
        assert ei.value.code == -2, args
    # null pointers, nop = 0, deriv outside {0, 1}: the C entry points themselves
    li, lf = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    av, D, GB = np.array(a), np.zeros(1), np.zeros(nop * (2 * prob.k - 1) * n)
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    d2, dm1 = np.array([0, 2], dtype=np.int32), np.array([-1, 1], dtype=np.int32)
    for fn, gp, out in ((L.bspatom_operator_matrix, p_(g), p_(D)),
                        (L.bspatom_operator_matrix_dev, C.c_void_p(gd.data_ptr()), C.c_void_p(Dd.data_ptr()))):
        good = [prob._h, nop, gp, p_(deriv), 1, p_(li), p_(lf), 1, 1, 1, 1, p_(av), out]
        assert fn(*good) == 0
        for pos in (0, 2, 3, 5, 6, 11, 12):                            # p, g, deriv, l_ini, l_fin, a, D
            assert fn(*[None if i == pos else v for i, v in enumerate(good)]) == -2, pos
        assert fn(*[0 if i == 1 else v for i, v in enumerate(good)]) == -2          # nop = 0
        assert fn(*[-1 if i == 1 else v for i, v in enumerate(good)]) == -2
        assert fn(*[p_(d2) if i == 3 else v for i, v in enumerate(good)]) == -2     # deriv = 2
        assert fn(*[p_(dm1) if i == 3 else v for i, v in enumerate(good)]) == -2    # deriv = -1
        assert fn(*good) == 0                                                       # a valid call afterwards
    for fn, gp, out in ((L.bspatom_operator_bands, p_(g), p_(GB)),
                        (L.bspatom_operator_bands_dev, C.c_void_p(gd.data_ptr()), C.c_void_p(GBd.data_ptr()))):
        good = [prob._h, nop, gp, p_(deriv), out]
        assert fn(*good) == 0
        for pos in (0, 2, 3, 4):
            assert fn(*[None if i == pos else v for i, v in enumerate(good)]) == -2, pos
        assert fn(*[0 if i == 1 else v for i, v in enumerate(good)]) == -2
        assert fn(*[p_(d2) if i == 3 else v for i, v in enumerate(good)]) == -2
        assert fn(*[p_(dm1) if i == 3 else v for i, v in enumerate(good)]) == -2
        assert fn(*good) == 0
    assert np.array_equal(GBd.cpu().numpy(), GB)
    prob.operator_matrix([(0, 1)], g, deriv, 1, 2, 1, 2, a)            # valid
    prob.assemble(0, nch)                                              # invalidates the state of the last solve
    for call in (lambda: prob.operator_matrix([(0, 1)], g, deriv, 1, 1, 1, 1, a),
                 lambda: prob.operator_matrix_dev([(0, 1)], nop, gd.data_ptr(), deriv, 1, 1, 1, 1, a, Dd.data_ptr())):
        with pytest.raises(capi.BspAtomError) as ei:
            call()
        assert ei.value.code == -2
    assert np.array_equal(prob.operator_bands(g, deriv).reshape(-1), GB)   # the bands need no solve
    prob.close()
