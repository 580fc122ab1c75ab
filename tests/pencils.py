"""Synthetic banded pencils (H, S) with prescribed spectra, for the tests of bsp_dsygv_ (csrc/dsygv.hip): the inverse iteration,
the cluster rule and the blocked S-orthonormalisation see here what the reference's radial pencils never show them -- several
clusters per call, clusters that start beyond column 0 and are no multiple of 64 wide, isolated eigenvalues beside them, exactly
repeated eigenvalues, eigenvectors the start vector of the inverse iteration is S-orthogonal to.

Plain NumPy, importable without a GPU.  tests/test_pencils_cpu.py proves with LAPACK alone that every case is a fair input;
tests/test_gpu_dsygv_pencils.py feeds the same cases to the library.  A case is built once per process (`case`) and LAPACK's answer
and the 113-bit truth of its eigenvalues are computed once (`lapack`, `truth`) and shared by every test that needs them."""
import functools
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


# ---- generators ----------------------------------------------------------------------------------------------------------------
def _sym_from_upper(M):
    U = np.triu(np.asarray(M, dtype=np.float64))
    return U + np.triu(U, 1).T


def make_pencil(lams, p, seed, offscale=0.3, return_factor=False):
    """H = U^T diag(perm(lams)) U, S = U^T U with U upper triangular of half-width p (diagonal 1 + rand, off-diagonals
    offscale * randn): formed in long double, rounded once to double, symmetrised from the upper triangle.  The pencil has
    half-width exactly p, the eigenvalues `lams` (to a few eps |lambda|_max) and the eigenvectors U^-1 e_i."""
    lams = np.asarray(lams, dtype=np.float64)
    n = len(lams)
    assert 0 <= p < max(n, 1)
    rng = np.random.default_rng(seed)
    Ub = np.zeros((p + 1, n))                                   # Ub[d, i] = U(i, i + d)
    Ub[0] = 1.0 + rng.random(n)
    for d in range(1, p + 1):
        Ub[d, :n - d] = offscale * rng.standard_normal(n - d)
    lp = lams[rng.permutation(n)]
    Ul = Ub.astype(LD); ll = lp.astype(LD)
    H = np.zeros((n, n), dtype=LD); S = np.zeros((n, n), dtype=LD)
    for a in range(p + 1):                                      # (U^T D U)(r + a, r + b) += U(r, r + a) D_r U(r, r + b)
        for b in range(a, p + 1):
            r = np.arange(n - b)
            t = Ul[a, r] * Ul[b, r]
            S[r + a, r + b] += t
            H[r + a, r + b] += t * ll[r]
    H = _sym_from_upper(H); S = _sym_from_upper(S)
    if return_factor:
        U = np.zeros((n, n))
        for d in range(p + 1):
            r = np.arange(n - d)
            U[r, r + d] = Ub[d, r]
        return H, S, U, lp
    return H, S


def diagonal_pencil(lams, seed):
    """S = diag(s), H = diag(s * perm(lams)) with s from a few dyadic values: for lams of at most 40 bits the products are exact, so
    the ratios H_ii / S_ii repeat EXACTLY where lams does."""
    lams = np.asarray(lams, dtype=np.float64)
    rng = np.random.default_rng(seed)
    s = rng.choice(np.array([0.75, 1.0, 1.5, 2.0, 3.0]), size=len(lams))
    lp = lams[rng.permutation(len(lams))]
    h = s * lp
    assert np.array_equal(h / s, lp)
    return np.diag(h), np.diag(s)


def direct_sum(pencils):
    """Block-diagonal pencil of the given (H, S) pairs: the same block repeated gives exact multiplicities."""
    n = sum(P[0].shape[0] for P in pencils)
    H = np.zeros((n, n)); S = np.zeros((n, n))
    o = 0
    for Hb, Sb in pencils:
        m = Hb.shape[0]
        H[o:o + m, o:o + m] = Hb; S[o:o + m, o:o + m] = Sb
        o += m
    return H, S


def persymmetric(n, p, well):
    """Toeplitz banded S and H (half-width p) plus a double-well diagonal v with v[i] == v[n-1-i] bit for bit: J H J == H and
    J S J == S exactly, so every eigenvector is symmetric or antisymmetric under i -> n-1-i -- and the constant start vector of
    the inverse iteration is exactly S-orthogonal to the antisymmetric half.  The two wells give symmetric / antisymmetric pairs
    with small gaps at the bottom of the spectrum."""
    assert 1 <= p < n
    s = np.array([1.0] + [0.25 ** d for d in range(1, p + 1)])             # diagonally dominant: S is positive definite
    h = np.array([2.0] + [-1.0 / d ** 2 for d in range(1, p + 1)])
    half = (n + 1) // 2
    x = (np.arange(half) - (n - 1) / 2.0) / (n / 4.0)                      # wells at a quarter and three quarters of the range
    vh = well * (x * x - 1.0) ** 2
    v = np.empty(n)
    v[:half] = vh; v[n - half:] = vh[::-1]
    H = np.zeros((n, n)); S = np.zeros((n, n))
    for d in range(p + 1):
        r = np.arange(n - d)
        H[r, r + d] = h[d]; S[r, r + d] = s[d]
        H[r + d, r] = h[d]; S[r + d, r] = s[d]
    H[np.arange(n), np.arange(n)] += v
    return H, S


# ---- named spectra -------------------------------------------------------------------------------------------------------------
CLUSTER_SIZES = [1, 2, 63, 64, 65, 1, 129, 3]                              # then the rest of n in one last cluster
TIGHT_COUNT, TIGHT_STEP = 40, 1e-13


def cluster_sizes(n):
    rest = n - sum(CLUSTER_SIZES)
    assert rest > 0
    return CLUSTER_SIZES + [rest]


def spectrum(name, n):
    if name == "uniform":
        return np.linspace(-1.0, 1.0, n)
    if name == "clusters":                                                 # centres 1, 2, 3, ..., each 1e-6 wide
        out = []
        for c, m in enumerate(cluster_sizes(n)):
            out.append(c + 1.0 + (np.linspace(-0.5e-6, 0.5e-6, m) if m > 1 else np.zeros(1)))
        return np.concatenate(out)
    if name == "tight":                                                    # 40 eigenvalues 1e-13 apart, midway between two of a spread-out rest
        rest = np.linspace(-1.0, 1.0, n - TIGHT_COUNT)
        m = (2 * len(rest)) // 3
        c = 0.5 * (rest[m] + rest[m + 1])
        return np.sort(np.concatenate([rest, c + TIGHT_STEP * (np.arange(TIGHT_COUNT) - TIGHT_COUNT // 2)]))
    if name == "graded":                                                   # both signs, ten decades
        m = n // 2
        return np.sort(np.concatenate([-np.logspace(-10.0, 0.0, m), 0.7 * np.logspace(-10.0, 0.0, n - m)]))
    raise KeyError(name)


def clusters_by_rule(w):
    """The cluster rule of csrc/dsygv.hip restated: neighbours closer than 1e-3 |lambda|_max, chained.  Returns [(c0, c1), ...]."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    ctol = 1e-3 * np.max(np.abs(w)) if n else 0.0
    out = []
    c0 = 0
    while c0 < n:
        c1 = c0 + 1
        while c1 < n and w[c1] - w[c1 - 1] <= ctol:
            c1 += 1
        out.append((c0, c1))
        c0 = c1
    return out


def metrics(H, S, w, Z):
    """orth = max|Z^T S Z - I|, resid = max|H Z - S Z diag(w)| / (max|w| max|S|)."""
    n = len(w)
    orth = float(np.max(np.abs(Z.T @ S @ Z - np.eye(n))))
    resid = float(np.max(np.abs(H @ Z - (S @ Z) * w)) / (np.max(np.abs(w)) * np.max(np.abs(S))))
    return orth, resid


def half_width(M):
    i, j = np.nonzero(M)
    return int(np.max(np.abs(i - j))) if len(i) else 0


def upper_bands(M, k):
    """Upper bands [k][n] of the symmetric matrix M: B[d, i] = M(i, i + d) (the layout of oracle.truth.band_eigs)."""
    n = M.shape[0]
    B = np.zeros((k, n))
    for d in range(min(k, n)):
        r = np.arange(n - d)
        B[d, r] = M[r, r + d]
    return B


# ---- the cases of tests/test_gpu_dsygv_pencils.py ------------------------------------------------------------------------------
class Case:
    def __init__(self, name, H, S, p, sizes=None, mults=None, persym=False):
        self.name, self.H, self.S, self.p = name, H, S, p
        self.n = H.shape[0]
        self.sizes = sizes          # intended cluster sizes under the rule, in ascending order of the eigenvalues
        self.mults = mults          # intended multiplicities of the exactly repeated eigenvalues (sorted), or None
        self.persym = persym


A_SIZES = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129]
B_WIDTHS = [0, 1, 7, 8, 9, 15]
E_DIAG_SIMPLE = 31


def _rule_sizes(lams):
    return [c1 - c0 for c0, c1 in clusters_by_rule(np.sort(lams))]


def _e_diag_lams():
    simple = -1.0 + np.arange(E_DIAG_SIMPLE) / 32.0                        # multiples of 1/32: exact products with the dyadic S
    return np.concatenate([simple, np.full(2, 0.25), np.full(3, 0.5), np.full(64, 0.75)])


def _build(name):
    kind, _, arg = name.partition("-")
    if kind == "A":
        n = int(arg[1:]); lams = spectrum("uniform", n); p = min(4, n - 1)
        return Case(name, *make_pencil(lams, p, 100 + n), p, _rule_sizes(lams))
    if kind == "B":
        p = int(arg[1:]); lams = spectrum("uniform", 200)
        return Case(name, *make_pencil(lams, p, 200 + p), p, _rule_sizes(lams))
    if name == "C-uniform":
        lams = spectrum("uniform", 200)
        return Case(name, *make_pencil(lams, 4, 300), 4, _rule_sizes(lams))
    if kind == "C":
        p = int(arg[1:])
        return Case(name, *make_pencil(spectrum("clusters", 600), p, 310 + p), p, cluster_sizes(600))
    if kind == "D":
        p = int(arg[1:]); lams = spectrum("tight", 300)
        return Case(name, *make_pencil(lams, p, 400 + p), p, _rule_sizes(lams))
    if name in ("E-sum2", "E-sum3"):
        m = int(name[-1]); lams = spectrum("uniform", 100)
        H, S = direct_sum([make_pencil(lams, 4, 500)] * m)
        return Case(name, H, S, 4, [m] * 100, [m] * 100)
    if name == "E-diag":
        lams = _e_diag_lams()
        return Case(name, *diagonal_pencil(lams, 510), 0, _rule_sizes(lams), [2, 3, 64])
    if name == "E-unequal":
        l1 = spectrum("uniform", 37); l2 = np.linspace(-0.9317, 0.9713, 91)
        H, S = direct_sum([make_pencil(l1, 4, 520), make_pencil(l2, 4, 521)])
        return Case(name, H, S, 4, _rule_sizes(np.concatenate([l1, l2])))
    if name == "F-deep128":
        # wells deep enough for a ladder of pair gaps from the bottom up: 2e-17, 6e-14, 8e-12, 6e-10, 3e-8 |lambda|_max, ... -- below,
        # at and above what double precision resolves; the eigenspaces of the unresolved pairs are generic (no repeated block)
        H, S = persymmetric(128, 3, 2.0)
        return Case(name, H, S, 3, None, None, True)
    if kind == "F":
        n = int(arg[1:])
        H, S = persymmetric(n, 3, 0.02)
        return Case(name, H, S, 3, None, None, True)
    if name in ("H-up", "H-down"):
        c = case("D-p4")
        return Case(name, np.ldexp(c.H, 200 if name == "H-up" else -200), c.S, 4, c.sizes)
    if name == "H-graded":
        lams = spectrum("graded", 400)
        return Case(name, *make_pencil(lams, 4, 600), 4, _rule_sizes(lams))
    raise KeyError(name)


CASE_NAMES = (["A-n%d" % n for n in A_SIZES] + ["B-p%d" % p for p in B_WIDTHS] + ["C-uniform", "C-p4", "C-p12", "D-p4", "D-p8",
              "E-sum2", "E-sum3", "E-diag", "E-unequal", "F-n255", "F-n256", "F-deep128", "H-up", "H-down", "H-graded"])


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def lapack(name):
    """LAPACK's answer (scipy.linalg.eigh: DSYGVD) on the case: w, Z."""
    import scipy.linalg
    c = case(name)
    w, Z = scipy.linalg.eigh(c.H, c.S)
    return w, Z


def truth_indices(name):
    """All indices for n <= 200; else a sample of 64 that holds both ends of every cluster of the rule and both ends of the spectrum."""
    c = case(name)
    if c.n <= 200:
        return np.arange(c.n)
    w = lapack(name)[0]
    ends = sorted({i for c0, c1 in clusters_by_rule(w) if c1 - c0 > 1 for i in (c0, c1 - 1)} | {0, c.n - 1})
    if len(ends) > 64:                                                     # many small clusters: an even sample of their ends
        ends = [ends[i] for i in np.unique(np.linspace(0, len(ends) - 1, 64).astype(int))]
    rest = np.setdiff1d(np.arange(c.n), ends)
    rng = np.random.default_rng(c.n)
    fill = rng.choice(rest, size=64 - len(ends), replace=False) if len(ends) < 64 else []
    return np.sort(np.concatenate([np.array(ends, dtype=int), np.array(fill, dtype=int)]))


@functools.lru_cache(maxsize=None)
def truth(name):
    """(idx, 113-bit eigenvalues at idx, |lambda|_max) of the ROUNDED pencil of the case: bisection on the inertia of H - x S in
    quad precision (oracle/truth_quad.c), independent of every algorithm under test and of LAPACK."""
    from oracle import truth as tq
    c = case(name)
    w = lapack(name)[0]
    lam = float(np.max(np.abs(w)))
    idx = truth_indices(name)
    k = max(c.p, 1) + 1
    hi, lo = tq.band_eigs(upper_bands(c.S, k), upper_bands(c.H, k), idx, w[idx], lam, rtol=1e-20)
    return idx, hi, lam


def gaps(w):
    """Distance of every eigenvalue to its nearest neighbour."""
    w = np.asarray(w)
    if len(w) < 2:
        return np.full(len(w), np.inf)
    d = np.diff(w)
    return np.minimum(np.concatenate([[np.inf], d]), np.concatenate([d, [np.inf]]))


def not_positive_definite(n, p, pos, seed=700):
    """A pencil whose S loses positive definiteness at leading minor pos + 1: the diagonal entry there is lowered by 1.5 times the
    square of the pivot its Cholesky factorisation would have had."""
    H, S, U, _ = make_pencil(spectrum("uniform", n), p, seed, return_factor=True)
    S = S.copy()
    S[pos, pos] -= 1.5 * U[pos, pos] ** 2
    return H, S
