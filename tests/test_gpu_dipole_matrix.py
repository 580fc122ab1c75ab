"""Dipole matrix blocks between eigenvector windows of many channel pairs in one call (bspatom_dipole_matrix / _dev,
csrc/dipole.hip): against the per-state bspatom_dipole_elements, against the compiled reference's TRANS_AMP, reciprocity,
independence of the batch and of the grouping, the device variant, the argument checks, the K slicing at n = 4096, and the
wall time against the loop of per-state calls it replaces.

The bound.  Both paths evaluate z^T A x in floating point, each with its own summation order, from the same z, A and x, so
    |D_block - D_elements| <= 2 (n + 2k + 4) eps sum_i |z_i| (|A| |x|)_i,   |A| = |a0| |R_r| + |a1| |R_1/r| + |a2| |R_d/dr|
(n + 2k + 4 roundings at most per path: 2k - 1 products and sums of a row of A x and the three of an entry of A, n of the dot
product).  The right-hand side is computed on the host from prob.eigvecs and prob.dipole_bands()."""
import time
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from conftest import load_golden
from test_gpu_stages import input_from_case, note

from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def abs_apply(RB, a, X):
    """(|A| |x_j|) for the rows x_j of X (m, n): |A| = sum_c |a_c| |RB[c]|, RB[c][d + k - 1][i] = R_c(i, i + d)"""
    k, n = (RB.shape[1] + 1) // 2, RB.shape[2]
    absA = sum(abs(a[c]) * np.abs(RB[c]) for c in range(3))
    Y = np.zeros_like(X)
    for d in range(-(k - 1), k):
        lo, hi = max(0, -d), min(n, n - d)                     # rows i with 0 <= i + d < n
        Y[:, lo:hi] += absA[d + k - 1, lo:hi] * np.abs(X[:, lo + d:hi + d])
    return Y


class Bounds:
    """the bound of a (pair, windows, a) block, eigenvector blocks cached per (channel, window)"""

    def __init__(self, prob):
        self.prob, self.RB, self.Z = prob, prob.dipole_bands(), {}

    def vecs(self, l, n0, count):
        key = (l, n0, count)
        if key not in self.Z:
            self.Z[key] = self.prob.eigvecs(l, n0, count)
        return self.Z[key]

    def sums(self, li, lf, n0_ini, ci, n0_fin, cf, a):
        """S[i, f] = sum_r |z_f(r)| (|A| |x_i|)(r)"""
        return abs_apply(self.RB, a, self.vecs(li, n0_ini, ci)) @ np.abs(self.vecs(lf, n0_fin, cf)).T

    def bound(self, *args):
        return 2.0 * (self.prob.nfun + 2 * self.prob.k + 4) * EPS * self.sums(*args)


def elements_block(prob, li, lf, n0_ini, ci, n0_fin, cf, a, rows=None):
    rows = range(ci) if rows is None else rows
    return np.stack([prob.dipole_elements(li, n0_ini + i, lf, n0_fin, cf, a) for i in rows])


def check_block(tag, D, R, B):
    ratio = float(np.max(np.abs(D - R) / np.maximum(B, np.finfo(float).tiny)))
    note("dipole_matrix %s: max |D - elements| / bound = %.3g (max|D| %.3g)" % (tag, ratio, np.max(np.abs(R))))
    assert np.all(np.abs(D - R) <= B), (tag, ratio)


def _solved(name, nl=None, **over):
    prob = capi.Problem(input_from_case(name, **over))
    nl = prob.lmax + 1 if nl is None else nl
    E, info = prob.solve(0, nl)
    assert np.all(info == 0)
    return prob


@pytest.fixture(scope="module")
def lin256():
    prob = _solved("lin256")
    assert prob.lmax == 3
    yield prob, Bounds(prob)
    prob.close()


@pytest.fixture(scope="module")
def lin1024():
    prob = _solved("lin1024", 2)
    yield prob, Bounds(prob)
    prob.close()


# ---- 1 ----------------------------------------------------------------------------------------------------------------
GAUGES = {"length": np.array([0.75, 0.0, 0.0]), "velocity": np.array([0.0, 2.0, -1.0])}
PAIRS = [(0, 1), (1, 0), (1, 1), (0, 1)]


@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "c1_lin", "lin256", "c5_1024_k11"])
def test_dipole_matrix_vs_per_state_call(name):
    """Pairs (0,1), (1,0), (1,1) and (0,1) again, both gauges (the pairs' coefficients differ by a factor, the repeated pair
    has the first one's); count_ini = 1 and 17 (at most nfun), count_fin = min(37, nfun - 1) rounded down to odd from
    state 2; then both windows ending at nfun.  Every element within the bound of dipole_elements; the repeated pair
    bit-identical to its first occurrence.  c5_1024_k11: k = 11 (the EB_MAX eigenvector instance, a wider band, several K
    slices); tiny8, n65_k4: n below one K tile, odd n (8-byte staging loads)."""
    prob = _solved(name, 2)
    n, bd = prob.nfun, Bounds(prob)
    cf = min(37, n - 1)
    cf = cf if cf % 2 else cf - 1
    for gname, g in GAUGES.items():
        a = np.stack([g, 1.25 * g, 1.5 * g, g])
        for ci in (1, min(17, n)):
            for n0_ini, n0_fin in ((1, 2), (n - ci + 1, n - cf + 1)):
                D = prob.dipole_matrix(PAIRS, n0_ini, ci, n0_fin, cf, a)
                assert D.shape == (4, ci, cf)
                for p in range(3):
                    li, lf = PAIRS[p]
                    R = elements_block(prob, li, lf, n0_ini, ci, n0_fin, cf, a[p])
                    check_block("%s %s pair %s ci %d n0 %d/%d" % (name, gname, PAIRS[p], ci, n0_ini, n0_fin), D[p], R,
                                bd.bound(li, lf, n0_ini, ci, n0_fin, cf, a[p]))
                assert np.array_equal(D[3], D[0])
    prob.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ta_len_s", "ta_vel_s", "ta_len_p", "ta_vel_p"])
def test_dipole_matrix_vs_compiled_reference(name):
    """D_ref[f] = ci_fin[:, f] . (c1 r1 + c2 r2) . ci_ini from the compiled reference's vectors and matrices (the DGEMV + DDOT
    of TRANS_AMP), coefficients of host.trans_amp, the reference's vector signs mapped to this library's convention as in
    test_transition_amplitudes_vs_reference.  A block of three initial states that contains n0_ini: its n0_ini row agrees to
    that test's bars, 1e-10 of max|D| on linear grids, 3e-7 with KIND_GRID=1."""
    import math
    g = load_golden(name)
    nfun, kp, n0i, l0, m0, lf, mf, mph, n0f, n1f = (int(v) for v in g["head"])
    t3a = host.three_j(lf, 1, l0, -mf, mph, m0)
    if kp == 1:
        t3b = host.three_j(lf, 1, l0, 0, 0, 0)
        c1, c2 = (-1.0) ** (lf + l0 + mf) * math.sqrt(float((2 * lf + 1) * (2 * l0 + 1))) * t3a * t3b, 0.0
        a = [c1, 0.0, 0.0]
    else:
        c1, c2 = (float(l0 + 1), -1.0) if lf == l0 + 1 else (float(l0), 1.0)
        a = [0.0, c1, c2]
    Dref = g["ci_fin"].T @ ((c1 * g["r1"] + c2 * g["r2"]) @ g["ci_ini"])

    def conv_sign(c):                        # eigvec.hip: first coefficient above 1e-8 of the largest one is positive
        big = np.where(np.abs(c) > 1e-8 * np.max(np.abs(c)))[0]
        return 1.0 if (len(big) == 0 or c[big[0]] > 0) else -1.0
    si = conv_sign(g["ci_ini"])
    Dref = np.array([Dref[i] * si * conv_sign(g["ci_fin"][:, i]) for i in range(n1f - n0f + 1)])
    prob = capi.Problem(host.input_from_namelist(str(g["namelist"])))
    assert prob.nfun == nfun
    E, info = prob.solve(0, prob.lmax + 1)
    assert np.all(info == 0)
    n0_blk = max(1, min(n0i - 1, nfun - 2))
    D = prob.dipole_matrix([(l0, lf)], n0_blk, 3, n0f, n1f - n0f + 1, a)
    prob.close()
    err = np.max(np.abs(D[0, n0i - n0_blk] - Dref)) / np.max(np.abs(Dref))
    note("dipole_matrix %s vs compiled reference: max|D| %.4g err %.2e" % (name, np.max(np.abs(Dref)), err))
    assert err <= (3e-7 if "KIND_GRID=1" in str(g["namelist"]) else 1e-10), err


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_dipole_matrix_length_gauge_reciprocity(lin256):
    """D(l -> l+1)[i, f] against D(l+1 -> l)[f, i] with equal windows (one eigenvector block per channel serves both roles):
    within the bound plus 4 eps of the same sum -- R_r is symmetric only up to rounding."""
    prob, bd = lin256
    a, n0, cnt = [1.0, 0.0, 0.0], 3, 45
    for l in range(3):
        D = prob.dipole_matrix([(l, l + 1), (l + 1, l)], n0, cnt, n0, cnt, a)
        S = bd.sums(l, l + 1, n0, cnt, n0, cnt, a)
        B = (2.0 * (prob.nfun + 2 * prob.k + 4) + 4.0) * EPS * S
        diff = np.abs(D[0] - D[1].T)
        note("dipole_matrix reciprocity lin256 l = %d: max diff / bound = %.3g" % (l, np.max(diff / B)))
        assert np.all(diff <= B), l
        assert np.max(np.abs(D[0])) > 0.1


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def _independence(prob, pairs, n0_ini, ci, n0_fin, cf, a):
    D = prob.dipole_matrix(pairs, n0_ini, ci, n0_fin, cf, a)
    assert np.array_equal(D, prob.dipole_matrix(pairs, n0_ini, ci, n0_fin, cf, a))          # run to run
    alone = [prob.dipole_matrix([pairs[p]], n0_ini, ci, n0_fin, cf, a[p])[0] for p in range(len(pairs))]
    for p in range(len(pairs)):
        assert np.array_equal(alone[p], D[p]), p
    capi.set_option("dipole_stage_mb", 1)                # several groups: two pairs of these sizes do not fit into 1 MiB
    try:
        Dg = prob.dipole_matrix(pairs, n0_ini, ci, n0_fin, cf, a)
        Dd = torch.full(D.shape, float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        prob.dipole_matrix_dev(pairs, n0_ini, ci, n0_fin, cf, a, Dd.data_ptr())
    finally:
        capi.set_option("dipole_stage_mb", 0)
    assert np.array_equal(Dg, D)
    assert np.array_equal(Dd.cpu().numpy(), D)
    assert np.max(np.abs(D)) > 0 and np.all(np.isfinite(D))


def test_dipole_matrix_independent_of_batch_and_grouping(lin256, lin1024):
    """lin256, seven pairs (channels repeated in both roles, l_ini = l_fin among them, windows of 101 and 120 states): the same
    call twice is bit-identical; every pair called alone equals its block of the joint call bit for bit; so does the joint call
    cut into several groups by dipole_stage_mb = 1, host and device variants.  Then three pairs at n = 1024, where the product
    runs in four K slices (the partials of several groups)."""
    prob, _ = lin256
    pairs = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2), (2, 2)]
    rng = np.random.default_rng(7)
    a = rng.standard_normal((7, 3))
    a[2, 1:] = 0.0
    _independence(prob, pairs, 2, 101, 5, 120, a)
    prob, _ = lin1024
    _independence(prob, [(0, 1), (1, 0), (1, 1)], 3, 40, 2, 33, rng.standard_normal((3, 3)))


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_dipole_matrix_dev_equals_host_variant(lin256):
    prob, _ = lin256
    pairs, a = [(0, 1), (1, 2), (3, 2)], np.array([[1.0, 0.0, 0.0], [0.0, 2.0, -1.0], [0.5, 1.0, 1.0]])
    Dh = prob.dipole_matrix(pairs, 1, 33, 4, 70, a)
    Dd = torch.full((3, 33, 70), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    prob.dipole_matrix_dev(pairs, 1, 33, 4, 70, a, Dd.data_ptr())
    out = Dd.cpu().numpy()
    assert not np.any(np.isnan(out))
    assert np.array_equal(out, Dh)
    # one triple is broadcast to every pair
    assert np.array_equal(prob.dipole_matrix(pairs, 1, 33, 4, 70, a[1]), prob.dipole_matrix(pairs, 1, 33, 4, 70, np.tile(a[1], (3, 1))))


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_dipole_matrix_argument_checks():
    prob = _solved("c1_lin")
    nch, n = prob.lmax + 1, prob.nfun
    Dd = torch.zeros(4 * n, dtype=torch.float64, device="cuda:0")
    a = [1.0, 0.0, 0.0]
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
        aa = np.zeros((0, 3)) if not args[0] else a
        with pytest.raises(capi.BspAtomError) as ei:
            prob.dipole_matrix(*args, aa)
        assert ei.value.code == -2, args
        with pytest.raises(capi.BspAtomError) as ei:
            prob.dipole_matrix_dev(*args, aa, Dd.data_ptr())
        assert ei.value.code == -2, args
    # null pointers
    L = capi.lib()
    li, lf = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    av, D = np.array(a), np.zeros(1)
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    for fn, out in ((L.bspatom_dipole_matrix, p_(D)), (L.bspatom_dipole_matrix_dev, C.c_void_p(Dd.data_ptr()))):
        assert fn(prob._h, 1, p_(li), p_(lf), 1, 1, 1, 1, p_(av), out) == 0
        assert fn(None, 1, p_(li), p_(lf), 1, 1, 1, 1, p_(av), out) == -2
        assert fn(prob._h, 1, None, p_(lf), 1, 1, 1, 1, p_(av), out) == -2
        assert fn(prob._h, 1, p_(li), None, 1, 1, 1, 1, p_(av), out) == -2
        assert fn(prob._h, 1, p_(li), p_(lf), 1, 1, 1, 1, None, out) == -2
        assert fn(prob._h, 1, p_(li), p_(lf), 1, 1, 1, 1, p_(av), None) == -2
    prob.dipole_matrix([(0, 1)], 1, 2, 1, 2, a)                     # valid
    prob.assemble(0, nch)                                         # invalidates the state of the last solve
    for call in (lambda: prob.dipole_matrix([(0, 1)], 1, 1, 1, 1, a),
                 lambda: prob.dipole_matrix_dev([(0, 1)], 1, 1, 1, 1, a, Dd.data_ptr())):
        with pytest.raises(capi.BspAtomError) as ei:
            call()
        assert ei.value.code == -2
    prob.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_dipole_matrix_k_slicing_at_c4_size():
    """c4_4096, channels 0 .. 1 (n = 4096), states 1 .. 256 on both sides, one pair (16 output tiles, four K slices of 1024):
    the first, middle and last row within the bound of dipole_elements."""
    prob = _solved("c4_4096", 2)
    assert prob.nfun == 4096
    a, cnt, rows = [0.0, 1.0, -1.0], 256, [0, 128, 255]
    D = prob.dipole_matrix([(0, 1)], 1, cnt, 1, cnt, a)
    R = elements_block(prob, 0, 1, 1, cnt, 1, cnt, a, rows=rows)
    bd = Bounds(prob)
    X = bd.vecs(0, 1, cnt)[rows]
    B = 2.0 * (prob.nfun + 2 * prob.k + 4) * EPS * (abs_apply(bd.RB, a, X) @ np.abs(bd.vecs(1, 1, cnt)).T)
    check_block("c4_4096 256 x 256 rows %s" % rows, D[0][rows], R, B)
    prob.close()


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_dipole_matrix_faster_than_the_loop_it_replaces(lin1024):
    """lin1024, one pair, 64 x 64 states: one dipole_matrix call against the 64 dipole_elements calls, both after a warm-up
    call.  By operation count the loop runs 64 x 65 inverse iterations and the call 128, so no finer bar than 'less wall
    time' is set; the ratio is logged."""
    prob, bd = lin1024
    a, cnt = [1.0, 0.0, 0.0], 64
    prob.dipole_matrix([(0, 1)], 1, cnt, 1, cnt, a)
    prob.dipole_elements(0, 1, 1, 1, cnt, a)
    t0 = time.perf_counter()
    D = prob.dipole_matrix([(0, 1)], 1, cnt, 1, cnt, a)
    t_call = time.perf_counter() - t0
    t0 = time.perf_counter()
    R = elements_block(prob, 0, 1, 1, cnt, 1, cnt, a)
    t_loop = time.perf_counter() - t0
    check_block("lin1024 64 x 64", D[0], R, bd.bound(0, 1, 1, cnt, 1, cnt, a))
    note("dipole_matrix lin1024 64 x 64 states, one pair: one call %.2f ms, 64 dipole_elements calls %.2f ms, x%.1f"
         % (1e3 * t_call, 1e3 * t_loop, t_loop / t_call))
    assert t_call < t_loop, (t_call, t_loop)
