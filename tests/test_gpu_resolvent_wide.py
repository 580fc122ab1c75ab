"""The coupled-channel resolvent for wide bands (bspatom_resolvent_coupled_wide / _dev, csrc/resolvent_wide.hip): backward error
against LAPACK's on the same matrix in the documented ordering from half-width 11 to the limit 255, the guarantees K1 - K4 of
include/bspatom.h bit for bit, Stark levels with 8 and 10 channels and Floquet quasi-energies with 10 and 14 blocks end to end through
host.coupled_eigenpair's default solver, the argument checks.  References, matrices and criteria are those of
test_gpu_resolvent_coupled.py (tests/resolvent_coupled_ref.py: dense NumPy, residuals in clongdouble)."""
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_coupled_ref as cref
import test_gpu_resolvent as single        # its fixtures (_input), right-hand sides (_vectors) and bit comparison (_same)
import test_gpu_resolvent_coupled as coupled   # its topology, coefficients and matrices
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
HYD10 = dict(single.HYD, l_fin=9)          # test_resolvent_cpu's grid with l = 0..9
K16_N20 = dict(single.K16, nfun=20)        # order 100 under half-width 79: the window never fills


def _problem(name):
    return capi.Problem(capi.make_input(**K16_N20) if name == "k16_n20" else single._input(name))


def _assembled(name):
    """test_gpu_resolvent_coupled._assembled with the extra grid: (problem, SB, HB[0:2], the absorber's band, the bands of r and d/dr)"""
    prob = _problem(name)
    r = prob.quadrature()[0]
    WB = prob.operator_bands(host.cap_profile(r, 0.5 * r[-1], 1e-2), [0])[0]
    RB = prob.dipole_bands()
    SB, HB = prob.assemble(0, 2)
    return prob, SB, HB, WB, np.stack([RB[0], RB[2]])


def _topology(nch):
    """test_gpu_resolvent_coupled's topology and one long-range entry between the first and the last channel"""
    return coupled._topology(nch) + [(0, nch - 1, 0)]


def _coefficients(nch, s):
    """its coefficients; the long-range entry s (0.25 + 0.1 i) on the band of r"""
    return np.concatenate([coupled._coefficients(nch, s), [[s * (0.25 + 0.1j), 0.0]]])


T1_CASES = [("n65_k4", 3, coupled.T1_MATS), ("k16_n40", 1, coupled.T1_MATS), ("n65_k4", 17, coupled.T1_MATS),
            ("k16_n20", 5, coupled.T1_MATS), ("lin256", 8, coupled.T1_MATS4), ("k16_n40", 9, coupled.T1_MATS),
            ("k16_n40", 16, coupled.T1_MATS4)]


# ---- T1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nch,mats", T1_CASES, ids=["%s-nch%d" % c[:2] for c in T1_CASES])
def test_backward_error_against_lapack(name, nch, mats):
    """test_gpu_resolvent_coupled's T1 on the wide call: omega = ||b - M x||_inf / (||M||_inf ||x||_inf + ||b||_inf) in long double
    on the matrix built from the caller-visible bands (channels l = c % 2, z + 0.01 c, its topology and coefficients, strength 1.0
    among them, plus one long-range entry (0, nch - 1)), nrhs / nproj = (1, 0) and (3, 2): omega <= 8 max(omega_ref, eps), omega_ref
    numpy.linalg.solve's on the same matrix in the documented ordering.  info == 0.  R against P^T x within (N + 2) eps sum |P| |x|.
    bw = 11 < a panel (n65_k4 nch 3), one channel (k16_n40, bw 15), bw = 67 just past the old limit (n65_k4 nch 17, N = 1105),
    N = 100 < 2 bw + 1 = 159 (k16_n20 nch 5), 128 panels in steady state (lin256 nch 8, bw 71, N = 2048), candidates over three
    waves and 2 bw + 1 = 287 no multiple of 16 (k16_n40 nch 9, bw 143), the limit bw = 255 (k16_n40 nch 16, N = 640).
    Measured on the MI355X, maximum of omega / max(omega_ref, eps) per case: n65_k4 nch 3: 0.17, k16_n40 nch 1: 0.486, n65_k4 nch 17:
    0.509, k16_n20 nch 5: 0.226, lin256 nch 8: 0.319, k16_n40 nch 9: 0.482, k16_n40 nch 16: 0.349."""
    prob, SB, HB, WB, G = _assembled(name)
    n, k = prob.nfun, prob.k
    N = nch * n
    assert nch * k - 1 <= 255
    l = [c % 2 for c in range(nch)]
    cp = _topology(nch)
    z = np.array([[zb + 0.01 * c for c in range(nch)] for zb, _, _ in mats])
    w = np.array([[wm] * nch for _, wm, _ in mats], dtype=np.int32)
    a = np.stack([_coefficients(nch, s) for _, _, s in mats])
    worst = 0.0
    dense = [(cref.dense_matrix(SB, HB, l, z[m], cp, G, a[m], WB[None], w[m]),
              cref.dense_matrix(SB, HB, l, z[m], cp, G, a[m], WB[None], w[m], np.clongdouble)) for m in range(len(mats))]
    if nch > 1:
        assert cref.half_width(dense[2 if len(mats) > 4 else 0][0], nch) <= nch * k - 1
    for nrhs, nproj in ((1, 0), (3, 2)):
        B, P = coupled._vectors(n, nch, nrhs, nproj, 7 + nrhs)
        X, R, info = prob.resolvent_coupled_wide(l, z, B, couplings=cp, G=G, a=a, W=WB, w=w, P=P)
        assert X.shape == (len(mats), nrhs, nch, n) and np.all(np.isfinite(X.view(np.float64)))
        assert np.all(info == 0), info
        assert (R is None) == (nproj == 0)
        for m, (zb, wm, s) in enumerate(mats):
            M, Ml = dense[m]
            Xref = cref.solve(M, B, nch)
            for r in range(nrhs):
                om, om_ref = cref.backward_error(Ml, X[m, r], B[r]), cref.backward_error(Ml, Xref[r], B[r])
                ratio = om / max(om_ref, EPS)
                worst = max(worst, ratio)
                print("%s nch %d m %d (z %s w %d s %g) rhs %d: omega %.3e  omega_ref %.3e  ratio %.3g" % (name, nch, m, zb, wm, s, r, om, om_ref, ratio))
                assert om <= 8.0 * max(om_ref, EPS), (name, nch, m, r, om, om_ref)
                for q in range(nproj):
                    xl, pl = X[m, r].astype(np.clongdouble).ravel(), P[q].astype(np.clongdouble).ravel()
                    bound = (N + 2) * EPS * float(np.sum(np.abs(pl) * np.abs(xl)))
                    assert abs(complex(np.sum(pl * xl)) - R[m, r, q]) <= bound, (name, nch, m, r, q)
    note("resolvent_coupled_wide %s nch %d (bw %d): max omega / max(omega_ref, eps) = %.3g" % (name, nch, nch * k - 1, worst))
    prob.close()


# ---- T2 ---------------------------------------------------------------------------------------------------------------
def test_independence_and_determinism():
    """K1, K2 bitwise on n65_k4 with nch = 17 (bw = 67): a batch of seven matrices (channels, energies, absorbers, coefficients
    mixed) with nrhs = 3, nproj = 2 against a second run, each matrix alone, the reversed order, resolvent_slots = 1 and 3,
    resolvent_stage_mb = 1, nrhs = 1 against the first of 3, nproj = 1 against the first of 2, want_x = False, and the _dev variant
    on torch tensors pre-filled with NaN."""
    prob, SB, HB, WB, G = _assembled("n65_k4")
    n, nch, nmat = prob.nfun, 17, 7
    same = single._same
    rng = np.random.default_rng(21)
    cp = _topology(nch)
    l = rng.integers(0, 2, (nmat, nch)).astype(np.int32)
    z = rng.uniform(-0.6, 2.0, (nmat, nch)) + 1j * rng.choice([0.0, 0.05, -0.05, 0.3], (nmat, nch))
    w = rng.integers(-1, 2, (nmat, nch)).astype(np.int32)
    w[z.imag == 0.0] = 0                                       # a real energy keeps its absorber
    a = rng.choice([0.0, 1e-2, 1.0], (nmat, 1, 1)) * (rng.standard_normal((nmat, len(cp), 2)) + 1j * rng.standard_normal((nmat, len(cp), 2)))
    W2 = np.stack([WB, 0.5 * WB])
    B, P = coupled._vectors(n, nch, 3, 2, 5)
    kw = dict(couplings=cp, G=G, W=W2)
    X, R, info = prob.resolvent_coupled_wide(l, z, B, a=a, w=w, P=P, **kw)
    assert np.all(info == 0) and np.all(np.isfinite(X.view(np.float64))) and np.max(np.abs(X)) > 0
    X2, R2, _ = prob.resolvent_coupled_wide(l, z, B, a=a, w=w, P=P, **kw)
    assert same(X2, X) and same(R2, R)                         # two runs
    for m in range(nmat):                                      # each matrix alone
        Xm, Rm, _ = prob.resolvent_coupled_wide(l[m], z[m], B, a=a[m], w=w[m], P=P, **kw)
        assert same(Xm[0], X[m]) and same(Rm[0], R[m]), m
    Xr, Rr, _ = prob.resolvent_coupled_wide(l[::-1], z[::-1], B, a=a[::-1], w=w[::-1], P=P, **kw)
    assert same(Xr[::-1], X) and same(Rr[::-1], R)             # the reversed order
    for opt, val in (("resolvent_slots", 1), ("resolvent_slots", 3), ("resolvent_stage_mb", 1)):
        capi.set_option(opt, val)
        try:
            Xo, Ro, _ = prob.resolvent_coupled_wide(l, z, B, a=a, w=w, P=P, **kw)
        finally:
            capi.set_option(opt, 0)
        assert same(Xo, X) and same(Ro, R), (opt, val)
    X1, R1, _ = prob.resolvent_coupled_wide(l, z, B[0], a=a, w=w, P=P[0], **kw)   # nrhs = 1, nproj = 1
    assert same(X1[:, 0], X[:, 0]) and same(R1[:, 0, 0], R[:, 0, 0])
    Xq, Rq, _ = prob.resolvent_coupled_wide(l, z, B, a=a, w=w, P=P, want_x=False, **kw)
    assert Xq is None and same(Rq, R)
    # the _dev variant on torch tensors, outputs pre-filled with NaN
    dev = "cuda:0"
    Bd, Pd, Wd, Gd = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (B, P, W2, G))
    Xd = torch.full((nmat, 3, nch, n), float("nan"), dtype=torch.complex128, device=dev)
    Rd = torch.full((nmat, 3, 2), float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.resolvent_coupled_wide_dev(l, z, 3, Bd.data_ptr(), couplings=cp, nop=2, G_ptr=Gd.data_ptr(), a=a, nabs=2,
                                            W_ptr=Wd.data_ptr(), w=w, nproj=2, P_ptr=Pd.data_ptr(), X_ptr=Xd.data_ptr(), R_ptr=Rd.data_ptr())
    assert np.all(infod == 0)
    assert same(Xd.cpu().numpy(), X) and same(Rd.cpu().numpy(), R)
    prob.close()


# ---- T3 ---------------------------------------------------------------------------------------------------------------
def test_real_problem_stays_real_and_eigenvalue_is_survived():
    """K3: every Im z = 0, no absorber, real coefficients, real B: every imaginary part of X (and of R with real P) is +-0.0, on
    n65_k4 with nch = 17 (bw 67) and k16_n40 with nch = 9 (bw 143), at coupling strengths 1e-2 and 1.0: the imaginary accumulators of
    the matrix cores only sum products with a zero factor.  z exactly on computed eigenvalues of uncoupled blocks: the result is
    finite and info >= 0."""
    for name, nch in (("n65_k4", 17), ("k16_n40", 9)):
        prob, SB, HB, WB, G = _assembled(name)
        B = np.random.default_rng(3).standard_normal((2, nch, prob.nfun))
        l = [c % 2 for c in range(nch)]
        z = np.array([[0.3 + 0.01 * c for c in range(nch)], [-1.0 + 0.2 * c for c in range(nch)]])
        a = np.stack([_coefficients(nch, 1e-2).real, _coefficients(nch, 1.0).real])
        X, R, info = prob.resolvent_coupled_wide(l, z, B, couplings=_topology(nch), G=G, a=a, P=B)
        assert np.all(info == 0) and np.max(np.abs(X.real)) > 0
        assert np.all(X.imag == 0.0) and np.all(R.imag == 0.0), name
        prob.close()
    prob = capi.Problem(single._input("n65_k4"))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    nch = 17
    B = np.random.default_rng(4).standard_normal((1, nch, prob.nfun))
    l = [c % 2 for c in range(nch)]
    z = np.array([[0.2 + 0.01 * c for c in range(nch)]] * 3)
    z[0, 0], z[1, 0], z[1, 1], z[2, 16], z[2, 5] = E[0, 0], E[0, 7], E[1, 3], E[0, 64], E[1, 10]
    X, R, info = prob.resolvent_coupled_wide(l, z, B)
    print("on eigenvalues: info", info, "max |x|", np.max(np.abs(X), axis=(1, 2, 3)))
    assert np.all(np.isfinite(X.view(np.float64))) and np.all(info >= 0)
    prob.close()


# ---- T4 ---------------------------------------------------------------------------------------------------------------
def test_transposed_entry_equals_transposed_band():
    """K4 bitwise on n65_k4 with nch = 17, with the band of d/dr, which is not symmetric: the call whose second directions are
    (c+1, c, ctr = 1) on D against the same call with those directions as (c+1, c, ctr = 0) on host.band_transpose(D)."""
    prob, SB, HB, WB, G = _assembled("n65_k4")
    n, nch = prob.nfun, 17
    D = G[1]
    DT = host.band_transpose(D)
    assert not np.array_equal(D, DT)
    G2 = np.stack([D, DT])
    B, P = coupled._vectors(n, nch, 2, 1, 9)
    l = [c % 2 for c in range(nch)]
    z = np.array([[0.3 + 0.01 * c + (0.05j if c % 3 == 1 else 0.0) for c in range(nch)],
                  [0.5 - 0.04 * c - (0.05j if c % 4 == 0 else 0.0) for c in range(nch)]])
    w = np.array([[0 if c % 3 != 1 else -1 for c in range(nch)], [0 if c % 4 != 0 else -1 for c in range(nch)]], dtype=np.int32)
    cp1 = [e for c in range(nch - 1) for e in ((c, c + 1, 0), (c + 1, c, 1))]
    cp0 = [(cr, cc, 0) for cr, cc, _ in cp1]
    s = np.array([(0.7, 0.7, -0.4 + 0.2j, -0.4 - 0.2j)[q % 4] for q in range(len(cp1))])
    a1 = np.zeros((len(cp1), 2), dtype=np.complex128); a1[:, 0] = s          # every entry on D, the second directions transposed
    a0 = np.zeros((len(cp1), 2), dtype=np.complex128); a0[0::2, 0] = s[0::2]; a0[1::2, 1] = s[1::2]   # the second directions on D^T
    X1, R1, i1 = prob.resolvent_coupled_wide(l, z, B, couplings=cp1, G=G2, a=a1, W=WB, w=w, P=P)
    X0, R0, i0 = prob.resolvent_coupled_wide(l, z, B, couplings=cp0, G=G2, a=a0, W=WB, w=w, P=P)
    assert np.all(i1 == 0) and np.all(i0 == 0) and np.max(np.abs(X1)) > 0
    assert single._same(X1, X0) and single._same(R1, R0)
    prob.close()


# ---- T5 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hydrogen10():
    """test_resolvent_cpu's hydrogen grid with l = 0..9: the problem with its bands held, E_1s, c_1s, the band of r, (SB, HB)"""
    prob = capi.Problem(capi.make_input(**HYD10))
    E, sinfo = prob.solve(0, 10)
    assert np.all(sinfo == 0)
    c1s = prob.eigvecs(0, 1, 1)[0]
    R_r = prob.dipole_bands()[0]
    SB, HB = prob.assemble(0, 10)
    yield dict(prob=prob, E1s=E[0, 0], c1s=c1s, R_r=R_r, SB=SB, HB=HB, n=prob.nfun, k=prob.k)
    prob.close()


@pytest.mark.parametrize("nl", [8, 10])
def test_stark_level_end_to_end(hydrogen10, nl):
    """Stark, l = 0..7 (bw 71) and l = 0..9 (bw 89): host.coupled_eigenpair with its DEFAULT solver (the wide call: bw > 63) at
    F = 0.005 and 0.01, shift -0.5, from (c_1s, 0, ..), against E_1s - (9/4) F^2 - (3555/64) F^4 - (2512779/512) F^6 within 1e-9,
    |Im lambda| <= 1e-15: the bounds of the 4-channel test (CPU dense deviations -3.1e-13 and -8.1e-11 for both channel counts)."""
    h = hydrogen10
    chans = [(l, 0) for l in range(nl)]
    assert nl * h["k"] - 1 > host.COUPLED_MAX_BAND
    for F in (0.005, 0.01):
        cp, a = host.stark_system(chans, F)
        x0 = np.zeros((nl, h["n"])); x0[0] = h["c1s"]
        lam, x, hist = host.coupled_eigenpair(h["prob"], list(range(nl)), cp, h["R_r"], a, -0.5, x0, iters=3)
        want = cref.stark_series(h["E1s"], F)
        print("Stark l = 0..%d F %.3f: lambda %.15f %+.1e i  series %.15f  deviation %.2e  last step %.1e"
              % (nl - 1, F, lam.real, lam.imag, want, lam.real - want, abs(hist[2] - hist[1])))
        assert abs(lam.real - want) <= 1e-9 and abs(lam.imag) <= 1e-15, F


@pytest.mark.parametrize("nphot,nblk", [(2, 10), (3, 14)])
def test_floquet_quasi_energy_end_to_end(hydrogen10, nphot, nblk):
    """Floquet, l = 0..3, omega = 0.2, F = 0.005, two photons either side (10 blocks, bw 89) and three (14 blocks, bw 125): lambda
    of coupled_eigenpair through the wide call against lambda of coupled_eigenpair(solver = dense) on resolvent_coupled_ref's dense
    matrix of the problem's own bands, within 1e-13, the bar of the CPU tests on this iteration (two dense orderings and entrywise
    8 eps perturbations differ by at most 5.6e-16; CPU values -0.5000370831994085 and -0.5000370799559866)."""
    h = hydrogen10
    blocks, zoff, cp, a = host.floquet_system([(0, 0), (1, 0), (2, 0), (3, 0)], nphot, 0.2, 0.005)
    assert len(blocks) == nblk
    l = [b[0][0] for b in blocks]
    x0 = np.zeros((nblk, h["n"])); x0[blocks.index(((0, 0), 0))] = h["c1s"]
    lam, _, hist = host.coupled_eigenpair(h["prob"], l, cp, h["R_r"], a, -0.5, x0, zoff=zoff, iters=3)

    def dense(l_, z_, B_):
        M = cref.dense_matrix(h["SB"], h["HB"], list(l_), z_, cp, h["R_r"][None], a)
        return cref.solve(M, B_[None], len(l_))[0]
    lam_ref, _, _ = host.coupled_eigenpair(h["prob"], l, cp, h["R_r"], a, -0.5, x0, zoff=zoff, iters=3, solver=dense)
    print("Floquet nphot %d (%d blocks): lambda %.16f %+.1e i  dense %.16f %+.1e i  difference %.2e"
          % (nphot, nblk, lam.real, lam.imag, lam_ref.real, lam_ref.imag, abs(lam - lam_ref)))
    assert abs(lam - lam_ref) <= 1e-13


# ---- T6 ---------------------------------------------------------------------------------------------------------------
def test_resolvent_coupled_wide_argument_checks():
    """test_gpu_resolvent_coupled's list on both wide variants; k = 16 with 17 channels (bw 271) is beyond the limit (bw = 255 itself
    passes in test_backward_error_against_lapack)"""
    prob = capi.Problem(single._input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: np.array(v, dtype=np.int32)
    nch = 2
    l, z, w = i32([0, 1, 1, 0]), np.array([0.3, 0.05, 0.1, -0.05, 0.2, 0.0, 0.4, 0.1]), i32([-1, 0, 0, -1])
    cr, cc, ctr = i32([0, 1]), i32([1, 0]), i32([0, 1])
    WB, GB, a = np.zeros((2 * k - 1) * n), np.ones((2 * k - 1) * n), np.array([0.1, 0.0, 0.1, 0.0] * 2)
    B, P = np.ones(2 * nch * n), np.ones(2 * nch * n)
    X, R, info = np.zeros(2 * 2 * nch * n), np.zeros(2 * 2), np.zeros(2, dtype=np.int32)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    WBd, GBd, Bd, Pd, Xd, Rd = dv(WB), dv(GB), dv(B), dv(P), dv(X), dv(R)
    dp = lambda t: C.c_void_p(t.data_ptr())
    variants = ((L.bspatom_resolvent_coupled_wide, p_(WB), p_(GB), p_(B), p_(P), p_(X), p_(R)),
                (L.bspatom_resolvent_coupled_wide_dev, dp(WBd), dp(GBd), dp(Bd), dp(Pd), dp(Xd), dp(Rd)))
    # 0 p, 1 nmat, 2 nch, 3 l, 4 z, 5 nabs, 6 WB, 7 w, 8 ncoup, 9 cr, 10 cc, 11 ctr, 12 nop, 13 GB, 14 a, 15 nrhs, 16 B, 17 nproj, 18 P, 19 X, 20 R, 21 info
    args = lambda wb, gb, b, pp, x, r: [prob._h, 2, nch, p_(l), p_(z), 1, wb, p_(w), 2, p_(cr), p_(cc), p_(ctr), 1, gb, p_(a), 1, b, 1, pp, x, r, p_(info)]
    for fn, *ptrs in variants:                                 # before any solve or assemble: no channel is there
        assert fn(*args(*ptrs)) == -2
    prob.assemble(0, 2)
    for fn, *ptrs in variants:
        good = args(*ptrs)
        sub = lambda pos, v: [v if i == pos else g for i, g in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 4, 16, 21):                          # p, l, z, B, info
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(6, None)) == -2                         # nabs = 1 without WB
        assert fn(*sub(18, None)) == -2                        # R without P
        assert fn(*sub(17, 0)) == -2                           # R with nproj = 0
        assert fn(*[None if i in (19, 20) else g for i, g in enumerate(good)]) == -2        # neither X nor R
        assert fn(*sub(19, None)) == 0 and fn(*sub(20, None)) == 0                          # one of them is enough
        assert fn(*[None if i in (18, 20) else g for i, g in enumerate(good)]) == 0         # P may be NULL when R is
        for pos in (1, 2, 15):                                 # nmat, nch, nrhs below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(5, -1)) == -2                           # nabs < 0
        assert fn(*sub(8, -1)) == -2                           # ncoup < 0
        for bad in ([0, 2, 1, 0], [0, 1, -1, 0]):              # a channel outside the bands held, per (m, c)
            assert fn(*sub(3, p_(i32(bad)))) == -2, bad
        for bad in ([-2, 0, 0, -1], [-1, 0, 0, 1]):            # w outside -1 .. nabs-1, per (m, c)
            assert fn(*sub(7, p_(i32(bad)))) == -2, bad
        assert fn(*[0 if i == 5 else (None if i == 6 else g) for i, g in enumerate(good)]) == -2   # w = 0 with no absorber at all
        assert fn(*sub(7, None)) == 0                          # w NULL: absorber 0 everywhere
        for pos, bad in ((9, [0, 2]), (9, [-1, 1]), (10, [2, 0]), (10, [1, -1]), (11, [0, 2]), (11, [-1, 1])):
            assert fn(*sub(pos, p_(i32(bad)))) == -2, (pos, bad)                            # a channel index / ctr out of range
        for pos in (9, 10, 11, 13, 14):                        # ncoup > 0 with cr, cc, ctr, GB or a NULL
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(12, 0)) == -2                           # ncoup > 0 with nop < 1
        assert fn(*[0 if i in (8, 12) else (None if i in (9, 10, 11, 13, 14) else g) for i, g in enumerate(good)]) == 0   # ncoup = 0 needs neither
        assert fn(*good) == 0                                  # a valid call afterwards
    prob.close()
    # the limit: bw = nch k - 1 <= 255.  k = 16 with 17 channels is bw = 271
    prob = capi.Problem(single._input("k16_n40"))
    prob.assemble(0, 2)
    with pytest.raises(capi.BspAtomError) as ei:
        prob.resolvent_coupled_wide([c % 2 for c in range(17)], 0.3 + 0.1j, np.ones((17, prob.nfun)))
    assert ei.value.code == -5
    prob.close()
