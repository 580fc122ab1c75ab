"""Resolvent solves on the banded pencil (bspatom_resolvent / _dev, csrc/resolvent.hip): backward error against LAPACK's on the same
system, the guarantees G1 - G3 of include/bspatom.h bit for bit, the spectral identity, the host helpers end to end, the argument
checks.  The reference is tests/resolvent_ref.py (dense NumPy, residuals in clongdouble); every matrix is rebuilt from the bands a
caller sees (Problem.assemble, Problem.operator_bands)."""
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import pivot_designs
import resolvent_ref as ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps

K16 = dict(kind_grid=0, ra=0.0, rb=20.0, k=16, nfun=40, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)
HYD = dict(kind_grid=0, ra=0.0, rb=40.0, k=9, nfun=96, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)      # test_resolvent_cpu's grid


def _input(name):
    if name == "k16_n40":
        return capi.make_input(**K16)
    if name == "k10_n65":
        return capi.make_input(**pivot_designs.GRIDS[name])
    if name == "c5_k11_n130":
        return input_from_case("c5_1024_k11", nfun=130)
    return input_from_case(name)


def _assembled(name):
    """(problem, SB, HB[0:2], the absorber's band): bands only, no solve"""
    prob = capi.Problem(_input(name))
    r = prob.quadrature()[0]
    WB = prob.operator_bands(host.cap_profile(r, 0.5 * r[-1], 1e-2), [0])[0]
    SB, HB = prob.assemble(0, 2)
    return prob, SB, HB, WB


def _vectors(n, nrhs, nproj, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))
    B[0] = B[0].real                                           # one real right-hand side
    P = rng.standard_normal((nproj, n)) + 1j * rng.standard_normal((nproj, n)) if nproj else None
    return B, P


# the 12 matrices of T1: l = 0, 1; z real inside the spectrum (no absorber: the pivot search really swaps rows), Im z = +-0.05;
# absorber off and on
T1_MATS = [(l, z, w) for l in (0, 1) for z in (0.3, 0.3 + 0.05j, 0.3 - 0.05j) for w in (-1, 0)]


# ---- T1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "lin256", "c5_k11_n130", "k16_n40"])
def test_backward_error_against_lapack(name):
    """omega = ||b - M x||_inf / (||M||_inf ||x||_inf + ||b||_inf) in long double from the caller-visible bands, for 12 matrices
    (T1_MATS), nrhs = 1 and 3, nproj = 0 and 2: omega <= 8 max(omega_ref, eps), omega_ref numpy.linalg.solve's on the same system
    (both are LU with partial pivoting of one matrix: the growth is shared, the complex product and reciprocal forms differ by a
    few ulp per operation).  info == 0.  R against P^T x from the returned X (in long double) within (n + 2) eps sum |P_i| |x_i|.
    n < 2b + 1 (tiny8), b = 3 with n no multiple of the prefetch block (n65_k4), b = 8 (lin256), b = 10 and b = 15 on the
    BT = 15 instance.  Measured on the MI355X, maximum of omega / max(omega_ref, eps) per case: tiny8 0.273, n65_k4 0.409, lin256
    0.103, c5_k11_n130 0.289, k16_n40 0.0459 (both omegas lie below eps: 1e-18 .. 1e-16; the ratio is omega / eps)."""
    prob, SB, HB, WB = _assembled(name)
    n = prob.nfun
    l = [m[0] for m in T1_MATS]; z = [m[1] for m in T1_MATS]; w = [m[2] for m in T1_MATS]
    worst = 0.0
    for nrhs, nproj in ((1, 0), (3, 2)):
        B, P = _vectors(n, nrhs, nproj, 7 + nrhs)
        X, R, info = prob.resolvent(l, z, B, W=WB, w=w, P=P)
        assert X.shape == (12, nrhs, n) and np.all(np.isfinite(X.view(np.float64)))
        assert np.all(info == 0), info
        assert (R is None) == (nproj == 0)
        for m, (lm, zm, wm) in enumerate(T1_MATS):
            Wm = WB if wm == 0 else None
            Xref = ref.solve(SB, HB[lm], zm, B, Wm)
            for r in range(nrhs):
                om = ref.backward_error(SB, HB[lm], zm, X[m, r], B[r], Wm)
                om_ref = ref.backward_error(SB, HB[lm], zm, Xref[r], B[r], Wm)
                ratio = om / max(om_ref, EPS)
                worst = max(worst, ratio)
                print("%s m %d (l %d z %s w %d) rhs %d: omega %.3e  omega_ref %.3e  ratio %.3g" % (name, m, lm, zm, wm, r, om, om_ref, ratio))
                assert om <= 8.0 * max(om_ref, EPS), (name, m, r, om, om_ref)
                for q in range(nproj):
                    xl, pl = X[m, r].astype(np.clongdouble), P[q].astype(np.clongdouble)
                    bound = (n + 2) * EPS * float(np.sum(np.abs(pl) * np.abs(xl)))
                    assert abs(complex(np.sum(pl * xl)) - R[m, r, q]) <= bound, (name, m, r, q)
    note("resolvent %s: max omega / max(omega_ref, eps) = %.3g" % (name, worst))
    prob.close()


# ---- T2 ---------------------------------------------------------------------------------------------------------------
def _same(a, b):
    bits = lambda v: np.ascontiguousarray(v).view(np.float64).view(np.uint64)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["lin256", "c5_1024_k11"])
def test_independence_and_determinism(name):
    """G1, G2 bitwise: a batch of 37 matrices (channels, energies and absorbers mixed) with nrhs = 3, nproj = 2 against a second
    run, each matrix alone, the reversed order, resolvent_slots = 1 and 3, resolvent_stage_mb = 1 (n = 1024: the host variant's X in
    two groups; both sizes: fewer slots), nrhs = 1 against the first of 3, nproj = 1 against the first of 2, and the _dev variant
    on torch tensors."""
    prob, SB, HB, WB = _assembled(name)
    n, k = prob.nfun, prob.k
    rng = np.random.default_rng(37)
    nmat = 37
    l = rng.integers(0, 2, nmat).astype(np.int32)
    z = rng.uniform(-0.6, 2.0, nmat) + 1j * rng.choice([0.0, 0.05, -0.05, 0.3], nmat)
    w = rng.integers(-1, 2, nmat).astype(np.int32)
    w[z.imag == 0.0] = 0                                       # a real energy keeps its absorber: never on an eigenvalue
    W2 = np.stack([WB, 0.5 * WB])
    B, P = _vectors(n, 3, 2, 5)
    X, R, info = prob.resolvent(l, z, B, W=W2, w=w, P=P)
    assert np.all(info == 0) and np.all(np.isfinite(X.view(np.float64))) and np.max(np.abs(X)) > 0
    X2, R2, _ = prob.resolvent(l, z, B, W=W2, w=w, P=P)
    assert _same(X2, X) and _same(R2, R)                       # two runs
    for m in range(nmat):                                      # each matrix alone
        Xm, Rm, _ = prob.resolvent(l[m], z[m], B, W=W2, w=w[m], P=P)
        assert _same(Xm[0], X[m]) and _same(Rm[0], R[m]), m
    Xr, Rr, _ = prob.resolvent(l[::-1], z[::-1], B, W=W2, w=w[::-1], P=P)
    assert _same(Xr[::-1], X) and _same(Rr[::-1], R)           # the reversed order
    for opt, val in (("resolvent_slots", 1), ("resolvent_slots", 3), ("resolvent_stage_mb", 1)):
        capi.set_option(opt, val)
        try:
            Xo, Ro, _ = prob.resolvent(l, z, B, W=W2, w=w, P=P)
        finally:
            capi.set_option(opt, 0)
        assert _same(Xo, X) and _same(Ro, R), (opt, val)
    X1, R1, _ = prob.resolvent(l, z, B[0], W=W2, w=w, P=P[0])  # nrhs = 1, nproj = 1
    assert _same(X1[:, 0], X[:, 0]) and _same(R1[:, 0, 0], R[:, 0, 0])
    Xn, Rn, _ = prob.resolvent(l, z, B, W=W2, w=w, P=None)     # no projections
    assert Rn is None and _same(Xn, X)
    Xq, Rq, _ = prob.resolvent(l, z, B, W=W2, w=w, P=P, want_x=False)
    assert Xq is None and _same(Rq, R)
    # the _dev variant on torch tensors, outputs pre-filled with NaN
    dev = "cuda:0"
    Bd, Pd, Wd = torch.from_numpy(B).to(dev), torch.from_numpy(P).to(dev), torch.from_numpy(W2).to(dev)
    Xd = torch.full((nmat, 3, n), float("nan"), dtype=torch.complex128, device=dev)
    Rd = torch.full((nmat, 3, 2), float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.resolvent_dev(l, z, 3, Bd.data_ptr(), nabs=2, W_ptr=Wd.data_ptr(), w=w, nproj=2, P_ptr=Pd.data_ptr(),
                               X_ptr=Xd.data_ptr(), R_ptr=Rd.data_ptr())
    assert np.all(infod == 0)
    assert _same(Xd.cpu().numpy(), X) and _same(Rd.cpu().numpy(), R)
    prob.close()


# ---- T3 ---------------------------------------------------------------------------------------------------------------
def test_real_problem_stays_real_and_eigenvalue_is_survived():
    """G3: real z, no absorber, real B: every imaginary part of X is +-0.0 (n65_k4 and the BT = 15 instance).  z exactly on a
    computed eigenvalue: the result is finite and info >= 0 (rounding may keep the pivot above the threshold)."""
    for name in ("n65_k4", "k16_n40"):
        prob, SB, HB, WB = _assembled(name)
        B = np.random.default_rng(3).standard_normal((2, prob.nfun))
        X, R, info = prob.resolvent([0, 1, 1], [0.3, 0.3, -1.0], B, P=B)
        assert np.all(info == 0) and np.max(np.abs(X.real)) > 0
        assert np.all(X.imag == 0.0) and np.all(R.imag == 0.0), name
        prob.close()
    prob = capi.Problem(_input("n65_k4"))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    B = np.random.default_rng(4).standard_normal((1, prob.nfun))
    zs = np.array([E[0, 0], E[0, 7], E[1, 3], E[1, 64]])
    X, R, info = prob.resolvent([0, 0, 1, 1], zs, B)
    print("on eigenvalues: info", info, "max |x|", np.max(np.abs(X), axis=(1, 2)))
    assert np.all(np.isfinite(X.view(np.float64))) and np.all(info >= 0)
    prob.close()


# ---- T4 ---------------------------------------------------------------------------------------------------------------
# |resolvent_ref.response - the same sum with scipy.linalg.eigh's vectors|, measured on the CPU from the oracle's bands of n65_k4
# (bit-identical to the assembly's) with the b, p below at z = 0.3 + 0.05 i: channel 0: 8.5e-13, channel 1: 2.3e-13 (|R| = 50, 52)
T4_CPU_DIFF = {0: 8.498340637724171e-13, 1: 2.3057084404723514e-13}


def test_spectral_identity():
    """n65_k4: R(z) = p^T (H_l - z S)^-1 b against sum_n (p^T c_n)(c_n^T b) / (E_n - z) over all 65 states from eigvecs, Im z = 0.05;
    tolerance 10 x the CPU-measured difference between the dense reference and the sum with scipy's vectors (T4_CPU_DIFF)."""
    prob = capi.Problem(_input("n65_k4"))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    n = prob.nfun
    b, p = np.random.default_rng(4).standard_normal(n), np.random.default_rng(5).standard_normal(n)
    z = 0.3 + 0.05j
    for l in (0, 1):
        Z = prob.eigvecs(l, 1, n)
        sos = complex(np.sum((Z @ p) * (Z @ b) / (E[l] - z)))
        _, R, info = prob.resolvent(l, z, b, P=p, want_x=False)
        assert info[0] == 0
        print("spectral identity l %d: R %s  sum %s  |diff| %.3e  tolerance %.3e" % (l, R[0, 0, 0], sos, abs(R[0, 0, 0] - sos), 10 * T4_CPU_DIFF[l]))
        assert abs(R[0, 0, 0] - sos) <= 10.0 * T4_CPU_DIFF[l], l
    prob.close()


# ---- T5 ---------------------------------------------------------------------------------------------------------------
def test_polarizability_and_photoabsorption_end_to_end():
    """host.polarizability(omega = 0) and host.photoabsorption at omega = 0.55, 0.7, 1.0, 1.5 on test_resolvent_cpu's grid against
    the CPU route recomputed from the problem's own bands (dense solves of resolvent_ref).  Each R(z) may differ from the dense
    reference's by ||p||_1 ||M^-1||_inf (||r_gpu||_inf + ||r_ref||_inf) with ||r|| <= omega (||M||_inf ||x||_inf + ||b||_inf), omega_gpu <= 8
    max(omega_ref, eps) (T1's bound), plus the two dot products' 2 (n + 2) eps sum |p_i| |x_i|.  alpha(0) within 1e-10 of 4.5."""
    prob = capi.Problem(capi.make_input(**HYD))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    n = prob.nfun
    omegas = np.array([0.55, 0.7, 1.0, 1.5])
    cap = lambda r: host.cap_profile(r, 20.0, 1e-3)
    alpha0 = complex(host.polarizability(prob, 1, 0.0))
    sigma = host.photoabsorption(prob, 1, omegas, cap)
    b = host.band_apply(prob.dipole_bands()[0], prob.eigvecs(0, 1, 1))[0]
    WB = prob.operator_bands(cap(prob.quadrature()[0]), [0])[0]
    SB, HB = prob.assemble(0, 2)                               # the problem's own bands (this ends the state of the solve)

    def cpu_route(z, W):
        """(R_ref, bound on |R_gpu - R_ref|)"""
        x = ref.solve(SB, HB[1], z, b, W)[0]
        om_ref = ref.backward_error(SB, HB[1], z, x, b, W)
        M = ref.dense_matrix(SB, HB[1], z, W)
        scale = np.max(np.sum(np.abs(M), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(b))
        res = (8.0 * max(om_ref, EPS) + om_ref) * scale
        return complex(np.sum(b * x)), np.sum(np.abs(b)) * ref.norm_inverse(SB, HB[1], z, W) * res + 2 * (n + 2) * EPS * np.sum(np.abs(b) * np.abs(x))

    E1s = E[0, 0]
    R0, t0 = cpu_route(E1s, None)
    print("alpha(0): gpu %.15f  cpu %.15f  |diff| %.3e  bound %.3e" % (alpha0.real, 2 * R0.real / 3, abs(alpha0 - 2 * R0 / 3), 2 * t0 / 3))
    assert abs(alpha0 - 2.0 * R0 / 3.0) <= 2.0 * t0 / 3.0
    assert abs(alpha0 - 4.5) <= 1e-10
    for i, om in enumerate(omegas):
        (Rp, tp), (Rm, tm) = cpu_route(E1s + om, WB), cpu_route(E1s - om, WB)
        s_ref = 4.0 * np.pi * om * ((Rp + Rm) / 3.0).imag / host.C_RESPONSE
        tol = 4.0 * np.pi * om * (tp + tm) / 3.0 / host.C_RESPONSE
        dev = sigma[i] / ref.sigma_h1s(om) - 1.0
        print("sigma(%.2f): gpu %.12e  cpu %.12e  |diff| %.3e  bound %.3e  vs closed form %.2e" % (om, sigma[i], s_ref, abs(sigma[i] - s_ref), tol, dev))
        assert abs(sigma[i] - s_ref) <= tol, om
        assert abs(dev) <= 6e-2, om
    prob.close()


# ---- T6 ---------------------------------------------------------------------------------------------------------------
def test_resolvent_argument_checks():
    prob = capi.Problem(_input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    l, z, w = np.array([0, 1], dtype=np.int32), np.array([0.3, 0.05, 0.1, -0.05]), np.array([-1, 0], dtype=np.int32)
    WB, B, P = np.zeros((2 * k - 1) * n), np.ones(2 * n), np.ones(2 * n)
    X, R, info = np.zeros(2 * 2 * n), np.zeros(2 * 2), np.zeros(2, dtype=np.int32)
    dv = lambda a: torch.from_numpy(a).to("cuda:0")
    WBd, Bd, Pd, Xd, Rd = dv(WB), dv(B), dv(P), dv(X), dv(R)
    dp = lambda t: C.c_void_p(t.data_ptr())
    variants = ((L.bspatom_resolvent, p_(WB), p_(B), p_(P), p_(X), p_(R)), (L.bspatom_resolvent_dev, dp(WBd), dp(Bd), dp(Pd), dp(Xd), dp(Rd)))
    for fn, wb, b, pp, x, r in variants:                       # before any solve or assemble: no channel is there
        assert fn(prob._h, 2, p_(l), p_(z), 1, wb, p_(w), 1, b, 1, pp, x, r, p_(info)) == -2
    prob.assemble(0, 2)
    for fn, wb, b, pp, x, r in variants:
        good = [prob._h, 2, p_(l), p_(z), 1, wb, p_(w), 1, b, 1, pp, x, r, p_(info)]
        sub = lambda pos, v: [v if i == pos else g for i, g in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 2, 3, 8, 13):                           # p, l, z, B, info
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(5, None)) == -2                         # nabs = 1 without WB
        assert fn(*sub(10, None)) == -2                        # R without P
        assert fn(*sub(9, 0)) == -2                            # R with nproj = 0
        assert fn(*[None if i in (11, 12) else g for i, g in enumerate(good)]) == -2        # neither X nor R
        assert fn(*sub(11, None)) == 0 and fn(*sub(12, None)) == 0                          # one of them is enough
        assert fn(*[None if i in (10, 12) else g for i, g in enumerate(good)]) == 0         # P may be NULL when R is
        for pos in (1, 7):                                     # nmat, nrhs below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(4, -1)) == -2                           # nabs < 0
        for bad in ([0, 2], [-1, 0]):                          # a channel outside the bands held
            assert fn(*sub(2, p_(np.array(bad, dtype=np.int32)))) == -2, bad
        for bad in ([-2, 0], [0, 1]):                          # w outside -1 .. nabs-1
            assert fn(*sub(6, p_(np.array(bad, dtype=np.int32)))) == -2, bad
        assert fn(*[0 if i == 4 else (None if i == 5 else g) for i, g in enumerate(good)]) == -2   # w = 0 with no absorber at all
        assert fn(*sub(6, None)) == 0                          # w NULL: absorber 0 everywhere
        assert fn(*good) == 0                                  # a valid call afterwards
    prob.solve(0, 1)                                           # the last solve holds channel 0 alone
    with pytest.raises(capi.BspAtomError) as ei:
        prob.resolvent([0, 1], 0.3 + 0.1j, np.ones(n))
    assert ei.value.code == -2
    X1, _, info1 = prob.resolvent(0, 0.3 + 0.1j, np.ones(n))
    assert info1[0] == 0 and np.all(np.isfinite(X1.view(np.float64)))
    assert capi.get_option("resolvent_stage_mb") == 0 and capi.get_option("resolvent_slots") == 0
    prob.close()
