"""Chains of resolvents (bspatom_resolvent_chain / _dev, csrc/resolvent.hip: resolvent_chain_kernel): the guarantees C1 - C6 of
include/bspatom.h bit for bit -- composition of bspatom_resolvent calls with the band apply restated on the CPU
(tests/resolvent_chain_ref.py) in between, independence, prefixes, one stage = bspatom_resolvent --, the backward error of the last
stage against LAPACK's, the host helpers end to end, the argument checks.  Cases and helpers are test_gpu_resolvent's."""
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note
from test_gpu_resolvent import HYD, _assembled, _input, _same, _vectors

import resolvent_ref as ref
import resolvent_chain_ref as cref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _operators(prob):
    """three operator bands (3, 2k-1, n): r, d/dr (not symmetric) and the overlap"""
    RB = prob.dipole_bands()
    SF = prob.operator_bands(np.ones(prob.quadrature()[0].size), [0])[0]
    return np.stack([RB[0], RB[2], SF])


def _chains(nchain, nstage, seed):
    """(l, z, w, a): channels 0 / 1, energies real inside the spectrum WITH an absorber or with Im z = +-0.05 (absorber on or off),
    two absorbers, real coefficients of three operators"""
    rng = np.random.default_rng(seed)
    l = rng.integers(0, 2, (nchain, nstage)).astype(np.int32)
    z = rng.uniform(-0.4, 1.5, (nchain, nstage)) + 1j * rng.choice([0.0, 0.05, -0.05], (nchain, nstage))
    w = rng.integers(-1, 2, (nchain, nstage)).astype(np.int32)
    w[(z.imag == 0.0) & (w < 0)] = 0                           # a real energy keeps an absorber: never on an eigenvalue
    a = rng.standard_normal((nchain, max(nstage - 1, 0), 3))
    return l, z, w, a


# ---- T1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "lin256", "c5_k11_n130", "k16_n40"])
def test_chain_is_the_composition_of_resolvent_calls(name):
    """C5, C4 bitwise: 6 chains of 3 stages, nrhs = 2, nproj = 2, channels, energies and absorbers mixed, three operators (r, d/dr,
    S) combined with real coefficients.  Every stage's R and info and the final X equal the staged route: Problem.resolvent with
    nmat = 1 per stage, its right-hand sides A x_{s-1} formed on the CPU by resolvent_chain_ref.band_combine_apply.  One stage
    equals Problem.resolvent on the same batch.  n < 2b + 1 (tiny8), n no multiple of the prefetch block (n65_k4), b = 8 (lin256),
    b = 10 and b = 15 on the BT = 15 instance."""
    prob, SB, HB, WB = _assembled(name)
    n = prob.nfun
    GB = _operators(prob)
    W2 = np.stack([WB, 0.5 * WB])
    nchain, nstage = 6, 3
    l, z, w, a = _chains(nchain, nstage, 61)
    B, P = _vectors(n, 2, 2, 9)
    X, R, info = prob.resolvent_chain(l, z, B, G=GB, a=a, W=W2, w=w, P=P)
    assert X.shape == (nchain, 2, n) and R.shape == (nchain, nstage, 2, 2) and info.shape == (nchain, nstage)
    assert np.all(info == 0), info
    assert np.all(np.isfinite(X.view(np.float64))) and np.max(np.abs(X)) > 0
    for c in range(nchain):
        y = B
        for s in range(nstage):
            if s:
                y = cref.band_combine_apply(GB, a[c, s - 1], xs[0])
            xs, rs, infs = prob.resolvent(l[c, s], z[c, s], y, W=W2, w=w[c, s], P=P)
            assert _same(rs[0], R[c, s]) and infs[0] == info[c, s], (name, c, s)
        assert _same(xs[0], X[c]), (name, c)
    X1, R1, info1 = prob.resolvent_chain(l[:, :1], z[:, :1], B, W=W2, w=w[:, :1], P=P)      # one stage: no G, no a
    Xr, Rr, infor = prob.resolvent(l[:, 0], z[:, 0], B, W=W2, w=w[:, 0], P=P)
    assert _same(X1, Xr) and _same(R1[:, 0], Rr) and np.array_equal(info1[:, 0], infor)
    prob.close()


# ---- T2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lin256", "c5_1024_k11"])
def test_chain_independence_determinism_prefix(name):
    """C1, C2, C3 bitwise: 37 chains of 3 stages, nrhs = 3, nproj = 2, against a second run, each chain alone, the reversed order,
    resolvent_slots = 1 and 3, resolvent_stage_mb = 1 (n = 1024: the host variant's X in two groups; both sizes: fewer slots),
    nrhs = 1 against the first of 3, no P, want_x=False, the chains cut to 1 and 2 stages (R, info of the prefix; the cut chain's
    X through one more stage by hand gives the next R), and the _dev variant on torch tensors pre-filled with NaN."""
    prob, SB, HB, WB = _assembled(name)
    n, k = prob.nfun, prob.k
    GB = _operators(prob)
    W2 = np.stack([WB, 0.5 * WB])
    nchain, nstage = 37, 3
    l, z, w, a = _chains(nchain, nstage, 37)
    B, P = _vectors(n, 3, 2, 5)

    def run(l=l, z=z, w=w, a=a, B=B, P=P, want_x=True):
        return prob.resolvent_chain(l, z, B, G=GB, a=a, W=W2, w=w, P=P, want_x=want_x)

    X, R, info = run()
    assert np.all(info == 0) and np.all(np.isfinite(X.view(np.float64))) and np.max(np.abs(X)) > 0
    X2, R2, info2 = run()
    assert _same(X2, X) and _same(R2, R) and np.array_equal(info2, info)                    # two runs
    for c in range(nchain):                                    # each chain alone
        Xc, Rc, _ = run(l=l[c], z=z[c], w=w[c], a=a[c:c + 1])
        assert _same(Xc[0], X[c]) and _same(Rc[0], R[c]), c
    Xv, Rv, _ = run(l=l[::-1], z=z[::-1], w=w[::-1], a=a[::-1])
    assert _same(Xv[::-1], X) and _same(Rv[::-1], R)           # the reversed order
    for opt, val in (("resolvent_slots", 1), ("resolvent_slots", 3), ("resolvent_stage_mb", 1)):
        capi.set_option(opt, val)
        try:
            Xo, Ro, _ = run()
        finally:
            capi.set_option(opt, 0)
        assert _same(Xo, X) and _same(Ro, R), (opt, val)
    X1, R1, _ = run(B=B[0])                                    # nrhs = 1
    assert _same(X1[:, 0], X[:, 0]) and _same(R1[:, :, 0], R[:, :, 0])
    Xn, Rn, _ = run(P=None)                                    # no projections
    assert Rn is None and _same(Xn, X)
    Xq, Rq, _ = run(want_x=False)
    assert Xq is None and _same(Rq, R)
    for cut in (1, 2):                                         # prefixes
        Xp, Rp, infop = run(l=l[:, :cut], z=z[:, :cut], w=w[:, :cut], a=a[:, :cut - 1])
        assert _same(Rp, R[:, :cut]) and np.array_equal(infop, info[:, :cut]), cut
        c = 5                                                  # the cut chain's X is x_{c, cut-1}: one more stage by hand
        y = cref.band_combine_apply(GB, a[c, cut - 1], Xp[c])
        _, rn, _ = prob.resolvent(l[c, cut], z[c, cut], y, W=W2, w=w[c, cut], P=P)
        assert _same(rn[0], R[c, cut]), cut
    # the _dev variant on torch tensors, outputs pre-filled with NaN
    dev = "cuda:0"
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    Bd, Pd, Wd, Gd = up(B), up(P), up(W2), up(GB)
    Xd = torch.full((nchain, 3, n), float("nan"), dtype=torch.complex128, device=dev)
    Rd = torch.full((nchain, nstage, 3, 2), float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.resolvent_chain_dev(l, z, 3, Bd.data_ptr(), nop=3, G_ptr=Gd.data_ptr(), a=a, nabs=2, W_ptr=Wd.data_ptr(), w=w, nproj=2,
                                     P_ptr=Pd.data_ptr(), X_ptr=Xd.data_ptr(), R_ptr=Rd.data_ptr())
    assert np.array_equal(infod, info)
    assert _same(Xd.cpu().numpy(), X) and _same(Rd.cpu().numpy(), R)
    prob.close()


# ---- T3 ---------------------------------------------------------------------------------------------------------------
def test_real_chain_stays_real():
    """C6: real z below the lowest eigenvalue of either channel (on no eigenvalue, so info = 0), no absorber, real B: every
    imaginary part of X is +-0.0 and every R (real P) is real, through three stages (n65_k4 and the BT = 15 instance)."""
    for name in ("n65_k4", "k16_n40"):
        prob = capi.Problem(_input(name))
        E, sinfo = prob.solve(0, 2)
        assert np.all(sinfo == 0)
        edge = float(np.min(E))
        GB = _operators(prob)
        B = np.random.default_rng(3).standard_normal((2, prob.nfun))
        a = np.random.default_rng(4).standard_normal((2, 2, 3))
        z = edge - np.array([[0.5, 1.0, 0.25], [2.0, 0.125, 1.5]])
        X, R, info = prob.resolvent_chain([[0, 1, 0], [1, 1, 0]], z, B, G=GB, a=a, P=B)
        assert np.all(info == 0) and np.max(np.abs(X.real)) > 0
        assert np.all(X.imag == 0.0) and np.all(R.imag == 0.0), name
        prob.close()


# ---- T4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lin256", "k16_n40"])
def test_last_stage_backward_error_against_lapack(name):
    """The LAST stage of chains of 2 and 3 stages: omega = ||y - M x||_inf / (||M||_inf ||x||_inf + ||y||_inf) in long double, M from the
    caller-visible bands, y = A x_prev rebuilt in long double from the X the chain cut by one stage returns (C3), x the full
    chain's X.  omega <= 8 max(omega_ref, eps), omega_ref numpy.linalg.solve's on the same matrix with the float64 right-hand side
    resolvent_chain_ref.band_combine_apply forms, measured against the same long double y: test_gpu_resolvent's T1 bound, for the
    same reason -- a stage is that kernel's LU (C5), the right-hand side's own rounding is shared by both.
    Measured on the MI355X, maximum of omega / max(omega_ref, eps) per case: lin256 0.108, k16_n40 0.388 (both omegas lie below eps:
    4e-18 .. 9e-17; the ratio is omega / eps)."""
    prob, SB, HB, WB = _assembled(name)
    n = prob.nfun
    GB = _operators(prob)
    GL = [ref.full_to_dense(g, np.longdouble) for g in GB]
    B, _ = _vectors(n, 2, 0, 13)
    worst = 0.0
    for nstage in (2, 3):
        l, z, w, a = _chains(4, nstage, 70 + nstage)
        w = np.minimum(w, 0)                                   # one absorber
        X, _, info = prob.resolvent_chain(l, z, B, G=GB, a=a, W=WB, w=w)
        Xp, _, _ = prob.resolvent_chain(l[:, :-1], z[:, :-1], B, G=GB, a=a[:, :-1], W=WB, w=w[:, :-1])
        assert np.all(info == 0)
        for c in range(4):
            Wm = WB if w[c, -1] == 0 else None
            A = sum(np.longdouble(a[c, -1, o]) * GL[o] for o in range(3))
            y64 = cref.band_combine_apply(GB, a[c, -1], Xp[c])
            Xref = ref.solve(SB, HB[l[c, -1]], z[c, -1], y64, Wm)
            for r in range(2):
                yl = A.astype(np.clongdouble) @ Xp[c, r].astype(np.clongdouble)
                om = ref.backward_error(SB, HB[l[c, -1]], z[c, -1], X[c, r], yl, Wm)
                om_ref = ref.backward_error(SB, HB[l[c, -1]], z[c, -1], Xref[r], yl, Wm)
                ratio = om / max(om_ref, EPS)
                worst = max(worst, ratio)
                print("%s nstage %d chain %d rhs %d: omega %.3e  omega_ref %.3e  ratio %.3g" % (name, nstage, c, r, om, om_ref, ratio))
                assert om <= 8.0 * max(om_ref, EPS), (name, nstage, c, r, om, om_ref)
    note("resolvent chain %s: max omega / max(omega_ref, eps) = %.3g" % (name, worst))
    prob.close()


# ---- T5 ---------------------------------------------------------------------------------------------------------------
def test_chain_helpers_end_to_end():
    """test_resolvent_chain_cpu's grid (channels 0, 1): host.cauchy_moments(prob, 1, 3) within 1e-9 of (9/2, 43/4, 319/12);
    host.two_photon for 1s -> 2s within 1e-9 of the dense CPU solve on the problem's own bands and vectors, and 1/3 of it within 1e-5
    of -7.85366; host.response_chain with one stage equals host.response bit for bit (with and without absorber and left operator);
    two_photon_ati gives the chain's own number."""
    prob = capi.Problem(capi.make_input(**HYD))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    mom = host.cauchy_moments(prob, 1, 3)
    print("moments", mom)
    assert mom.shape == (3,) and np.max(np.abs(mom - np.array([4.5, 43.0 / 4.0, 319.0 / 12.0]))) <= 1e-9
    omega = 0.5 * (E[0, 1] - E[0, 0])
    amp = complex(host.two_photon(prob, 1, 1, (0, 2), omega))
    cap = lambda r: host.cap_profile(r, 20.0, 1e-3)
    zs = E[0, 0] + np.array([[0.2 + 0.05j, 0.7], [1.1, -0.3]])
    for absorber in (None, cap):
        zz = zs + (0.0 if absorber else 0.05j)
        for a_left in (None, (0.0, 1.0, 0.5)):
            one = host.response_chain(prob, 0, 1, [(1, (1.0, 0.0, 0.25))], zz[..., None], absorber=absorber,
                                      left=None if a_left is None else (0, 1, a_left))
            assert one.shape == zz.shape
            assert _same(one, host.response(prob, 0, 1, 1, (1.0, 0.0, 0.25), zz, absorber=absorber, a_left=a_left))
    om2 = np.array([0.3, 0.45])
    ati = host.two_photon_ati(prob, 1, (1, 0), om2, cap)
    r1 = (1.0, 0.0, 0.0)
    assert _same(ati, host.response_chain(prob, 0, 1, [(1, r1), (0, r1)], E[0, 0] + np.stack([om2, 2 * om2], axis=-1), absorber=cap))
    assert np.all(np.isfinite(ati)) and np.all(ati.imag != 0.0)
    c = prob.eigvecs(0, 1, 2)
    RB = prob.dipole_bands()
    b, p = host.band_apply(RB[0], c[:1])[0], host.band_apply(RB[0], c[1:])[0]
    SB, HB = prob.assemble(0, 2)                               # the problem's own bands (this ends the state of the solve)
    cpu = ref.response(SB, HB[1], E[0, 0] + omega, b, p=p)
    print("two_photon 1s-2s: gpu %.12f  cpu %.12f  |diff| %.3e  (1/3: %.9f)" % (amp.real, cpu.real, abs(amp - cpu), amp.real / 3))
    assert abs(amp - cpu) <= 1e-9
    assert abs(abs(amp) / 3.0 - 7.85366) <= 1e-5               # the sign is that of the two vectors' signs
    prob.close()


# ---- T6 ---------------------------------------------------------------------------------------------------------------
def test_chain_argument_checks():
    """every BSPATOM_ERR_ARG condition of bspatom_resolvent_chain returns -2 and writes nothing, host and _dev"""
    prob = capi.Problem(_input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: np.array(v, dtype=np.int32)
    nchain, nstage, nop = 2, 2, 2
    l, w = i32([0, 1, 1, 0]), i32([-1, 0, 0, -1])
    z = np.array([0.3, 0.05, 0.1, -0.05, 0.2, 0.05, -0.1, 0.05])
    a = np.array([1.0, 0.5, -0.5, 2.0])
    WB, B, P = np.zeros((2 * k - 1) * n), np.ones(2 * n), np.ones(2 * n)
    GB = np.ascontiguousarray(prob.dipole_bands()[:2]).reshape(-1)
    SENT = -7.25
    X, R, info = np.full(2 * nchain * n, SENT), np.full(2 * nchain * nstage, SENT), np.full(nchain * nstage, -7, dtype=np.int32)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    WBd, GBd, Bd, Pd, Xd, Rd = dv(WB), dv(GB), dv(B), dv(P), dv(X), dv(R)
    dp = lambda t: C.c_void_p(t.data_ptr())
    variants = ((L.bspatom_resolvent_chain, p_(WB), p_(GB), p_(B), p_(P), p_(X), p_(R)),
                (L.bspatom_resolvent_chain_dev, dp(WBd), dp(GBd), dp(Bd), dp(Pd), dp(Xd), dp(Rd)))
    # positions: 0 p, 1 nchain, 2 nstage, 3 l, 4 z, 5 nabs, 6 WB, 7 w, 8 nop, 9 GB, 10 a, 11 nrhs, 12 B, 13 nproj, 14 P, 15 X, 16 R, 17 info
    mk = lambda wb, gb, b, pp, x, r: [prob._h, nchain, nstage, p_(l), p_(z), 1, wb, p_(w), nop, gb, p_(a), 1, b, 1, pp, x, r, p_(info)]
    for fn, *ptrs in variants:                                 # before any solve or assemble: no channel is there
        assert fn(*mk(*ptrs)) == -2
    prob.assemble(0, 2)
    for fn, *ptrs in variants:
        good = mk(*ptrs)
        sub = lambda pos, v: [v if i == pos else g for i, g in enumerate(good)]
        for pos in (0, 3, 4, 12, 17):                          # p, l, z, B, info
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(6, None)) == -2                         # nabs = 1 without WB
        assert fn(*sub(14, None)) == -2                        # R without P
        assert fn(*sub(13, 0)) == -2                           # R with nproj = 0
        assert fn(*[None if i in (15, 16) else g for i, g in enumerate(good)]) == -2        # neither X nor R
        for pos in (1, 2, 11):                                 # nchain, nstage, nrhs below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(5, -1)) == -2                           # nabs < 0
        for bad in ([0, 1, 1, 2], [0, -1, 1, 0], [2, 1, 1, 0]):                             # a channel outside the bands held, any stage
            assert fn(*sub(3, p_(i32(bad)))) == -2, bad
        for bad in ([-1, 0, 0, -2], [-1, 1, 0, -1]):           # w outside -1 .. nabs-1, any stage
            assert fn(*sub(7, p_(i32(bad)))) == -2, bad
        assert fn(*[0 if i == 5 else (None if i == 6 else g) for i, g in enumerate(good)]) == -2   # w = 0 with no absorber at all
        assert fn(*sub(8, 0)) == -2 and fn(*sub(8, -1)) == -2  # nstage > 1 with nop < 1
        assert fn(*sub(9, None)) == -2 and fn(*sub(10, None)) == -2                         # nstage > 1 without GB, without a
        one = lambda nop, gb, a: [{2: 1, 8: nop, 9: gb, 10: a}.get(i, g) for i, g in enumerate(good)]   # the same with one stage
        assert fn(*one(nop=-1, gb=good[9], a=good[10])) == -2  # nop < 0, even where no operator is needed
        # nothing was written by any refused call
        assert np.all(X == SENT) and np.all(R == SENT) and np.all(info == -7)
        assert bool(torch.all(Xd == SENT)) and bool(torch.all(Rd == SENT))
        assert fn(*one(nop=0, gb=None, a=None)) == 0           # one stage needs neither GB nor a
        assert np.all(info[:2] == 0) and np.all(info[2:] == -7)
        info[:] = -7
        assert fn(*sub(15, None)) == 0 and fn(*sub(16, None)) == 0                          # one of X and R is enough
        assert fn(*[None if i in (14, 16) else g for i, g in enumerate(good)]) == 0         # P may be NULL when R is
        assert fn(*sub(7, None)) == 0                          # w NULL: absorber 0 everywhere
        assert fn(*good) == 0 and np.all(info == 0)            # a valid call afterwards
        X[:], R[:], info[:] = SENT, SENT, -7
        Xd.fill_(SENT); Rd.fill_(SENT)
        torch.cuda.synchronize()
    with pytest.raises(capi.BspAtomError) as ei:
        prob.resolvent_chain([0, 2], 0.3 + 0.1j, np.ones(n), G=GB.reshape(2, 2 * k - 1, n), a=[[1.0, 0.0]])
    assert ei.value.code == -2
    prob.close()
