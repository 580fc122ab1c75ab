"""u(r) and u'(r) for blocks of states on the GPU (bspatom_quadrature / bspatom_tabulate* / bspatom_wavefunctions*,
csrc/wavefn.hip) against the CPU restatement of test_wavefunctions_cpu.py (BSPALL from the oracle, the ordered NumPy sum):
bit for bit on the quadrature grid and on caller's points, the bounds of the output, wavefunctions == tabulate(eigvecs_batch),
the link to write_wf and to the compiled reference's wf_n0.dat, the quadrature identities against S and the dipole blocks, the
argument checks, and the C4 size."""
import time
import ctypes as C
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from conftest import load_golden
from test_gpu_stages import note
from test_wavefunctions_cpu import case_kw, quadrature_ref, basis_ref, tabulate_ref

import oracle as orc
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
K16 = dict(kind_grid=0, ra=0.0, rb=40.0, k=16, nfun=70, l_fin=0, zatom=1.0)     # the largest order of this build (ka = 19)


def setup(name, **over):
    """(problem, oracle cfg, rt, aind, xg, wg) of a committed input, or of the k = 16 problem"""
    kw = dict(K16) if name == "k16" else case_kw(name, **over)
    prob = capi.Problem(capi.make_input(**kw))
    cfg = orc.make_cfg(**kw)
    rt, aind, xg, wg = orc.grid(cfg)
    assert np.array_equal(rt, prob.grid()[0])
    return prob, cfg, rt, aind, xg, wg


def solved(name, nl=None, **over):
    prob, cfg, rt, aind, xg, wg = setup(name, **over)
    nl = prob.lmax + 1 if nl is None else nl
    E, info = prob.solve(0, nl)
    assert np.all(info == 0)
    return prob, cfg, rt, aind, xg, wg


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def nan_dev(n):
    t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    return t


GUARD = 64


def tabulate_dev_checked(prob, Z, r, npts, deriv=True):
    """tabulate_dev into NaN-filled tensors with GUARD elements behind each table: (U, dU) as arrays, guards asserted NaN"""
    nvec = Z.shape[0]
    Zd = dev(Z)
    Ud, dUd = nan_dev(nvec * npts + GUARD), nan_dev(nvec * npts + GUARD)
    assert prob.tabulate_dev(nvec, Zd.data_ptr(), Ud.data_ptr(), dUd.data_ptr() if deriv else None, r=r) == npts
    U, dU = Ud.cpu().numpy(), dUd.cpu().numpy()
    assert np.all(np.isnan(U[nvec * npts:])) and np.all(np.isnan(dU[nvec * npts:]))
    if not deriv:
        assert np.all(np.isnan(dU))
    return U[:nvec * npts].reshape(nvec, npts), dU[:nvec * npts].reshape(nvec, npts)


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "bsp0", "bc1", "ka_ra"])
def test_quadrature_equals_restatement(name):
    prob, cfg, rt, aind, xg, wg = setup(name)
    r, w = prob.quadrature()
    rr, wr = quadrature_ref(rt, xg, wg)
    assert r.size == prob.nointv * prob.ka
    assert np.array_equal(r, rr) and np.array_equal(w, wr)
    prob.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def caller_points(rt, npts, rng):
    """rb first (interv's walk down), ra, every distinct knot, 40 random points, then duplicates of what is there; shuffled.
    npts None: all of it (every distinct knot is in), else its first npts, filled up with random points and duplicates"""
    ra, rb = rt[0], rt[-1]
    knots = rng.permutation(np.unique(rt))
    pool = np.concatenate([[rb, ra], knots, ra + (rb - ra) * rng.random(40)])
    pool = np.concatenate([pool, pool[rng.integers(0, pool.size, size=24)]])
    if npts is None:
        return rng.permutation(pool)
    if npts > pool.size:
        more = ra + (rb - ra) * rng.random(npts - pool.size)
        more[::3] = pool[rng.integers(0, pool.size, size=more[::3].size)]
        pool = np.concatenate([pool, more])
    return rng.permutation(pool[:npts])


@pytest.mark.parametrize("name", ["tiny8", "n65_k4", "bsp0", "lin256", "c5_1024_k11", "k16"])
def test_tabulate_bit_for_bit(name):
    """Random coefficient vectors, nvec = 1 and 37, host and device variants, U and dU against the restatement with
    np.array_equal: on the quadrature grid (the assembly's point table), on caller's points of npts = 1, 63, 257 (rb, ra, knots,
    unsorted random points, duplicates), and on every distinct knot at once."""
    prob, cfg, rt, aind, xg, wg = setup(name)
    rng = np.random.default_rng(11)
    n, k = prob.nfun, prob.k
    Zall = rng.standard_normal((37, n)) * 10.0 ** rng.integers(-3, 3, size=(37, 1))
    rq, _ = quadrature_ref(rt, xg, wg)
    allknots = caller_points(rt, None, rng)
    assert set(np.unique(rt)) <= set(allknots)
    grids = [("quadrature", None, rq)]
    grids += [("caller %d" % m, caller_points(rt, m, rng), None) for m in (1, 63, 257)]
    grids += [("all knots", allknots, None)]
    for tag, r, rref in grids:
        pts = rref if r is None else r
        basis = basis_ref(cfg, rt, aind, pts)
        Uall, dUall = tabulate_ref(k, Zall, basis)
        for nvec in (1, 37):
            Z = Zall[:nvec]
            U, dU = prob.tabulate(Z, r=r)
            assert U.shape == (nvec, pts.size)
            assert np.array_equal(U, Uall[:nvec]), (name, tag, nvec, "U host")
            assert np.array_equal(dU, dUall[:nvec]), (name, tag, nvec, "dU host")
            assert np.array_equal(prob.tabulate(Z, r=r, deriv=False), Uall[:nvec]), (name, tag, nvec, "U host, values only")
            Ud, dUd = tabulate_dev_checked(prob, Z, r, pts.size)
            assert np.array_equal(Ud, Uall[:nvec]), (name, tag, nvec, "U dev")
            assert np.array_equal(dUd, dUall[:nvec]), (name, tag, nvec, "dU dev")
        assert pts.size == 1 or (np.max(np.abs(Uall)) > 0 and np.max(np.abs(dUall)) > 0)      # u(rb) itself is zero (boundary condition)
    prob.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_tabulate_dev_stays_inside_its_tables():
    """n65_k4, 37 vectors, 257 caller's points and the quadrature grid (neither a multiple of the point tile): with dU = NULL the
    NaN-filled dU tensor stays NaN, and the guard elements behind U_dev (and dU_dev) stay NaN."""
    prob, cfg, rt, aind, xg, wg = setup("n65_k4")
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((37, prob.nfun))
    for r in (caller_points(rt, 257, rng), None):
        pts = quadrature_ref(rt, xg, wg)[0] if r is None else r
        Uref, dUref = tabulate_ref(prob.k, Z, basis_ref(cfg, rt, aind, pts))
        U, _ = tabulate_dev_checked(prob, Z, r, pts.size, deriv=False)
        assert np.array_equal(U, Uref)
        U, dU = tabulate_dev_checked(prob, Z, r, pts.size, deriv=True)
        assert np.array_equal(U, Uref) and np.array_equal(dU, dUref)
    prob.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_wavefunctions_equal_tabulate_of_eigvecs_batch():
    """lin256, channels 1 .. 3, states 2 .. 38: wavefunctions == tabulate(eigvecs_batch) bit for bit on the quadrature grid and on
    caller's points; host == _dev; the same bits with wf_stage_mb = 1 (several groups through the stage buffer)."""
    prob, cfg, rt, aind, xg, wg = solved("lin256")
    l0, nl, n0, cnt = 1, 3, 2, 37
    Z = prob.eigvecs_batch(l0, nl, n0, cnt)
    rng = np.random.default_rng(9)
    for r in (None, caller_points(rt, 257, rng)):
        Ut, dUt = prob.tabulate(Z.reshape(nl * cnt, -1), r=r)
        npts = Ut.shape[1]
        U, dU = prob.wavefunctions(l0, nl, n0, cnt, r=r)
        assert U.shape == (nl, cnt, npts)
        assert np.array_equal(U.reshape(nl * cnt, npts), Ut) and np.array_equal(dU.reshape(nl * cnt, npts), dUt)
        assert np.array_equal(prob.wavefunctions(l0, nl, n0, cnt, r=r, deriv=False), U)
        Ud, dUd = nan_dev(nl * cnt * npts + GUARD), nan_dev(nl * cnt * npts + GUARD)
        capi.set_option("wf_stage_mb", 1)
        try:
            assert nl * cnt * npts * 16 > 3 * (1 << 20) or r is not None       # quadrature grid: more than three passes
            Ug, dUg = prob.wavefunctions(l0, nl, n0, cnt, r=r)
            assert prob.wavefunctions_dev(l0, nl, n0, cnt, Ud.data_ptr(), dUd.data_ptr(), r=r) == npts
        finally:
            capi.set_option("wf_stage_mb", 0)
        assert np.array_equal(Ug, U) and np.array_equal(dUg, dU)
        a, b = Ud.cpu().numpy(), dUd.cpu().numpy()
        assert np.all(np.isnan(a[nl * cnt * npts:])) and np.all(np.isnan(b[nl * cnt * npts:]))
        assert np.array_equal(a[:nl * cnt * npts].reshape(U.shape), U) and np.array_equal(b[:nl * cnt * npts].reshape(U.shape), dU)
        Ud2 = nan_dev(nl * cnt * npts)
        prob.wavefunctions_dev(l0, nl, n0, cnt, Ud2.data_ptr(), None, r=r)
        assert np.array_equal(Ud2.cpu().numpy().reshape(U.shape), U)
    # every state of the three channels (512 KiB of eigenvectors each): under wf_stage_mb = 1 the inverse iterations run in two
    # groups of channels (2 + 1)
    r = caller_points(rt, 63, rng)
    n = prob.nfun
    Ut = prob.tabulate(prob.eigvecs_batch(l0, nl, 1, n).reshape(nl * n, n), r=r, deriv=False).reshape(nl, n, 63)
    Ud = nan_dev(nl * n * 63 + GUARD)
    capi.set_option("wf_stage_mb", 1)
    try:
        Ug = prob.wavefunctions(l0, nl, 1, n, r=r, deriv=False)
        prob.wavefunctions_dev(l0, nl, 1, n, Ud.data_ptr(), None, r=r)
    finally:
        capi.set_option("wf_stage_mb", 0)
    a = Ud.cpu().numpy()
    assert np.array_equal(Ug, Ut) and np.array_equal(a[:nl * n * 63].reshape(Ut.shape), Ut) and np.all(np.isnan(a[nl * n * 63:]))
    prob.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bsp0", "lin256"])
def test_wavefunctions_vs_write_wf_and_reference(name):
    """The state (l_ini, n0_ini) at write_wf's points.  |u - write_wf(eigvec)| <= 8 k eps max|c|: both are the same k-term sum of
    basis values that are positive and sum to one, the terms bounded by max|c|; they differ only by the FMA contraction of
    wf_kernel.  Against the compiled reference's wf_n0.dat rows: the bar of test_gpu_solve.py, 2e-8 of max|u|."""
    prob, cfg, rt, aind, xg, wg = solved(name)
    g = load_golden(name)
    l, n0 = prob.inp.l_ini, prob.inp.n0_ini
    c = prob.eigvec(l, n0)
    r, u = prob.write_wf(c)
    U = prob.wavefunctions(l, 1, n0, 1, r=r, deriv=False)[0, 0]
    err, bound = float(np.max(np.abs(U - u))), 8 * prob.k * EPS * float(np.max(np.abs(c)))
    note("wavefunctions %s vs write_wf: max diff %.3g, bound %.3g" % (name, err, bound))
    assert err <= bound
    # the vector of wavefunctions is bspatom_eigvecs' (bspatom_eigvec may hand out the one computed early, beside the solve, from
    # the pencil's own eigenvalue: the same state, other last bits)
    assert np.array_equal(U, prob.tabulate(prob.eigvecs(l, n0, 1), r=r, deriv=False)[0])
    rows, idx = g["wf_rows"], g["wf_idx"]
    sgn = np.sign(np.dot(U[idx], rows[:, 1]))
    err = float(np.max(np.abs(sgn * U[idx] - rows[:, 1])) / np.max(np.abs(rows[:, 1])))
    note("wavefunctions %s vs the reference's wf_n0.dat: %.3g of max|u|" % (name, err))
    assert err <= 2e-8
    prob.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lin256", "c1_exp"])
def test_quadrature_identities(name):
    """States 1 .. 32 of the pairs (0, 1) and (1, 2).  On the assembly's points sum_p w u_i u_j is c_i^T S c_j: within 1e-9 of
    delta_ij (the project's bar for Z S Z^T).  radial_matrix with g = r, g = 1/r and g = 1 with deriv against dipole_matrix with
    a = (1,0,0), (0,1,0), (0,0,1): within 1e-12 max|D| -- the same identities evaluated on the CPU from LAPACK vectors gave at most
    2.5e-14 (c1_exp), the bar is 40 times that."""
    prob, cfg, rt, aind, xg, wg = solved(name, 3, l_fin=2)
    pairs, cnt = [(0, 1), (1, 2)], 32
    r, w = prob.quadrature()
    U = prob.wavefunctions(0, 3, 1, cnt, deriv=False)
    for l in range(3):
        G = (U[l] * w) @ U[l].T
        err = float(np.max(np.abs(G - np.eye(cnt))))
        note("wavefunctions %s l = %d: max |sum w u_i u_j - delta_ij| = %.3g" % (name, l, err))
        assert err < 1e-9
    for tag, g, deriv, a in (("r", lambda x: x, False, [1.0, 0.0, 0.0]), ("1/r", lambda x: 1.0 / x, False, [0.0, 1.0, 0.0]),
                             ("d/dr", lambda x: np.ones_like(x), True, [0.0, 0.0, 1.0])):
        D = prob.dipole_matrix(pairs, 1, cnt, 1, cnt, a)
        R = host.radial_matrix(prob, pairs, g, 1, cnt, 1, cnt, deriv=deriv)
        assert R.shape == D.shape
        err = float(np.max(np.abs(R - D)) / np.max(np.abs(D)))
        note("radial_matrix %s g = %s vs dipole_matrix: %.3g of max|D| = %.3g" % (name, tag, err, np.max(np.abs(D))))
        assert err <= 1e-12
    Rarr = host.radial_matrix(prob, pairs, r, 1, cnt, 1, cnt)       # g as an array on the grid
    assert np.array_equal(Rarr, host.radial_matrix(prob, pairs, lambda x: x, 1, cnt, 1, cnt))
    prob.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_wavefunction_argument_checks():
    prob, cfg, rt, aind, xg, wg = solved("c1_lin")
    nch, n = prob.lmax + 1, prob.nfun
    ra, rb = rt[0], rt[-1]
    nr = prob.quadrature()[0].size
    L = capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    Z = np.ones((2, n)); pts = np.array([ra, 0.5 * (ra + rb), rb])
    U = np.zeros(2 * max(nr, 3)); dU = np.zeros_like(U)
    Zd, Ud, dUd = dev(Z), nan_dev(U.size), nan_dev(U.size)
    nrc = C.c_int(0)
    assert L.bspatom_quadrature(prob._h, C.byref(nrc), None, None) == 0 and nrc.value == nr
    assert L.bspatom_quadrature(None, C.byref(nrc), None, None) == -2
    assert L.bspatom_quadrature(prob._h, None, None, None) == -2
    below, above, nanp = pts.copy(), pts.copy(), pts.copy()
    below[1] = ra - 1e-9 - abs(ra) * 1e-12; above[2] = np.nextafter(rb, np.inf); nanp[0] = np.nan
    infp = pts.copy(); infp[1] = np.inf
    for fn, z, u, du in ((L.bspatom_tabulate, p_(Z), p_(U), p_(dU)),
                         (L.bspatom_tabulate_dev, C.c_void_p(Zd.data_ptr()), C.c_void_p(Ud.data_ptr()), C.c_void_p(dUd.data_ptr()))):
        assert fn(prob._h, 2, z, 3, p_(pts), u, du) == 0
        assert fn(prob._h, 2, z, 3, p_(pts), u, None) == 0
        assert fn(prob._h, 2, z, nr, None, u, du) == 0
        assert fn(None, 2, z, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 2, None, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 2, z, 3, p_(pts), None, du) == -2
        assert fn(prob._h, 0, z, 3, p_(pts), u, du) == -2                 # nvec < 1
        assert fn(prob._h, 2, z, 0, p_(pts), u, du) == -2                 # npts < 1
        assert fn(prob._h, 2, z, nr - 1, None, u, du) == -2               # r == NULL with npts != nr
        assert fn(prob._h, 2, z, nr + 1, None, u, du) == -2
        for bad in (below, above, nanp, infp):
            assert fn(prob._h, 2, z, 3, p_(bad), u, du) == -2
    for fn, u, du in ((L.bspatom_wavefunctions, p_(U), p_(dU)),
                      (L.bspatom_wavefunctions_dev, C.c_void_p(Ud.data_ptr()), C.c_void_p(dUd.data_ptr()))):
        assert fn(prob._h, 0, 1, 1, 2, 3, p_(pts), u, du) == 0
        assert fn(prob._h, 0, 1, 1, 2, nr, None, u, None) == 0
        assert fn(None, 0, 1, 1, 2, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 0, 1, 1, 2, 3, p_(pts), None, du) == -2
        assert fn(prob._h, 0, 1, 1, 2, 0, p_(pts), u, du) == -2           # npts < 1
        assert fn(prob._h, 0, 1, 1, 2, nr - 1, None, u, du) == -2
        for bad in (below, above, nanp):
            assert fn(prob._h, 0, 1, 1, 2, 3, p_(bad), u, du) == -2
        assert fn(prob._h, nch, 1, 1, 2, 3, p_(pts), u, du) == -2         # a channel outside the last solve
        assert fn(prob._h, -1, 1, 1, 2, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 0, nch + 1, 1, 2, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 0, 0, 1, 2, 3, p_(pts), u, du) == -2           # nl < 1
        assert fn(prob._h, 0, 1, 0, 2, 3, p_(pts), u, du) == -2           # a window outside 1 .. nfun
        assert fn(prob._h, 0, 1, n, 2, 3, p_(pts), u, du) == -2
        assert fn(prob._h, 0, 1, 1, 0, 3, p_(pts), u, du) == -2           # count < 1
    with pytest.raises(capi.BspAtomError) as ei:
        prob.wavefunctions(0, 1, 1, 1, r=[rb + 1.0])
    assert ei.value.code == -2
    prob.assemble(0, nch)                                               # invalidates the state of the last solve
    for fn, u, du in ((L.bspatom_wavefunctions, p_(U), p_(dU)),
                      (L.bspatom_wavefunctions_dev, C.c_void_p(Ud.data_ptr()), C.c_void_p(dUd.data_ptr()))):
        assert fn(prob._h, 0, 1, 1, 2, 3, p_(pts), u, du) == -2
    assert L.bspatom_tabulate(prob._h, 2, p_(Z), 3, p_(pts), p_(U), p_(dU)) == 0      # needs no solve
    prob.close()


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_wavefunctions_at_c4_size():
    """C4 grid (n = 4096, k = 9, 49 080 quadrature points), 4 channels solved, states 1 .. 64, wavefunctions_dev with u and u'
    (201 MB): three sampled vectors bit-equal to the restatement applied to eigvecs_batch's vectors; tabulate_dev of 64
    device-resident vectors takes less wall time than 64 write_wf calls on the same vectors at npts + 1 uniform points (only
    'faster' is asserted; the ratio is logged)."""
    prob, cfg, rt, aind, xg, wg = solved("c4_4096", 4, l_fin=3)
    nl, cnt = 4, 64
    rq, _ = quadrature_ref(rt, xg, wg)
    npts = rq.size
    assert npts == prob.nointv * prob.ka == 49080
    Ud = torch.empty((nl, cnt, npts), dtype=torch.float64, device="cuda:0")
    dUd = torch.empty((nl, cnt, npts), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert prob.wavefunctions_dev(0, nl, 1, cnt, Ud.data_ptr(), dUd.data_ptr()) == npts
    Z = prob.eigvecs_batch(0, nl, 1, cnt)
    basis = basis_ref(cfg, rt, aind, rq)
    for c, j in ((0, 0), (2, 31), (3, 63)):
        Uref, dUref = tabulate_ref(prob.k, Z[c, j], basis)
        assert np.array_equal(Ud[c, j].cpu().numpy(), Uref[0]), (c, j)
        assert np.array_equal(dUd[c, j].cpu().numpy(), dUref[0]), (c, j)
    Zd = dev(Z[1])
    Ut = torch.empty((cnt, npts), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    prob.tabulate_dev(cnt, Zd.data_ptr(), Ut.data_ptr(), None)          # the first launches outside the timing
    prob.write_wf(Z[1, 0], npts)
    t0 = time.perf_counter()
    prob.tabulate_dev(cnt, Zd.data_ptr(), Ut.data_ptr(), None)
    t_call = time.perf_counter() - t0
    t0 = time.perf_counter()
    for j in range(cnt):
        prob.write_wf(Z[1, j], npts)
    t_loop = time.perf_counter() - t0
    assert np.array_equal(Ut.cpu().numpy(), Ud[1].cpu().numpy())
    note("tabulate_dev c4_4096, 64 vectors x %d points: one call %.3f ms, 64 write_wf calls %.2f ms, x%.1f"
         % (npts, 1e3 * t_call, 1e3 * t_loop, t_loop / t_call))
    assert t_call < t_loop, (t_call, t_loop)
    prob.close()
