"""u(r), u'(r) of blocks of states (bspatom_quadrature / bspatom_tabulate / bspatom_wavefunctions, csrc/wavefn.hip) without a
GPU: the entry points are bound, the kernels are in the library with no scratch and no spilled VGPRs at every order, the
quadrature rule gives nointv*ka points on every committed input, and host.write_wf_states / host.radial_matrix do what they
say against a stand-in problem.

This file also holds the CPU restatement the GPU tests (test_gpu_wavefunctions.py) compare with bit for bit:
  quadrature_ref   r = (rt[i+1]+rt[i])/2 + xg*((rt[i+1]-rt[i])/2), w = f2*wg on the intervals with rt[i+1] > rt[i]
  basis_ref        BSPALL at every point (oracle.lib().orc_bspall: interv + two bsplvb recurrences, compiled without FMA)
  tabulate_ref     U = U + c_j * B[:, jf] for jf = 1 .. k in this order from 0.0, c_j = 0 outside 1 .. nfun"""
import ctypes as C
import glob
import os
import sys
import numpy as np
import pytest
from conftest import ROOT, GOLDEN

import oracle as orc
from bspatom_amd import capi, host
from bspatom_amd.namelist import read_namelists

NEW = ("bspatom_quadrature", "bspatom_tabulate", "bspatom_tabulate_dev", "bspatom_wavefunctions", "bspatom_wavefunctions_dev")


# ---- the restatement ------------------------------------------------------------------------------------------------
def case_kw(name, **over):
    nl = read_namelists(open(os.path.join(GOLDEN, "inputs", name + ".inp")).read())
    kw = {}
    kw.update(nl["vars_bsp"]); kw.update(nl["vars_tise"]); kw.update(over)
    return {k.lower(): v for k, v in kw.items()}


def quadrature_ref(rt, xg, wg):
    r, w = [], []
    for i in range(len(rt) - 1):
        if rt[i + 1] > rt[i]:
            f1 = (rt[i + 1] + rt[i]) / 2.0
            f2 = (rt[i + 1] - rt[i]) / 2.0
            r.append(f1 + xg * f2)
            w.append(f2 * wg)
    return np.concatenate(r), np.concatenate(w)


def basis_ref(cfg, rt, aind, r):
    """B[ip, jf], dB[ip, jf] (jf < k) and left[ip] (1-based) of BSPALL at the points r"""
    L = orc.lib()
    f = L.orc_bspall
    f.argtypes = [C.POINTER(orc.OrcCfg), C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    r = np.ascontiguousarray(r, dtype=np.float64)
    k = cfg.k
    B = np.zeros((r.size, k)); dB = np.zeros((r.size, k)); left = np.zeros(r.size, dtype=np.int64)
    lf = C.c_int(0)
    prt, pa = rt.ctypes.data_as(C.c_void_p), aind.ctypes.data_as(C.c_void_p)
    for ip in range(r.size):
        st = f(C.byref(cfg), prt, pa, float(r[ip]), C.byref(lf), B[ip].ctypes.data_as(C.c_void_p), dB[ip].ctypes.data_as(C.c_void_p))
        assert st == 0, (ip, r[ip], st)
        left[ip] = lf.value
    return B, dB, left


def tabulate_ref(k, Z, basis):
    """U[v, ip], dU[v, ip] from the rows of Z (nvec, nfun) and basis = basis_ref(...): the ordered sum"""
    B, dB, left = basis
    Z = np.atleast_2d(Z)
    nfun = Z.shape[1]
    U = np.zeros((Z.shape[0], left.size)); dU = np.zeros_like(U)
    for jf in range(1, k + 1):
        j = jf + (left - k)                                        # 1-based function index per point
        ok = (j >= 1) & (j <= nfun)
        c = np.where(ok[None, :], Z[:, np.clip(j - 1, 0, nfun - 1)], 0.0)
        U = U + c * B[None, :, jf - 1]
        dU = dU + c * dB[None, :, jf - 1]
    return U, dU


# ---- 1 ----------------------------------------------------------------------------------------------------------------
def test_wavefunction_entry_points_bound():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
    for m in ("quadrature", "tabulate", "tabulate_dev", "wavefunctions", "wavefunctions_dev"):
        assert hasattr(capi.Problem, m), m
    assert hasattr(host, "write_wf_states") and hasattr(host, "radial_matrix")
    capi.set_option("wf_stage_mb", 3)
    assert capi.get_option("wf_stage_mb") == 3
    capi.set_option("wf_stage_mb", 0)


def test_wavefunction_kernels_in_library_without_scratch_or_spills():
    """basis_table_kernel<K> for K = 1 .. 16, tabulate_kernel<K, DERIV> for both DERIV, and the gather of the quadrature grid in
    the code-object notes of libbspatom.so: private segment 0, VGPR spills 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    for key, inst in (("basis_table_kernel", 16), ("tabulate_kernel", 32), ("basis_gather_kernel", 1)):
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == inst, (key, sorted(n for n in ks if "basis_" in n or "tabulate" in n))
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
ALL_INPUTS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "inputs", "*.inp")))


@pytest.mark.parametrize("name", ALL_INPUTS)
def test_quadrature_rule_has_nointv_ka_points(name):
    """The rule of bspatom_quadrature on the host's own knots and Gauss-Legendre rule (bspatom_host_setup): ka points per
    interval of positive width = nointv*ka on every committed input (WFALL's nr, TorusFuns.f90:87), ascending, inside
    (ra, rb), weights positive; and the oracle's grid gives the same bits."""
    assert "bspatom_quadrature" in capi.EXPORTS
    kw = case_kw(name)
    s, rt, aind, xg, wg = capi.host_setup(capi.make_input(**kw))
    r, w = quadrature_ref(rt, xg, wg)
    assert r.size == s.nointv * s.ka, (r.size, s.nointv, s.ka)
    assert np.all(np.diff(r) > 0) and r[0] > rt[0] and r[-1] < rt[-1]
    assert np.all(w > 0)
    cfg = orc.make_cfg(**kw)
    rto, _, xgo, wgo = orc.grid(cfg)
    ro, wo = quadrature_ref(rto, xgo, wgo)
    assert np.array_equal(ro, r) and np.array_equal(wo, w)


def test_restatement_reproduces_the_oracle_write_wf():
    """tabulate_ref at WRITE_WF's points equals the oracle's orc_write_wf bit for bit (both are the ordered no-FMA sum), and
    its derivative column is the basis derivative the assembly uses: the restatement the GPU tests rely on is WFALL's."""
    assert hasattr(capi.Problem, "tabulate")
    kw = case_kw("n65_k4")
    cfg = orc.make_cfg(**kw)
    rt, aind, xg, wg = orc.grid(cfg)
    c = np.random.default_rng(3).standard_normal(cfg.nfun)
    r, u = orc.write_wf(cfg, rt, c, npts=500)
    U, dU = tabulate_ref(cfg.k, c, basis_ref(cfg, rt, aind, r))
    assert np.array_equal(U[0], u)
    h = 1e-6                                                     # u' against a central difference of u, away from the knots
    rm = r[1:-1][np.min(np.abs(r[1:-1, None] - rt[None, :]), axis=1) > 2 * h]
    Up = tabulate_ref(cfg.k, c, basis_ref(cfg, rt, aind, rm + h))[0][0]
    Um = tabulate_ref(cfg.k, c, basis_ref(cfg, rt, aind, rm - h))[0][0]
    dUm = tabulate_ref(cfg.k, c, basis_ref(cfg, rt, aind, rm))[1][0]
    assert np.max(np.abs((Up - Um) / (2 * h) - dUm)) < 1e-6 * max(1.0, np.max(np.abs(dUm)))


# ---- 3 ----------------------------------------------------------------------------------------------------------------
class _Inp:
    ra, rb = 0.5, 40.5


class _FakeProblem:
    """stands in for capi.Problem: 30 quadrature points, u_{l,n}(r) = cos((n + l/4) r), u' its derivative"""
    inp = _Inp()

    def __init__(self):
        self.calls = []
        self.r = np.linspace(0.6, 40.4, 30)
        self.w = np.linspace(0.5, 2.0, 30)

    def quadrature(self):
        return self.r.copy(), self.w.copy()

    def wavefunctions(self, l0, nl, n0, count, r=None, deriv=True):
        self.calls.append((l0, nl, n0, count, None if r is None else np.array(r), deriv))
        r = self.r if r is None else np.asarray(r)
        q = np.array([[n0 + j + 0.25 * (l0 + c) for j in range(count)] for c in range(nl)])[:, :, None]
        U = np.cos(q * r[None, None, :]); dU = -q * np.sin(q * r[None, None, :])
        return (U, dU) if deriv else U


def test_write_wf_states_files_format_and_one_call(tmp_path):
    prob = _FakeProblem()
    npts = 40
    paths = host.write_wf_states(str(tmp_path), prob, 2, 3, 4, npts=npts)
    assert [os.path.basename(p) for p in paths] == ["wf_l2_n%d.dat" % n for n in (3, 4, 5, 6)]
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths)
    assert len(prob.calls) == 1
    l0, nl, n0, count, r, deriv = prob.calls[0]
    assert (l0, nl, n0, count, deriv) == (2, 1, 3, 4, False)
    rr = 0.5 + np.arange(npts + 1) * ((40.5 - 0.5) / npts)          # WRITE_WF: r_i = ra + i*(rb-ra)/npts
    assert np.array_equal(r, rr)
    U = prob.wavefunctions(2, 1, 3, 4, r=rr, deriv=False)[0]
    for j, p in enumerate(paths):
        lines = open(p).read().split("\n")
        assert lines[-1] == "" and len(lines) == npts + 2          # npts + 1 records
        for i, line in enumerate(lines[:-1]):
            assert len(line) == 40                                  # '(2G20.10)'
            assert line == host.fortran_g(float(rr[i]), 20, 10) + host.fortran_g(float(U[j, i]), 20, 10)
        val = np.array([[float(x) for x in line.split()] for line in lines[:-1]])
        assert np.allclose(val[:, 0], rr, rtol=1e-9, atol=0) and np.allclose(val[:, 1], U[j], rtol=1e-9, atol=1e-300)


def test_radial_matrix_against_direct_sums():
    prob = _FakeProblem()
    pairs = [(0, 1), (1, 0), (1, 2), (0, 1)]
    r, w = prob.quadrature()
    for deriv in (False, True):
        for g in (lambda x: 1.0 / x, r * r):
            prob.calls.clear()
            D = host.radial_matrix(prob, pairs, g, 2, 3, 1, 5, deriv=deriv)
            assert D.shape == (4, 3, 5)
            calls = list(prob.calls)
            gv = g(r) if callable(g) else g
            for p, (li, lf) in enumerate(pairs):
                Ui, dUi = prob.wavefunctions(li, 1, 2, 3)
                Uf = prob.wavefunctions(lf, 1, 1, 5, deriv=False)
                X = (dUi if deriv else Ui)[0]
                want = np.einsum("q,iq,fq->if", w * gv, X, Uf[0])
                assert np.allclose(D[p], want, rtol=1e-13, atol=1e-13 * np.max(np.abs(want)))
            assert np.array_equal(D[3], D[0])
            # one table per distinct channel and role, every one on the quadrature grid
            assert sorted((c[0], c[2], c[3], c[5]) for c in calls) == sorted(
                [(0, 2, 3, deriv), (1, 2, 3, deriv), (1, 1, 5, False), (0, 1, 5, False), (2, 1, 5, False)])
            assert all(c[1] == 1 and c[4] is None for c in calls)
    with pytest.raises(ValueError):
        host.radial_matrix(prob, pairs, np.ones(7), 1, 1, 1, 1)
