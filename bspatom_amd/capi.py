"""ctypes binding of libbspatom.so (include/bspatom.h).  No torch, no numpy fallbacks: if the
shared library or a gfx950 device is missing the calls fail loudly (there is no CPU path)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbspatom.so")

ERRORS = {-1: "HIP runtime error", -2: "invalid argument", -3: "FATAL ERROR - BSPLVB",
          -4: "no gfx950 device (libbspatom has no CPU path)", -5: "unsupported"}


class BspAtomError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        super().__init__("%s failed: %s (code %d)" % (where or "libbspatom", ERRORS.get(code, "error"), code))


class Input(C.Structure):
    _fields_ = [("kind_grid", C.c_int32), ("k", C.c_int32), ("ka", C.c_int32), ("nfun", C.c_int32),
                ("kind_bc1", C.c_int32), ("kind_bc2", C.c_int32),
                ("ra", C.c_double), ("rb", C.c_double), ("rmax", C.c_double),
                ("n0_ini", C.c_int32), ("l_ini", C.c_int32), ("m_ini", C.c_int32), ("l_fin", C.c_int32),
                ("lmax", C.c_int32), ("kind_pot", C.c_int32),
                ("emax_fin", C.c_double), ("zatom", C.c_double)]


class Sizes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nfun", "k", "ka", "nkp", "nointv", "nbc1", "nbc2", "lmax",
                                         "nintv_exp", "nintv_lin", "npad")]


EXPORTS = ["bspatom_input_defaults", "bspatom_device_count", "bspatom_host_setup", "bspatom_problem_create", "bspatom_problem_destroy",
           "bspatom_problem_sizes", "bspatom_problem_grid", "bspatom_problem_route", "bspatom_assemble", "bspatom_solve", "bspatom_solve_dev",
           "bspatom_eigvec", "bspatom_eigvecs", "bspatom_eigvecs_batch", "bspatom_eigvecs_batch_dev", "bspatom_dipole_bands", "bspatom_dipole_elements", "bspatom_dipole_matrix", "bspatom_dipole_matrix_dev",
           "bspatom_operator_bands", "bspatom_operator_bands_dev", "bspatom_operator_matrix", "bspatom_operator_matrix_dev", "bspatom_resolvent", "bspatom_resolvent_dev", "bspatom_resolvent_chain", "bspatom_resolvent_chain_dev", "bspatom_resolvent_coupled", "bspatom_resolvent_coupled_dev", "bspatom_resolvent_coupled_wide", "bspatom_resolvent_coupled_wide_dev", "bspatom_write_wf", "bspatom_quadrature", "bspatom_tabulate", "bspatom_tabulate_dev", "bspatom_wavefunctions", "bspatom_wavefunctions_dev", "bspatom_tdse_propagate", "bspatom_tdse_propagate_dev", "bspatom_tdse_observe", "bspatom_tdse_observe_dev", "bspatom_tdse_lawson", "bspatom_tdse_lawson_dev", "bspatom_tdse_static", "bspatom_tdse_static_dev", "bspatom_tdse_fields", "bspatom_tdse_fields_dev", "bspatom_tdse_adaptive", "bspatom_tdse_adaptive_dev", "bspatom_last_timing", "bspatom_early_vector_state", "bsp_dsygv_", "bspatom_stage_gemm",
           "bspatom_stage_standard_form", "bspatom_stage_sy2sb", "bspatom_stage_panel", "bspatom_stage_sb2st", "bspatom_stage_sb2sb", "bspatom_stage_bisect", "bspatom_stage_crawford", "bspatom_stage_band_eigenvalue",
           "bspatom_release_scratch", "bspatom_run_token", "bspatom_comm_create", "bspatom_comm_allgather", "bspatom_comm_collectives", "bspatom_comm_destroy",
           "bspatom_set_option", "bspatom_get_option", "bspatom_kernel_times", "bspatom_kernel_slot_name"]

# what include/bspatom_tdse_spline.h, the part of the header for the spline-basis TDSE, declares (EXPORTS is include/bspatom.h's own text)
SPLINE_EXPORTS = ["bspatom_tdse_spline", "bspatom_tdse_spline_dev", "bspatom_tdse_spline_wide", "bspatom_tdse_spline_wide_dev"]

# what include/bspatom_tdse_split.h, the part of the header for the split-step spline-basis TDSE, declares
SPLIT_EXPORTS = ["bspatom_tdse_split", "bspatom_tdse_split_dev"]

# what include/bspatom_spline_expect.h, the part of the header for expectation values in the spline basis, declares
EXPECT_EXPORTS = ["bspatom_spline_expect", "bspatom_spline_expect_dev", "bspatom_tdse_split_observe", "bspatom_tdse_split_observe_dev"]

# what include/bspatom_spline_window.h, the part of the header for the window operator on spline packets, declares
WINDOW_EXPORTS = ["bspatom_spline_window", "bspatom_spline_window_dev"]
WINDOW_MAX_FAC = 8                          # BSPATOM_WINDOW_MAX_FAC

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libbspatom.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C bspatom_amd/csrc); there is no fallback implementation")
        L = C.CDLL(LIB_PATH)
        vp, i32, dbl, lng = C.c_void_p, C.c_int, C.c_double, C.c_long
        L.bspatom_input_defaults.argtypes = [C.POINTER(Input)]
        L.bspatom_input_defaults.restype = None
        L.bspatom_host_setup.argtypes = [C.POINTER(Input), C.POINTER(Sizes), vp, vp, vp, vp]
        L.bspatom_problem_create.argtypes = [C.POINTER(Input), i32, C.POINTER(vp)]
        L.bspatom_problem_destroy.argtypes = [vp]
        L.bspatom_problem_destroy.restype = None
        L.bspatom_problem_sizes.argtypes = [vp, C.POINTER(Sizes)]
        L.bspatom_problem_grid.argtypes = [vp, vp, vp, vp, vp]
        L.bspatom_problem_route.argtypes = [vp]
        L.bspatom_assemble.argtypes = [vp, i32, i32, vp, vp]
        L.bspatom_solve.argtypes = [vp, i32, i32, vp, vp]
        L.bspatom_solve_dev.argtypes = [vp, i32, i32, vp, vp]
        L.bspatom_eigvec.argtypes = [vp, i32, i32, vp]
        L.bspatom_eigvecs.argtypes = [vp, i32, i32, i32, vp]
        L.bspatom_eigvecs_batch.argtypes = [vp, i32, i32, i32, i32, vp]
        L.bspatom_eigvecs_batch_dev.argtypes = [vp, i32, i32, i32, i32, vp]
        L.bspatom_dipole_elements.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
        L.bspatom_dipole_matrix.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]
        L.bspatom_dipole_matrix_dev.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]
        L.bspatom_dipole_bands.argtypes = [vp, vp]
        L.bspatom_operator_bands.argtypes = [vp, i32, vp, vp, vp]
        L.bspatom_operator_bands_dev.argtypes = [vp, i32, vp, vp, vp]
        L.bspatom_operator_matrix.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]
        L.bspatom_operator_matrix_dev.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp]
        L.bspatom_resolvent.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.bspatom_resolvent_dev.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.bspatom_resolvent_chain.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.bspatom_resolvent_chain_dev.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.bspatom_resolvent_coupled.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.bspatom_resolvent_coupled_dev.argtypes = list(L.bspatom_resolvent_coupled.argtypes)
        L.bspatom_resolvent_coupled_wide.argtypes = list(L.bspatom_resolvent_coupled.argtypes)
        L.bspatom_resolvent_coupled_wide_dev.argtypes = list(L.bspatom_resolvent_coupled.argtypes)
        L.bspatom_write_wf.argtypes = [vp, vp, i32, vp, vp]
        L.bspatom_quadrature.argtypes = [vp, C.POINTER(i32), vp, vp]
        L.bspatom_tabulate.argtypes = [vp, i32, vp, i32, vp, vp, vp]
        L.bspatom_tabulate_dev.argtypes = [vp, i32, vp, i32, vp, vp, vp]
        L.bspatom_wavefunctions.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp]
        L.bspatom_wavefunctions_dev.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp]
        # the TDSE calls: propagate's 16 arguments, + obs_every, obs, + scheme and the static lists, + what fields and adaptive add
        t16 = [vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, dbl, vp, vp, i32, vp, vp]
        t18 = t16 + [i32, vp]
        t24 = t18 + [i32, i32, vp, vp, vp, vp]
        for name, types in (("propagate", t16), ("observe", t18), ("lawson", t18), ("static", t24), ("fields", t24 + [i32, vp]),
                            ("adaptive", t24 + [i32, dbl, i32, i32, vp, i32, vp, vp, vp])):
            getattr(L, "bspatom_tdse_" + name).argtypes = list(types)
            getattr(L, "bspatom_tdse_" + name + "_dev").argtypes = list(types)
        L.bspatom_tdse_spline.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, i32, dbl, vp, vp, i32, vp, i32, i32, vp, vp, vp]
        L.bspatom_tdse_spline_dev.argtypes = list(L.bspatom_tdse_spline.argtypes)
        L.bspatom_tdse_spline_wide.argtypes = list(L.bspatom_tdse_spline.argtypes)
        L.bspatom_tdse_spline_wide_dev.argtypes = list(L.bspatom_tdse_spline.argtypes)
        L.bspatom_tdse_split.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, dbl, vp, vp, i32, vp, i32, i32, vp, vp, vp]
        L.bspatom_tdse_split_dev.argtypes = list(L.bspatom_tdse_split.argtypes)
        L.bspatom_spline_expect.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        L.bspatom_spline_expect_dev.argtypes = list(L.bspatom_spline_expect.argtypes)
        L.bspatom_tdse_split_observe.argtypes = L.bspatom_tdse_split.argtypes + [i32, vp, vp]
        L.bspatom_spline_window.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
        L.bspatom_spline_window_dev.argtypes = list(L.bspatom_spline_window.argtypes)
        L.bspatom_tdse_split_observe_dev.argtypes = list(L.bspatom_tdse_split_observe.argtypes)
        L.bspatom_last_timing.argtypes = [vp, vp]
        L.bspatom_early_vector_state.argtypes = [vp, vp]
        L.bspatom_stage_gemm.argtypes = [i32, i32, i32, i32, vp, lng, lng, lng, lng, vp, lng, lng, lng, lng,
                                         vp, lng, lng, lng, lng, dbl, dbl]
        L.bspatom_stage_standard_form.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        L.bspatom_stage_sy2sb.argtypes = [i32, i32, vp, vp]
        L.bspatom_stage_sb2st.argtypes = [i32, i32, i32, vp, vp, vp]
        L.bspatom_stage_panel.argtypes = [i32, i32, i32, vp, vp, vp]
        L.bspatom_stage_sb2sb.argtypes = [i32, i32, i32, vp]
        L.bspatom_stage_bisect.argtypes = [i32, i32, vp, vp, vp]
        L.bspatom_stage_crawford.argtypes = [i32, i32, i32, vp, vp, vp, vp]
        L.bspatom_stage_band_eigenvalue.argtypes = [i32, i32, vp, vp, i32, vp]
        L.bsp_dsygv_.restype = None
        L.bspatom_set_option.argtypes = [C.c_char_p, i32]
        L.bspatom_get_option.argtypes = [C.c_char_p, C.POINTER(i32)]
        L.bspatom_kernel_times.argtypes = [vp, vp, i32]
        L.bspatom_kernel_slot_name.argtypes = [i32]
        L.bspatom_kernel_slot_name.restype = C.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptr(x):
    """a pointer argument from a host array, a device address (0: NULL) or None"""
    if x is None or isinstance(x, np.ndarray):
        return _p(x)
    return C.c_void_p(x) if x else None


def _chk(rc, where):
    if rc != 0:
        raise BspAtomError(rc, where)


def make_input(**kw):
    inp = Input()
    lib().bspatom_input_defaults(C.byref(inp))
    names = {f[0] for f in Input._fields_}
    for key, v in kw.items():
        key = key.lower()
        if key in names:
            setattr(inp, key, v)
    return inp


def host_setup(inp, arrays=True):
    """READ_INPUTS sizes and GRID/gauleg arrays, computed on the host (works without a GPU)."""
    s = Sizes()
    _chk(lib().bspatom_host_setup(C.byref(inp), C.byref(s), None, None, None, None), "bspatom_host_setup")
    if not arrays:
        return s
    rt = np.zeros(s.nkp); aind = np.zeros(2 * s.nfun); xg = np.zeros(s.ka); wg = np.zeros(s.ka)
    _chk(lib().bspatom_host_setup(C.byref(inp), C.byref(s), _p(rt), _p(aind), _p(xg), _p(wg)), "bspatom_host_setup")
    return s, rt, aind, xg, wg


class Problem:
    """One B-spline radial problem resident on one MI355X (wraps bspatom_problem)."""

    def __init__(self, inp, device=0):
        self._h = C.c_void_p()
        _chk(lib().bspatom_problem_create(C.byref(inp), device, C.byref(self._h)), "bspatom_problem_create")
        s = Sizes()
        _chk(lib().bspatom_problem_sizes(self._h, C.byref(s)), "bspatom_problem_sizes")
        self.sizes = s
        self.inp = inp
        for n, _ in Sizes._fields_:
            setattr(self, n, getattr(s, n))

    def close(self):
        if self._h:
            lib().bspatom_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def grid(self):
        rt = np.zeros(self.nkp); aind = np.zeros(2 * self.nfun); xg = np.zeros(self.ka); wg = np.zeros(self.ka)
        _chk(lib().bspatom_problem_grid(self._h, _p(rt), _p(aind), _p(xg), _p(wg)), "bspatom_problem_grid")
        return rt, aind, xg, wg

    def assemble(self, l0, nl):
        SB = np.zeros((self.k, self.nfun)); HB = np.zeros((nl, self.k, self.nfun))
        _chk(lib().bspatom_assemble(self._h, l0, nl, _p(SB), _p(HB)), "bspatom_assemble")
        return SB, HB

    def solve(self, l0, nl):
        E = np.zeros((nl, self.nfun)); info = np.zeros(nl, dtype=np.int32)
        _chk(lib().bspatom_solve(self._h, l0, nl, _p(E), _p(info)), "bspatom_solve")
        self.last_E, self.last_l0 = E, l0              # host.tdse_system takes the eigenvalues of its channels from here
        return E, info

    def solve_dev(self, l0, nl, dev_ptr):
        info = np.zeros(nl, dtype=np.int32)
        _chk(lib().bspatom_solve_dev(self._h, l0, nl, C.c_void_p(dev_ptr), _p(info)), "bspatom_solve_dev")
        return info

    def eigvec(self, l, n0):
        c = np.zeros(self.nfun)
        _chk(lib().bspatom_eigvec(self._h, l, n0, _p(c)), "bspatom_eigvec")
        return c

    def dipole_bands(self):
        """Full bands (3, 2k-1, nfun) of int B_i r B_j, int B_i (1/r) B_j, int B_i B_j' (rij of KIND_PI = 1, 2)."""
        RB = np.zeros((3, 2 * self.k - 1, self.nfun))
        _chk(lib().bspatom_dipole_bands(self._h, _p(RB)), "bspatom_dipole_bands")
        return RB

    def eigvecs(self, l, n0, count):
        """Eigenvectors n0 .. n0+count-1 (1-based) of channel l: array (count, nfun), each S-normalised."""
        Z = np.zeros((count, self.nfun))
        _chk(lib().bspatom_eigvecs(self._h, l, n0, count, _p(Z)), "bspatom_eigvecs")
        return Z

    def eigvecs_batch(self, l0, nl, n0, count):
        """Eigenvectors n0 .. n0+count-1 (1-based) of channels l0 .. l0+nl-1 in one call: array (nl, count, nfun),
        [c] bit-identical to eigvecs(l0 + c, n0, count)."""
        Z = np.zeros((max(nl, 0), max(count, 0), self.nfun))
        _chk(lib().bspatom_eigvecs_batch(self._h, l0, nl, n0, count, _p(Z)), "bspatom_eigvecs_batch")
        return Z

    def eigvecs_batch_dev(self, l0, nl, n0, count, dev_ptr):
        """eigvecs_batch into device memory of this problem's device (nl * count * nfun doubles at dev_ptr, e.g. a torch
        tensor's data_ptr()), written in place; returns when the vectors are there."""
        _chk(lib().bspatom_eigvecs_batch_dev(self._h, l0, nl, n0, count, C.c_void_p(dev_ptr)), "bspatom_eigvecs_batch_dev")

    def dipole_elements(self, l_ini, n0_ini, l_fin, n0_fin, count, a):
        """D[i] = c(l_fin, n0_fin+i)^T (a[0] R_r + a[1] R_1/r + a[2] R_d/dr) c(l_ini, n0_ini), 1-based state numbers:
        the DGEMV + DDOT of TRANS_AMP (PhotoIon.f90:95-107) for channels of the last solved batch."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == (3,)
        D = np.zeros(count)
        _chk(lib().bspatom_dipole_elements(self._h, l_ini, n0_ini, l_fin, n0_fin, count, _p(a), _p(D)), "bspatom_dipole_elements")
        return D

    @staticmethod
    def _dipole_pairs(pairs, a):
        pr = np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2)
        li, lf = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (3,):
            a = np.broadcast_to(a, (len(pr), 3))
        assert a.shape == (len(pr), 3), a.shape
        return li, lf, np.ascontiguousarray(a)

    def dipole_matrix(self, pairs, n0_ini, count_ini, n0_fin, count_fin, a):
        """D[p, i, f] = c(l_fin, n0_fin+f)^T (a[p,0] R_r + a[p,1] R_1/r + a[p,2] R_d/dr) c(l_ini, n0_ini+i) for every
        (l_ini, l_fin) = pairs[p] in one call: array (npairs, count_ini, count_fin); row [p, i] is dipole_elements(l_ini,
        n0_ini + i, l_fin, n0_fin, count_fin, a[p]) up to the summation order.  a: (npairs, 3), or one triple for every pair."""
        li, lf, a = self._dipole_pairs(pairs, a)
        D = np.zeros((len(li), max(count_ini, 0), max(count_fin, 0)))
        _chk(lib().bspatom_dipole_matrix(self._h, len(li), _p(li), _p(lf), n0_ini, count_ini, n0_fin, count_fin, _p(a), _p(D)),
             "bspatom_dipole_matrix")
        return D

    def dipole_matrix_dev(self, pairs, n0_ini, count_ini, n0_fin, count_fin, a, dev_ptr):
        """dipole_matrix into device memory of this problem's device (npairs * count_ini * count_fin doubles at dev_ptr, e.g. a
        torch tensor's data_ptr()), written in place; returns when the block is there."""
        li, lf, a = self._dipole_pairs(pairs, a)
        _chk(lib().bspatom_dipole_matrix_dev(self._h, len(li), _p(li), _p(lf), n0_ini, count_ini, n0_fin, count_fin, _p(a),
                                             C.c_void_p(dev_ptr)), "bspatom_dipole_matrix_dev")

    def _nr(self):
        nr = C.c_int(0)
        _chk(lib().bspatom_quadrature(self._h, C.byref(nr), None, None), "bspatom_quadrature")
        return nr.value

    @staticmethod
    def _deriv(deriv, nop):
        deriv = np.ascontiguousarray(deriv, dtype=np.int32).reshape(-1)
        assert deriv.shape == (nop,), deriv.shape
        return deriv

    def _operators(self, g, deriv):
        """(nop, g as (nop, nr) float64, deriv as (nop,) int32) of host operator arguments"""
        g = np.ascontiguousarray(g, dtype=np.float64)
        g = g.reshape(-1, g.shape[-1]) if g.ndim else g.reshape(1, 1)
        assert g.shape[1] == self._nr(), (g.shape, self._nr())
        return g.shape[0], g, self._deriv(deriv, g.shape[0])

    @staticmethod
    def _operator_pairs(pairs, a, nop):
        pr = np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2)
        li, lf = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (nop,):
            a = np.broadcast_to(a, (len(pr), nop))
        assert a.shape == (len(pr), nop), a.shape
        return li, lf, np.ascontiguousarray(a)

    def operator_bands(self, g, deriv):
        """Full bands (nop, 2k-1, nfun) of G_o(i, j) = sum_q B_i(r_q) g[o, q] X_j(r_q) w_q on the quadrature grid (quadrature()),
        X = B_j (deriv[o] = 0) or B_j' (1): [o, d + k - 1, i] = G_o(i, i + d).  With g = (r, 1/r, 1), deriv = (0, 0, 1) these are
        dipole_bands() bit for bit.  g: (nop, nr) or (nr,)."""
        nop, g, deriv = self._operators(g, deriv)
        GB = np.zeros((nop, 2 * self.k - 1, self.nfun))
        _chk(lib().bspatom_operator_bands(self._h, nop, _p(g), _p(deriv), _p(GB)), "bspatom_operator_bands")
        return GB

    def operator_bands_dev(self, nop, g_ptr, deriv, GB_ptr):
        """operator_bands with g (nop * nr doubles at g_ptr) and the bands (nop * (2k-1) * nfun doubles at GB_ptr) in device memory
        of this problem's device, e.g. torch tensors' data_ptr(); written in place.  deriv is a host array."""
        _chk(lib().bspatom_operator_bands_dev(self._h, nop, C.c_void_p(g_ptr), _p(self._deriv(deriv, nop)), C.c_void_p(GB_ptr)),
             "bspatom_operator_bands_dev")

    def operator_matrix(self, pairs, g, deriv, n0_ini, count_ini, n0_fin, count_fin, a):
        """D[p, i, f] = c(l_fin, n0_fin+f)^T (sum_o a[p, o] G_o) c(l_ini, n0_ini+i) for every (l_ini, l_fin) = pairs[p] in one call,
        G_o the operator_bands of (g, deriv): array (npairs, count_ini, count_fin), the layout and the conventions of
        dipole_matrix.  a: (npairs, nop), or (nop,) for every pair."""
        nop, g, deriv = self._operators(g, deriv)
        li, lf, a = self._operator_pairs(pairs, a, nop)
        D = np.zeros((len(li), max(count_ini, 0), max(count_fin, 0)))
        _chk(lib().bspatom_operator_matrix(self._h, nop, _p(g), _p(deriv), len(li), _p(li), _p(lf), n0_ini, count_ini, n0_fin,
                                           count_fin, _p(a), _p(D)), "bspatom_operator_matrix")
        return D

    def operator_matrix_dev(self, pairs, nop, g_ptr, deriv, n0_ini, count_ini, n0_fin, count_fin, a, dev_ptr):
        """operator_matrix with g (nop * nr doubles at g_ptr) and D (npairs * count_ini * count_fin doubles at dev_ptr) in device
        memory of this problem's device, written in place; deriv and a are host arrays.  Returns when the block is there."""
        li, lf, a = self._operator_pairs(pairs, a, nop)
        _chk(lib().bspatom_operator_matrix_dev(self._h, nop, C.c_void_p(g_ptr), _p(self._deriv(deriv, nop)), len(li), _p(li), _p(lf),
                                               n0_ini, count_ini, n0_fin, count_fin, _p(a), C.c_void_p(dev_ptr)),
             "bspatom_operator_matrix_dev")

    @staticmethod
    def _resolvent_matrices(l, z, w, nabs):
        """(nmat, l as int32, z as complex128, w as int32 or None) with scalars broadcast to the longest of the three"""
        l, z = np.atleast_1d(np.asarray(l, dtype=np.int32)), np.atleast_1d(np.asarray(z, dtype=np.complex128))
        w = None if w is None else np.atleast_1d(np.asarray(w, dtype=np.int32))
        nmat = max(l.size, z.size, 1 if w is None else w.size)
        bc = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (nmat,)) if a.size == 1 else a)
        l, z, w = bc(l), bc(z), bc(w)
        assert l.shape == z.shape == (nmat,) and (w is None or w.shape == (nmat,)), (l.shape, z.shape)
        return nmat, l, z, w

    def resolvent(self, l, z, B, W=None, w=None, P=None, want_x=True):
        """Solves (H_l[m] - i W_w[m] - z[m] S) x = B[r] for every matrix m and right-hand side r in one call (bspatom_resolvent), and
        the projections R[m, r, q] = sum_i P[q, i] x[m, r, i] (bilinear, no conjugate).  l, z, w: scalars or arrays of one length
        (scalars broadcast); the channels are those of the last solve() or assemble().  B: (nrhs, nfun) or (nfun,), P: (nproj, nfun),
        (nfun,) or None, complex or real.  W: full bands (nabs, 2k-1, nfun) or (2k-1, nfun) as operator_bands returns them, or None;
        w[m] = -1 switches the absorber off for matrix m, w=None takes W[0] everywhere.  Returns (X, R, info): X (nmat, nrhs, nfun)
        complex128 or None (want_x False), R (nmat, nrhs, nproj) complex128 or None (P None), info (nmat,) replaced pivots (0)."""
        n = self.nfun
        B = np.ascontiguousarray(np.asarray(B, dtype=np.complex128).reshape(-1, n))
        P = None if P is None else np.ascontiguousarray(np.asarray(P, dtype=np.complex128).reshape(-1, n))
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        nabs = 0 if W is None else W.shape[0]
        nmat, l, z, w = self._resolvent_matrices(l, z, w, nabs)
        nrhs, nproj = B.shape[0], 0 if P is None else P.shape[0]
        X = np.zeros((nmat, nrhs, n), dtype=np.complex128) if want_x else None
        R = np.zeros((nmat, nrhs, nproj), dtype=np.complex128) if P is not None else None
        info = np.zeros(nmat, dtype=np.int32)
        _chk(lib().bspatom_resolvent(self._h, nmat, _p(l), _p(z), nabs, _p(W), _p(w), nrhs, _p(B), nproj, _p(P), _p(X), _p(R),
                                     _p(info)), "bspatom_resolvent")
        return X, R, info

    def resolvent_dev(self, l, z, nrhs, B_ptr, nabs=0, W_ptr=None, w=None, nproj=0, P_ptr=None, X_ptr=None, R_ptr=None):
        """resolvent with B (nrhs * nfun complex), W (nabs * (2k-1) * nfun doubles), P (nproj * nfun complex), X (nmat * nrhs * nfun
        complex) and R (nmat * nrhs * nproj complex) in device memory of this problem's device, e.g. torch tensors' data_ptr(); X and
        R are written in place (either pointer may be None).  l, z, w are host values as in resolvent.  Returns info."""
        nmat, l, z, w = self._resolvent_matrices(l, z, w, nabs)
        info = np.zeros(nmat, dtype=np.int32)
        vp = lambda a: None if a is None else C.c_void_p(a)
        _chk(lib().bspatom_resolvent_dev(self._h, nmat, _p(l), _p(z), nabs, vp(W_ptr), _p(w), nrhs, vp(B_ptr), nproj, vp(P_ptr),
                                         vp(X_ptr), vp(R_ptr), _p(info)), "bspatom_resolvent_dev")
        return info

    @staticmethod
    def _chain_stages(l, z, w, a, nop):
        """(nchain, nstage, l int32, z complex128, w int32 or None, a float64 or None), each (nchain, nstage) -- a (nchain, nstage-1,
        nop) -- and contiguous; l, z, w broadcast from (nstage,) or scalars, a from (nstage-1, nop) or, with one operator, (nstage-1,);
        a None with one operator means coefficient 1"""
        l, z = np.asarray(l, dtype=np.int32), np.asarray(z, dtype=np.complex128)
        w = None if w is None else np.asarray(w, dtype=np.int32)
        shape = np.broadcast_shapes(l.shape, z.shape, () if w is None else w.shape)
        assert len(shape) <= 2, shape
        nchain, nstage = (1,) * (2 - len(shape)) + tuple(shape)
        assert nstage >= 1, shape
        if nstage == 1:
            a = None
        else:
            assert nop >= 1, "a chain of more than one stage needs operator bands G"
            a = np.ones((nstage - 1, nop)) if a is None and nop == 1 else a
            assert a is not None, "a (nchain, nstage-1, nop) is needed with more than one operator"
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1 and nop == 1:
                a = a[:, None]
            if a.ndim == 3 and nchain == 1:
                nchain = a.shape[0]
            a = np.ascontiguousarray(np.broadcast_to(a, (nchain, nstage - 1, nop)))
        bc = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nchain, nstage)))
        return nchain, nstage, bc(l), bc(z), bc(w), a

    def resolvent_chain(self, l, z, B, G=None, a=None, W=None, w=None, P=None, want_x=True):
        """Chains of resolvents with an operator in between, every chain on the GPU from its first factorisation to its last
        projection in one call (bspatom_resolvent_chain): x[c, 0, r] = M[c, 0]^-1 B[r], x[c, s, r] = M[c, s]^-1 A[c, s] x[c, s-1, r],
        M[c, s] = H_l[c, s] - i W_w[c, s] - z[c, s] S, A[c, s] = sum_o a[c, s-1, o] G[o].  l, z, w: (nchain, nstage), broadcast from
        (nstage,) or scalars; G: full bands (nop, 2k-1, nfun) or (2k-1, nfun) as dipole_bands / operator_bands return them (None
        with one stage); a: real, (nchain, nstage-1, nop), broadcast from (nstage-1, nop), None with one operator: coefficient 1.
        B, W, P as in resolvent.  Returns (X, R, info): X (nchain, nrhs, nfun) complex128, the LAST stage's solutions, or None
        (want_x False); R (nchain, nstage, nrhs, nproj) complex128, sum_i P[q, i] x[c, s, r, i] of EVERY stage (bilinear), or None
        (P None); info (nchain, nstage) replaced pivots (0).  A chain cut to s+1 stages gives the same R, info of those stages bit
        for bit and x[c, s] as its X; one stage is resolvent bit for bit."""
        n = self.nfun
        B = np.ascontiguousarray(np.asarray(B, dtype=np.complex128).reshape(-1, n))
        P = None if P is None else np.ascontiguousarray(np.asarray(P, dtype=np.complex128).reshape(-1, n))
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        G = None if G is None else np.ascontiguousarray(np.asarray(G, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        nabs, nop = 0 if W is None else W.shape[0], 0 if G is None else G.shape[0]
        nchain, nstage, l, z, w, a = self._chain_stages(l, z, w, a, nop)
        nrhs, nproj = B.shape[0], 0 if P is None else P.shape[0]
        X = np.zeros((nchain, nrhs, n), dtype=np.complex128) if want_x else None
        R = np.zeros((nchain, nstage, nrhs, nproj), dtype=np.complex128) if P is not None else None
        info = np.zeros((nchain, nstage), dtype=np.int32)
        _chk(lib().bspatom_resolvent_chain(self._h, nchain, nstage, _p(l), _p(z), nabs, _p(W), _p(w), nop, _p(G), _p(a), nrhs, _p(B),
                                           nproj, _p(P), _p(X), _p(R), _p(info)), "bspatom_resolvent_chain")
        return X, R, info

    def resolvent_chain_dev(self, l, z, nrhs, B_ptr, nop=0, G_ptr=None, a=None, nabs=0, W_ptr=None, w=None, nproj=0, P_ptr=None,
                            X_ptr=None, R_ptr=None):
        """resolvent_chain with B (nrhs * nfun complex), G (nop * (2k-1) * nfun doubles), W (nabs * (2k-1) * nfun doubles), P (nproj *
        nfun complex), X (nchain * nrhs * nfun complex) and R (nchain * nstage * nrhs * nproj complex) in device memory of this
        problem's device, e.g. torch tensors' data_ptr(); X and R are written in place (either pointer may be None).  l, z, w, a are
        host values as in resolvent_chain.  Returns info (nchain, nstage)."""
        nchain, nstage, l, z, w, a = self._chain_stages(l, z, w, a, nop)
        info = np.zeros((nchain, nstage), dtype=np.int32)
        vp = lambda v: None if v is None else C.c_void_p(v)
        _chk(lib().bspatom_resolvent_chain_dev(self._h, nchain, nstage, _p(l), _p(z), nabs, vp(W_ptr), _p(w), nop, vp(G_ptr), _p(a), nrhs,
                                               vp(B_ptr), nproj, vp(P_ptr), vp(X_ptr), vp(R_ptr), _p(info)), "bspatom_resolvent_chain_dev")
        return info

    @staticmethod
    def _coupled_system(l, z, w, couplings, a, nop):
        """(nmat, nch, l int32, z complex128, w int32 or None -- each (nmat, nch), broadcast from (nch,) --, cr, cc, ctr int32
        (ncoup,) or None, a complex128 (nmat, ncoup, nop) or None, broadcast from (ncoup, nop) or, with one operator, (ncoup,); a
        None with one operator means coefficient 1), all contiguous"""
        l, z = np.asarray(l, dtype=np.int32), np.asarray(z, dtype=np.complex128)
        w = None if w is None else np.asarray(w, dtype=np.int32)
        shape = np.broadcast_shapes(l.shape, z.shape, () if w is None else w.shape)
        assert 1 <= len(shape) <= 2, "l, z, w must be (nch,) or (nmat, nch), got %s" % (shape,)
        nmat, nch = (1,) * (2 - len(shape)) + tuple(shape)
        ncoup = 0 if couplings is None else len(couplings)
        cr = cc = ctr = None
        if ncoup == 0:
            a = None
        else:
            assert nop >= 1, "couplings need operator bands G"
            top = np.asarray(couplings, dtype=np.int32).reshape(ncoup, 3)
            cr, cc, ctr = (np.ascontiguousarray(top[:, q]) for q in range(3))
            a = np.ones((ncoup, nop)) if a is None and nop == 1 else a
            assert a is not None, "a (nmat, ncoup, nop) is needed with more than one operator"
            a = np.asarray(a, dtype=np.complex128)
            if a.ndim == 1 and nop == 1:
                a = a[:, None]
            if a.ndim == 3 and nmat == 1:
                nmat = a.shape[0]
            a = np.ascontiguousarray(np.broadcast_to(a, (nmat, ncoup, nop)))
        bc = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(v, (nmat, nch)))
        return nmat, nch, bc(l), bc(z), bc(w), cr, cc, ctr, a

    def _resolvent_coupled_host(self, entry, l, z, B, couplings, G, a, W, w, P, want_x):
        """resolvent_coupled / resolvent_coupled_wide: the host arrays of one call to the entry point `entry`"""
        n = self.nfun
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        G = None if G is None else np.ascontiguousarray(np.asarray(G, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        nabs, nop = 0 if W is None else W.shape[0], 0 if G is None else G.shape[0]
        nmat, nch, l, z, w, cr, cc, ctr, a = self._coupled_system(l, z, w, couplings, a, nop)
        B = np.ascontiguousarray(np.asarray(B, dtype=np.complex128).reshape(-1, nch, n))
        P = None if P is None else np.ascontiguousarray(np.asarray(P, dtype=np.complex128).reshape(-1, nch, n))
        nrhs, nproj, ncoup = B.shape[0], 0 if P is None else P.shape[0], 0 if cr is None else cr.size
        X = np.zeros((nmat, nrhs, nch, n), dtype=np.complex128) if want_x else None
        R = np.zeros((nmat, nrhs, nproj), dtype=np.complex128) if P is not None else None
        info = np.zeros(nmat, dtype=np.int32)
        _chk(getattr(lib(), entry)(self._h, nmat, nch, _p(l), _p(z), nabs, _p(W), _p(w), ncoup, _p(cr), _p(cc), _p(ctr), nop,
                                    _p(G), _p(a), nrhs, _p(B), nproj, _p(P), _p(X), _p(R), _p(info)), entry)
        return X, R, info

    def resolvent_coupled(self, l, z, B, couplings=None, G=None, a=None, W=None, w=None, P=None, want_x=True):
        """Several channels coupled to ALL orders, one banded LU per matrix on the GPU (bspatom_resolvent_coupled): matrix m acts on
        nch blocks of nfun coefficients, diagonal block c = H_l[m, c] - i W_w[m, c] - z[m, c] S, and every entry (cr, cc, ctr) of
        `couplings` adds sum_o a[m, p, o] G[o] -- its transpose where ctr = 1 -- to block (cr, cc); no partner is added, a Hermitian
        coupling is two entries.  l, z, w: (nmat, nch), broadcast from (nch,); every channel has its own energy (a Floquet block
        carries z - n omega); G: full bands (nop, 2k-1, nfun) or (2k-1, nfun) as dipole_bands / operator_bands return them; a: COMPLEX,
        (nmat, ncoup, nop), broadcast from (ncoup, nop) or, with one operator, (ncoup,); None with one operator: coefficient 1.
        B: (nrhs, nch, nfun) or (nch, nfun), P: (nproj, nch, nfun), (nch, nfun) or None; W, w as in resolvent.  Returns (X, R, info):
        X (nmat, nrhs, nch, nfun) complex128 or None (want_x False), R (nmat, nrhs, nproj) = sum over all channels of P x (bilinear)
        or None (P None), info (nmat,) replaced pivots (0).  nch * k - 1 <= 63, else BspAtomError(-5)."""
        return self._resolvent_coupled_host("bspatom_resolvent_coupled", l, z, B, couplings, G, a, W, w, P, want_x)

    def resolvent_coupled_wide(self, l, z, B, couplings=None, G=None, a=None, W=None, w=None, P=None, want_x=True):
        """resolvent_coupled for WIDE bands (bspatom_resolvent_coupled_wide, csrc/resolvent_wide.hip): the same arguments and results,
        a blocked LU on the matrix cores, nch * k - 1 <= BSPATOM_COUPLED_WIDE_MAX_BAND = 255 (any half-width from 1 on), else
        BspAtomError(-5).  Not bit-identical to resolvent_coupled where both apply: another order of summation."""
        return self._resolvent_coupled_host("bspatom_resolvent_coupled_wide", l, z, B, couplings, G, a, W, w, P, want_x)

    def _resolvent_coupled_device(self, entry, l, z, nrhs, B_ptr, couplings, nop, G_ptr, a, nabs, W_ptr, w, nproj, P_ptr, X_ptr, R_ptr):
        """resolvent_coupled_dev / resolvent_coupled_wide_dev: one call to the entry point `entry` on device pointers"""
        nmat, nch, l, z, w, cr, cc, ctr, a = self._coupled_system(l, z, w, couplings, a, nop)
        info = np.zeros(nmat, dtype=np.int32)
        vp = lambda v: None if v is None else C.c_void_p(v)
        _chk(getattr(lib(), entry)(self._h, nmat, nch, _p(l), _p(z), nabs, vp(W_ptr), _p(w), 0 if cr is None else cr.size,
                                    _p(cr), _p(cc), _p(ctr), nop, vp(G_ptr), _p(a), nrhs, vp(B_ptr), nproj, vp(P_ptr),
                                    vp(X_ptr), vp(R_ptr), _p(info)), entry)
        return info

    def resolvent_coupled_dev(self, l, z, nrhs, B_ptr, couplings=None, nop=0, G_ptr=None, a=None, nabs=0, W_ptr=None, w=None, nproj=0,
                              P_ptr=None, X_ptr=None, R_ptr=None):
        """resolvent_coupled with B (nrhs * nch * nfun complex), G (nop * (2k-1) * nfun doubles), W (nabs * (2k-1) * nfun doubles), P
        (nproj * nch * nfun complex), X (nmat * nrhs * nch * nfun complex) and R (nmat * nrhs * nproj complex) in device memory of this
        problem's device, e.g. torch tensors' data_ptr(); X and R are written in place (either pointer may be None).  l, z, w,
        couplings, a are host values as in resolvent_coupled.  Returns info (nmat,)."""
        return self._resolvent_coupled_device("bspatom_resolvent_coupled_dev", l, z, nrhs, B_ptr, couplings, nop, G_ptr, a, nabs, W_ptr, w,
                                              nproj, P_ptr, X_ptr, R_ptr)

    def resolvent_coupled_wide_dev(self, l, z, nrhs, B_ptr, couplings=None, nop=0, G_ptr=None, a=None, nabs=0, W_ptr=None, w=None, nproj=0,
                                   P_ptr=None, X_ptr=None, R_ptr=None):
        """resolvent_coupled_dev for wide bands (bspatom_resolvent_coupled_wide_dev): the same arguments, nch * k - 1 <= 255"""
        return self._resolvent_coupled_device("bspatom_resolvent_coupled_wide_dev", l, z, nrhs, B_ptr, couplings, nop, G_ptr, a, nabs, W_ptr,
                                              w, nproj, P_ptr, X_ptr, R_ptr)

    def write_wf(self, c, npts=10000):
        c = np.ascontiguousarray(c, dtype=np.float64)
        r = np.zeros(npts + 1); u = np.zeros(npts + 1)
        _chk(lib().bspatom_write_wf(self._h, _p(c), npts, _p(r), _p(u)), "bspatom_write_wf")
        return r, u

    def quadrature(self):
        """(r, w): points and weights of the assembly's Gauss-Legendre quadrature on the knot intervals of positive width,
        ascending, ka per interval -- the grid `r=None` selects in tabulate / wavefunctions."""
        nr = C.c_int(0)
        _chk(lib().bspatom_quadrature(self._h, C.byref(nr), None, None), "bspatom_quadrature")
        r = np.zeros(nr.value); w = np.zeros(nr.value)
        _chk(lib().bspatom_quadrature(self._h, C.byref(nr), _p(r), _p(w)), "bspatom_quadrature")
        return r, w

    def _points(self, r):
        """(npts, host array or None) of a points argument: None = the quadrature grid"""
        if r is None:
            nr = C.c_int(0)
            _chk(lib().bspatom_quadrature(self._h, C.byref(nr), None, None), "bspatom_quadrature")
            return nr.value, None
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        return r.size, r

    def tabulate(self, Z, r=None, deriv=True):
        """u(r) = sum_j Z[v, j] B_j(r) and, with deriv, u'(r) for the rows of Z (nvec, nfun) at the points r (host array, any
        order, inside [ra, rb]; None: the quadrature grid): (U, dU), each (nvec, npts), or U alone."""
        Z = np.ascontiguousarray(Z, dtype=np.float64).reshape(-1, self.nfun)
        npts, r = self._points(r)
        U = np.zeros((Z.shape[0], npts)); dU = np.zeros_like(U) if deriv else None
        _chk(lib().bspatom_tabulate(self._h, Z.shape[0], _p(Z), npts, _p(r), _p(U), _p(dU)), "bspatom_tabulate")
        return (U, dU) if deriv else U

    def tabulate_dev(self, nvec, Z_ptr, U_ptr, dU_ptr=None, r=None):
        """tabulate with the vectors (nvec * nfun doubles at Z_ptr) and the tables (nvec * npts doubles at U_ptr and, unless
        None, at dU_ptr) in device memory of this problem's device, e.g. torch tensors' data_ptr(); written in place.  r is
        a host array or None (the quadrature grid).  Returns npts when the tables are there."""
        npts, r = self._points(r)
        _chk(lib().bspatom_tabulate_dev(self._h, nvec, C.c_void_p(Z_ptr), npts, _p(r), C.c_void_p(U_ptr),
                                        C.c_void_p(dU_ptr) if dU_ptr else None), "bspatom_tabulate_dev")
        return npts

    def wavefunctions(self, l0, nl, n0, count, r=None, deriv=True):
        """u(r) and, with deriv, u'(r) of eigenvectors n0 .. n0+count-1 (1-based) of channels l0 .. l0+nl-1 of the last solve at
        the points r (None: the quadrature grid): (U, dU), each (nl, count, npts), or U alone; equal to tabulate applied to
        eigvecs_batch(l0, nl, n0, count), bit for bit."""
        npts, r = self._points(r)
        U = np.zeros((max(nl, 0), max(count, 0), npts)); dU = np.zeros_like(U) if deriv else None
        _chk(lib().bspatom_wavefunctions(self._h, l0, nl, n0, count, npts, _p(r), _p(U), _p(dU)), "bspatom_wavefunctions")
        return (U, dU) if deriv else U

    def wavefunctions_dev(self, l0, nl, n0, count, U_ptr, dU_ptr=None, r=None):
        """wavefunctions into device memory of this problem's device (nl * count * npts doubles at U_ptr and, unless None, at
        dU_ptr), written in place.  Returns npts when the tables are there."""
        npts, r = self._points(r)
        _chk(lib().bspatom_wavefunctions_dev(self._h, l0, nl, n0, count, npts, _p(r), C.c_void_p(U_ptr),
                                             C.c_void_p(dU_ptr) if dU_ptr else None), "bspatom_wavefunctions_dev")
        return npts

    @staticmethod
    def _tdse_pairs(pairs):
        pr = np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2)
        return np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])

    # What the twelve tdse_* methods share.  A host method: _tdse_host, its own check of the field, _tdse_out, the call on
    # _tdse_common (+ _tdse_static_args), _tdse_result; a _dev method: the call on the same lists with addresses in the arrays' places.
    @staticmethod
    def _tdse_host(E, pairs, D, a0):
        """(E, ci, cf, D, a, one, nscan): contiguous E (nch, count), D (npairs, count, count) and a fresh a (nscan, nch, count);
        one: a0 was a single wave packet (nch, count)"""
        E = np.ascontiguousarray(E, dtype=np.float64)
        nch, count = E.shape
        ci, cf = Problem._tdse_pairs(pairs)
        D = np.ascontiguousarray(D, dtype=np.float64).reshape(len(ci), count, count)
        a = np.array(a0, dtype=np.complex128, order="C")
        one = a.ndim == 2
        a = np.ascontiguousarray(a.reshape(-1, nch, count))
        return E, ci, cf, D, a, one, a.shape[0]

    @staticmethod
    def _tdse_out(a, nsteps, snap_every, obs_every=0, ow=4):
        """(err, snaps, obs) for a (nscan, nch, count): snaps None without snap_every, obs (rows of ow) None without obs_every"""
        nscan, nch, count = a.shape
        snaps = np.zeros((nsteps // snap_every, nscan, nch, count), dtype=np.complex128) if snap_every > 0 else None
        obs = np.zeros((Problem.tdse_nobs(nsteps, obs_every), nscan, nch, ow)) if obs_every > 0 else None
        return np.zeros(nscan), snaps, obs

    def _tdse_common(self, nch, count, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err):
        """the 16 arguments every bspatom_tdse_* call begins with; E, D, field, a, snap: host arrays, device addresses or None"""
        D, ci_, cf_ = (D, ci, cf) if len(ci) else (None, None, None)
        return [self._h, nch, count, _ptr(E), len(ci), _p(ci_), _p(cf_), _ptr(D), nscan, nsteps, float(dt), _ptr(field), _ptr(a),
                snap_every, _ptr(snap), _p(err)]

    @staticmethod
    def _tdse_static_args(scheme, si, sf, skind, W):
        """scheme and the static lists as bspatom_tdse_static takes them; W: a host array or a device address"""
        ns = len(si)
        return [int(scheme), ns] + ([_p(si), _p(sf), _p(skind), _ptr(W)] if ns else [None] * 4)

    @staticmethod
    def _tdse_result(a, one, err, obs=None, snaps=None):
        return (a[0] if one else a, err) + (() if obs is None else (obs,)) + (() if snaps is None else (snaps,))

    def tdse_propagate(self, E, pairs, D, a0, field, dt, snap_every=0):
        """nsteps fixed Runge-Kutta steps dt of i da/dt = (E + f(t) D) a in the eigenstate basis (bspatom_tdse_propagate) for nscan
        wave packets at once.  E: (nch, count); pairs: [(ci, cf)] channel positions; D: (npairs, count, count), D[p, i, f] between
        state i of channel ci and state f of cf (dipole_matrix's layout); a0: complex (nscan, nch, count) or (nch, count);
        field: complex (nsteps, 6, nscan), f_q at the stage times (host.field_table).  Returns (a, err), err (nscan,) the largest
        embedded error estimate of a step, or (a, err, snaps) with snaps (nsteps // snap_every, nscan, nch, count)."""
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        field = np.ascontiguousarray(field, dtype=np.complex128)
        nsteps = field.shape[0] if field.ndim == 3 else 0
        assert field.shape == (nsteps, 6, nscan), (field.shape, nscan)
        err, snaps, _ = self._tdse_out(a, nsteps, snap_every)
        _chk(lib().bspatom_tdse_propagate(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snaps, err)),
             "bspatom_tdse_propagate")
        return self._tdse_result(a, one, err, None, snaps)

    def tdse_propagate_dev(self, nch, count, E_ptr, pairs, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, snap_every=0, snap_ptr=None):
        """tdse_propagate with E (nch * count doubles at E_ptr), D, the field table (nsteps * 6 * nscan complex) and the amplitudes
        (nscan * nch * count complex at a_ptr, advanced in place) in device memory of this problem's device, e.g. torch tensors'
        data_ptr(); snapshots, if asked for, at snap_ptr.  pairs is a host list.  Returns err (nscan,) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        err = np.zeros(nscan)
        _chk(lib().bspatom_tdse_propagate_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr,
                                                                 snap_every, snap_ptr, err)), "bspatom_tdse_propagate_dev")
        return err

    @staticmethod
    def tdse_nobs(nsteps, obs_every):
        """the number of rows of tdse_observe: the steps 0, obs_every, .. < nsteps and nsteps itself"""
        return 1 if nsteps == 0 else (nsteps - 1) // obs_every + 2

    def tdse_observe(self, E, pairs, D, a0, field, dt, obs_every=1, snap_every=0):
        """tdse_propagate with the observables of the steps 0, obs_every, 2 obs_every, .. < nsteps and of the final state
        (bspatom_tdse_observe; host.obs_steps gives the step numbers).  Returns (a, err, obs) or (a, err, obs, snaps); obs:
        (nobs, nscan, nch, 4), [.., c, :] = sum |a_c|^2, sum E_c |a_c|^2, Re z_c, Im z_c with z_c = sum over the pairs with cf = c of
        conj(a_cf) . D_p^T a_ci (host.tdse_expectations sums them).  a, err and snaps have the bits of tdse_propagate.  A field of
        no steps (shape (0, 6, nscan)) measures a0 as given: the expectation values of any blocks over any wave packets."""
        if obs_every < 1:
            raise ValueError("tdse_observe needs obs_every >= 1 (tdse_propagate is the call without observables)")
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        field = np.ascontiguousarray(field, dtype=np.complex128)
        nsteps = field.shape[0] if field.ndim == 3 else 0
        assert field.shape == (nsteps, 6, nscan), (field.shape, nscan)
        err, snaps, obs = self._tdse_out(a, nsteps, snap_every, obs_every)
        _chk(lib().bspatom_tdse_observe(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snaps, err),
                                        obs_every, _p(obs)), "bspatom_tdse_observe")
        return self._tdse_result(a, one, err, obs, snaps)

    def tdse_observe_dev(self, nch, count, E_ptr, pairs, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, obs_every, obs_ptr, snap_every=0,
                         snap_ptr=None):
        """tdse_propagate_dev with the observables written in place at obs_ptr (tdse_nobs(nsteps, obs_every) * nscan * nch * 4
        doubles of device memory).  Returns err (nscan,) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        err = np.zeros(nscan)
        _chk(lib().bspatom_tdse_observe_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, snap_every,
                                                               snap_ptr, err), obs_every, _ptr(obs_ptr)), "bspatom_tdse_observe_dev")
        return err

    def tdse_lawson(self, E, pairs, D, a0, field, dt, obs_every=0, snap_every=0):
        """tdse_propagate / tdse_observe with Lawson (integrating-factor) steps of the same tableau (bspatom_tdse_lawson): the free
        evolution exp(-i E t) is exact, so the step is bounded by |f| ||D|| and not by dt max|E|.  The arguments and layouts are
        tdse_observe's; obs_every = 0 propagates only.  Returns (a, err[, obs][, snaps]) as tdse_propagate / tdse_observe do, all in
        the Schroedinger picture at step boundaries."""
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        field = np.ascontiguousarray(field, dtype=np.complex128)
        nsteps = field.shape[0] if field.ndim == 3 else 0
        assert field.shape == (nsteps, 6, nscan), (field.shape, nscan)
        err, snaps, obs = self._tdse_out(a, nsteps, snap_every, obs_every)
        _chk(lib().bspatom_tdse_lawson(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snaps, err),
                                       obs_every, _p(obs)), "bspatom_tdse_lawson")
        return self._tdse_result(a, one, err, obs, snaps)

    def tdse_lawson_dev(self, nch, count, E_ptr, pairs, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, obs_every=0, obs_ptr=None, snap_every=0,
                        snap_ptr=None):
        """tdse_lawson on device memory, the arguments of tdse_observe_dev (obs_every = 0 with obs_ptr None: no observables).
        Returns err (nscan,) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        err = np.zeros(nscan)
        _chk(lib().bspatom_tdse_lawson_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, snap_every,
                                                              snap_ptr, err), obs_every, _ptr(obs_ptr)), "bspatom_tdse_lawson_dev")
        return err

    @staticmethod
    def _tdse_static(static, count=None):
        """(si, sf, skind, W or None) of a static argument (spairs, skind, W); None or empty lists: no static block"""
        if static is None:
            return (np.zeros(0, dtype=np.int32),) * 3 + (None,)
        spairs, skind, W = static
        si, sf = Problem._tdse_pairs(spairs)
        skind = np.ascontiguousarray(np.asarray(skind, dtype=np.int32).reshape(-1))
        if len(skind) != len(si):
            raise ValueError("static: %d pairs but %d kinds" % (len(si), len(skind)))
        if count is not None:
            W = np.ascontiguousarray(W, dtype=np.float64).reshape(len(si), count, count)
        return si, sf, skind, W

    def tdse_static(self, E, pairs, D, a0, field, dt, static, scheme=1, obs_every=0, snap_every=0):
        """tdse_observe / tdse_lawson with static blocks beside the driven couplings (bspatom_tdse_static): static = (spairs, skind, W),
        spairs [(si, sf)] channel positions (si == sf allowed: an in-channel block), skind[j] 0 (+ W_j^T a_si) or 1 (- i W_j^T a_si,
        an absorber when W_j is symmetric positive), W (nstat, count, count), W[j, i, f] between state i of si and state f of sf
        (operator_matrix's layout; host.tdse_absorber builds the absorber).  A block acts on channel sf alone, without a conjugate
        partner and without the field.  scheme: 1 = Lawson steps, 0 = the plain tableau.  Returns (a, err[, obs][, snaps]) as
        tdse_lawson does; obs: (nobs, nscan, nch, 6), [..., :4] as tdse_observe, [..., 4:] = Re, Im of s_c = conj(a_c) . S_c
        (host.tdse_static_rates, host.tdse_yield)."""
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        si, sf, skind, W = self._tdse_static(static, E.shape[1])
        field = np.ascontiguousarray(field, dtype=np.complex128)
        nsteps = field.shape[0] if field.ndim == 3 else 0
        assert field.shape == (nsteps, 6, nscan), (field.shape, nscan)
        err, snaps, obs = self._tdse_out(a, nsteps, snap_every, obs_every, 6)
        _chk(lib().bspatom_tdse_static(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snaps, err),
                                       obs_every, _p(obs), *self._tdse_static_args(scheme, si, sf, skind, W)), "bspatom_tdse_static")
        return self._tdse_result(a, one, err, obs, snaps)

    def tdse_static_dev(self, nch, count, E_ptr, pairs, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, static, scheme=1, obs_every=0,
                        obs_ptr=None, snap_every=0, snap_ptr=None):
        """tdse_static on device memory: the arguments of tdse_lawson_dev, static = (spairs, skind, W_ptr) with the nstat * count * count
        doubles of W at W_ptr, and rows of 6 doubles per (scan, channel) at obs_ptr.  Returns err (nscan,) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        si, sf, skind, W_ptr = self._tdse_static(static)
        err = np.zeros(nscan)
        _chk(lib().bspatom_tdse_static_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, snap_every,
                                                              snap_ptr, err), obs_every, _ptr(obs_ptr),
                                           *self._tdse_static_args(scheme, si, sf, skind, W_ptr)), "bspatom_tdse_static_dev")
        return err

    def tdse_adaptive(self, E, pairs, D, a0, fn, dt, static, tol, max_level, nsub=1, level0=0, scheme=1, obs_every=0, snap_every=0,
                      log_cap=0):
        """tdse_static with step-size control on the device (bspatom_tdse_adaptive): dt and the nsteps of fn describe the COARSE grid;
        inside every coarse step the controller halves the step, down to dt / 2**max_level, until the embedded estimate of every scan is
        within tol, and doubles it again where the estimate is below tol / 64.  fn: complex (nsteps * nsub + 1, 2, nscan), [i, 0, q] =
        f_q and [i, 1, q] = df_q/dt at t0 + i dt / nsub (host.field_nodes); the library integrates the equation with the cubic Hermite
        interpolant of these nodes.  Returns (a, err[, obs][, snaps], stats, log): obs and snaps on the coarse grid as tdse_static
        gives them, stats int64 (6,) = accepted, rejected, forced, deepest level, level at the end (level0 of a continued run),
        attempts; log = (log_i (nlog, 4) int32 rows (n, m, j, flag), log_e (nlog, nscan), log_f (nlog, 6, nscan) complex) of the first
        log_cap attempts (host.adapt_steps).  The step sequence depends on all scans of the call; a forced step (flag 2) may exceed tol."""
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        si, sf, skind, W = self._tdse_static(static, E.shape[1])
        fn = np.ascontiguousarray(fn, dtype=np.complex128)
        nsub = int(nsub)
        if fn.ndim != 3 or fn.shape[1:] != (2, nscan) or nsub < 1 or (fn.shape[0] - 1) % nsub:
            raise ValueError("fn must be (nsteps * nsub + 1, 2, nscan) with nscan = %d, nsub = %d, got %s" % (nscan, nsub, fn.shape))
        nsteps = (fn.shape[0] - 1) // nsub
        err, snaps, obs = self._tdse_out(a, nsteps, snap_every, obs_every, 6)
        stats = np.zeros(6, dtype=np.int64)
        log_i = np.zeros((log_cap, 4), dtype=np.int32) if log_cap > 0 else None
        log_e = np.zeros((log_cap, nscan)) if log_cap > 0 else None
        log_f = np.zeros((log_cap, 6, nscan), dtype=np.complex128) if log_cap > 0 else None
        _chk(lib().bspatom_tdse_adaptive(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, fn, a, snap_every, snaps, err),
                                         obs_every, _p(obs), *self._tdse_static_args(scheme, si, sf, skind, W), nsub, float(tol),
                                         int(max_level), int(level0), _p(stats), int(log_cap), _p(log_i), _p(log_e), _p(log_f)),
             "bspatom_tdse_adaptive")
        nlog = int(min(stats[5], log_cap))
        log = (log_i[:nlog], log_e[:nlog], log_f[:nlog]) if log_cap > 0 else (np.zeros((0, 4), dtype=np.int32), np.zeros((0, nscan)),
                                                                             np.zeros((0, 6, nscan), dtype=np.complex128))
        return self._tdse_result(a, one, err, obs, snaps) + (stats, log)

    def tdse_adaptive_dev(self, nch, count, E_ptr, pairs, D_ptr, nscan, nsteps, dt, fn_ptr, a_ptr, static, tol, max_level, nsub=1, level0=0,
                          scheme=1, obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None, log_cap=0, log_ptrs=None):
        """tdse_adaptive on device memory: the arguments of tdse_static_dev with the node table ((nsteps * nsub + 1) * 2 * nscan complex)
        at fn_ptr; log_ptrs = (log_i, log_e, log_f) device pointers for log_cap entries (4 int32, nscan doubles, 6 * nscan complex
        each).  Returns (err (nscan,), stats (6,) int64) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        si, sf, skind, W_ptr = self._tdse_static(static)
        err = np.zeros(nscan)
        stats = np.zeros(6, dtype=np.int64)
        _chk(lib().bspatom_tdse_adaptive_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, fn_ptr, a_ptr, snap_every,
                                                                snap_ptr, err), obs_every, _ptr(obs_ptr),
                                             *self._tdse_static_args(scheme, si, sf, skind, W_ptr), int(nsub), float(tol), int(max_level),
                                             int(level0), _p(stats), int(log_cap), *[_ptr(x) for x in (log_ptrs or (None,) * 3)]),
             "bspatom_tdse_adaptive_dev")
        return err, stats

    @staticmethod
    def _tdse_fidx(fidx, npairs):
        """fidx as int32 (npairs,); None stays None (the library's NULL: all pairs on field 0, one field only)"""
        if fidx is None:
            return None
        fidx = np.ascontiguousarray(np.asarray(fidx, dtype=np.int32).reshape(-1))
        if len(fidx) != npairs:
            raise ValueError("fidx: %d entries for %d pairs" % (len(fidx), npairs))
        return fidx

    def tdse_fields(self, E, pairs, D, fidx, a0, field, dt, static=None, scheme=1, obs_every=0, snap_every=0):
        """tdse_static with several drive fields (bspatom_tdse_fields): fidx[p] names the field that multiplies pair p, field is complex
        (nsteps, 6, nfield, nscan), [n, s, g, q] = f_{g,q} at the stage times (host.field_table_pol builds the two fields of a
        field of any direction on the blocks of host.tdse_system_pol); nfield <= 3.  Returns (a, err[, obs][, snaps]) as tdse_static
        does; obs: (nobs, nscan, nch, 4 + 2 nfield), [..., :2] population and sum E |a|^2, [..., 2:4] = Re, Im of z_{c,0}, [..., 4:6] of s_c,
        [..., 4 + 2g: 6 + 2g] of z_{c,g}, z_{c,g} the sum over the pairs of field g that end in c (host.tdse_dipole_vector).  A field of
        shape (0, 6, nfield, nscan) measures a0 as given."""
        E, ci, cf, D, a, one, nscan = self._tdse_host(E, pairs, D, a0)
        fidx = self._tdse_fidx(fidx, len(ci))
        si, sf, skind, W = self._tdse_static(static, E.shape[1])
        field = np.ascontiguousarray(field, dtype=np.complex128)
        if field.ndim != 4 or field.shape[1] != 6 or field.shape[3] != nscan:
            raise ValueError("field must have shape (nsteps, 6, nfield, %d), got %s" % (nscan, field.shape))
        nsteps, nfield = field.shape[0], field.shape[2]
        err, snaps, obs = self._tdse_out(a, nsteps, snap_every, obs_every, 4 + 2 * max(nfield, 1))
        _chk(lib().bspatom_tdse_fields(*self._tdse_common(*E.shape, E, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snaps, err),
                                       obs_every, _p(obs), *self._tdse_static_args(scheme, si, sf, skind, W), nfield,
                                       _p(fidx) if len(ci) else None), "bspatom_tdse_fields")
        return self._tdse_result(a, one, err, obs, snaps)

    def tdse_fields_dev(self, nch, count, E_ptr, pairs, D_ptr, fidx, nfield, nscan, nsteps, dt, field_ptr, a_ptr, static=None, scheme=1,
                        obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None):
        """tdse_fields on device memory: the arguments of tdse_static_dev with fidx (a host list, or None with nfield = 1) and nfield; the
        field table nsteps * 6 * nfield * nscan complex at field_ptr, rows of 4 + 2 nfield doubles per (scan, channel) at obs_ptr.
        Returns err (nscan,) when the result is there."""
        ci, cf = self._tdse_pairs(pairs)
        fidx = self._tdse_fidx(fidx, len(ci))
        si, sf, skind, W_ptr = self._tdse_static(static)
        err = np.zeros(nscan)
        _chk(lib().bspatom_tdse_fields_dev(*self._tdse_common(nch, count, E_ptr, ci, cf, D_ptr, nscan, nsteps, dt, field_ptr, a_ptr, snap_every,
                                                              snap_ptr, err), obs_every, _ptr(obs_ptr),
                                           *self._tdse_static_args(scheme, si, sf, skind, W_ptr), int(nfield), _p(fidx) if len(ci) else None),
             "bspatom_tdse_fields_dev")
        return err

    @staticmethod
    def _spline_system(l, w, couplings, coef, nscan, nsteps, nop):
        """(nch, l int32 (nch,), w int32 (nch,) or None, cr, cc, ctr int32 (ncoup,) or None, coef complex128 (nsteps, nscan, ncoup, nop)
        or None, broadcast from (nsteps, ncoup, nop) -- every scan the same pulse), contiguous"""
        l = np.ascontiguousarray(np.asarray(l, dtype=np.int32).reshape(-1))
        w = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.int32), l.shape))
        ncoup = 0 if couplings is None else len(couplings)
        cr = cc = ctr = None
        if ncoup == 0:
            coef = None
        else:
            assert nop >= 1, "couplings need operator bands G"
            top = np.asarray(couplings, dtype=np.int32).reshape(ncoup, 3)
            cr, cc, ctr = (np.ascontiguousarray(top[:, q]) for q in range(3))
            if nsteps == 0:
                coef = None
            else:
                assert coef is not None, "coef (nsteps, nscan, ncoup, nop) is needed with couplings"
                coef = np.asarray(coef, dtype=np.complex128)
                if coef.ndim == 3:
                    coef = coef[:, None]
                assert coef.ndim == 4 and coef.shape[0] == nsteps, (coef.shape, nsteps)
                coef = np.ascontiguousarray(np.broadcast_to(coef, (nsteps, nscan, ncoup, nop)))
        return l.size, l, w, cr, cc, ctr, coef

    @staticmethod
    def _split_system(l, w, Q, lam):
        """(nch, l int32 (nch,), w int32 (nch,) or None, Q float64 (nch, nch) or None, lam float64 (nch,) or None), contiguous"""
        nch, l, w = Problem._spline_system(l, w, None, None, 0, 0, 0)[:3]
        Q = None if Q is None else np.ascontiguousarray(np.asarray(Q, dtype=np.float64).reshape(nch, nch))
        lam = None if lam is None else np.ascontiguousarray(np.asarray(lam, dtype=np.float64).reshape(nch))
        return nch, l, w, Q, lam

    def _spline_run(self, nch, c0, W, P, nsteps, obs_every, snap_every, nexp=0):
        """what the host calls of tdse_spline and tdse_split share: (nabs, W (nabs, 2k-1, nfun) or None, nscan, c complex (nscan, nch,
        nfun), a copy of c0, nproj, P (nproj, nch, nfun) or None (without rows), snaps, obs with rows nch + 2 nproj + 2 nexp wide, info,
        result), contiguous; result() is what the calls return once the entry point has filled the arrays"""
        n = self.nfun
        W = None if W is None else np.ascontiguousarray(np.asarray(W, dtype=np.float64).reshape(-1, 2 * self.k - 1, n))
        c = np.array(c0, dtype=np.complex128, order="C")
        one = c.ndim == 2
        c = np.ascontiguousarray(c.reshape(-1, nch, n))
        nscan = c.shape[0]
        P = None if P is None or obs_every < 1 else np.ascontiguousarray(np.asarray(P, dtype=np.complex128).reshape(-1, nch, n))
        nproj = 0 if P is None else P.shape[0]
        snaps = np.zeros((nsteps // snap_every, nscan, nch, n), dtype=np.complex128) if snap_every > 0 else None
        obs = np.zeros((self.tdse_nobs(nsteps, obs_every), nscan, nch + 2 * nproj + 2 * nexp)) if obs_every > 0 else None
        info = np.zeros(nscan, dtype=np.int32)
        result = lambda: (c[0] if one else c, info) + (() if obs is None else (obs,)) + (() if snaps is None else (snaps,))
        return 0 if W is None else W.shape[0], W, nscan, c, nproj, P, snaps, obs, info, result

    def tdse_spline(self, l, c0, dt, nsteps, couplings=None, G=None, coef=None, W=None, w=None, P=None, obs_every=0, snap_every=0):
        """nsteps Crank-Nicolson steps dt of i S dc/dt = (sum_c (H_l[c] - i W_w[c]) + V(t)) c in the B-spline basis itself
        (bspatom_tdse_spline): the whole continuum of the box, any absorber, any coupling, one banded LU per step and packet, the
        matrix resolvent_coupled's at z = 2i/dt.  l, w: (nch,); couplings [(cr, cc, ctr)], G, W as in resolvent_coupled; coef: COMPLEX
        (nsteps, nscan, ncoup, nop), the coefficient of entry p and operator o during step n of scan q -- the field at the step's
        MIDPOINT times the angular factor (host.spline_coefficients) --, broadcast from (nsteps, ncoup, nop).  c0: complex (nscan, nch,
        nfun) or (nch, nfun).  Returns (c, info), then obs if obs_every >= 1 -- (nobs, nscan, nch + 2 nproj): N_ch = Re c_ch^H S c_ch
        per channel, then Re, Im of sum P_r (S c) for the projections P (nproj, nch, nfun), for the steps 0, obs_every, .. < nsteps
        and the final state (tdse_nobs) --, then snaps (nsteps // snap_every, nscan, nch, nfun) if snap_every >= 1.  info (nscan,):
        replaced pivots, 0.  nsteps = 0 with obs_every >= 1 only measures.  nch * k - 1 <= 63, else BspAtomError(-5)."""
        return self._tdse_spline("bspatom_tdse_spline", l, c0, dt, nsteps, couplings, G, coef, W, w, P, obs_every, snap_every)

    def tdse_spline_wide(self, l, c0, dt, nsteps, couplings=None, G=None, coef=None, W=None, w=None, P=None, obs_every=0, snap_every=0):
        """tdse_spline on the blocked LU for wide bands (bspatom_tdse_spline_wide): the same arguments and results, the matrix
        resolvent_coupled_wide's at z = 2i/dt, nch * k - 1 <= 255, else BspAtomError(-5).  Not promised bit-equal to tdse_spline where
        both apply; host.spline_propagate chooses between them."""
        return self._tdse_spline("bspatom_tdse_spline_wide", l, c0, dt, nsteps, couplings, G, coef, W, w, P, obs_every, snap_every)

    def _tdse_spline(self, entry, l, c0, dt, nsteps, couplings, G, coef, W, w, P, obs_every, snap_every):
        """the body of tdse_spline and tdse_spline_wide: the arrays of the call, the entry point by name"""
        G = None if G is None else np.ascontiguousarray(np.asarray(G, dtype=np.float64).reshape(-1, 2 * self.k - 1, self.nfun))
        nop = 0 if G is None else G.shape[0]
        nabs, W, nscan, c, nproj, P, snaps, obs, info, result = self._spline_run(np.asarray(l).size, c0, W, P, nsteps, obs_every, snap_every)
        nch, l, w, cr, cc, ctr, coef = self._spline_system(l, w, couplings, coef, nscan, nsteps, nop)
        _chk(getattr(lib(), entry)(self._h, nscan, nch, _p(l), nabs, _p(W), _p(w), 0 if cr is None else cr.size, _p(cr), _p(cc), _p(ctr),
                                   nop, _p(G), nsteps, float(dt), _p(coef), _p(c), snap_every, _p(snaps), obs_every, nproj, _p(P),
                                   _p(obs), _p(info)), entry)
        return result()

    def tdse_spline_dev(self, l, nscan, nsteps, dt, c_ptr, couplings=None, nop=0, G_ptr=None, coef_ptr=None, nabs=0, W_ptr=None, w=None,
                        nproj=0, P_ptr=None, obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None):
        """tdse_spline with the packets (nscan * nch * nfun complex at c_ptr, advanced in place), G, W, the coefficient table (nsteps *
        nscan * ncoup * nop complex), P, the rows and the snapshots in device memory of this problem's device, e.g. torch tensors'
        data_ptr(); l, w and couplings are host values.  Returns info (nscan,) when the result is there."""
        return self._tdse_spline_dev("bspatom_tdse_spline_dev", l, nscan, nsteps, dt, c_ptr, couplings, nop, G_ptr, coef_ptr, nabs, W_ptr, w, nproj,
                                     P_ptr, obs_every, obs_ptr, snap_every, snap_ptr)

    def tdse_spline_wide_dev(self, l, nscan, nsteps, dt, c_ptr, couplings=None, nop=0, G_ptr=None, coef_ptr=None, nabs=0, W_ptr=None, w=None,
                             nproj=0, P_ptr=None, obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None):
        """tdse_spline_dev on the blocked LU for wide bands (bspatom_tdse_spline_wide_dev): the same arguments, nch * k - 1 <= 255."""
        return self._tdse_spline_dev("bspatom_tdse_spline_wide_dev", l, nscan, nsteps, dt, c_ptr, couplings, nop, G_ptr, coef_ptr, nabs, W_ptr, w,
                                     nproj, P_ptr, obs_every, obs_ptr, snap_every, snap_ptr)

    def _tdse_spline_dev(self, entry, l, nscan, nsteps, dt, c_ptr, couplings, nop, G_ptr, coef_ptr, nabs, W_ptr, w, nproj, P_ptr, obs_every, obs_ptr,
                         snap_every, snap_ptr):
        """the body of tdse_spline_dev and tdse_spline_wide_dev: the entry point by name"""
        nch, l, w, cr, cc, ctr, _ = self._spline_system(l, w, couplings, None, nscan, 0, nop)
        info = np.zeros(nscan, dtype=np.int32)
        _chk(getattr(lib(), entry)(self._h, nscan, nch, _p(l), nabs, _ptr(W_ptr), _p(w), 0 if cr is None else cr.size, _p(cr),
                                   _p(cc), _p(ctr), nop, _ptr(G_ptr), nsteps, float(dt), _ptr(coef_ptr), _ptr(c_ptr), snap_every,
                                   _ptr(snap_ptr), obs_every, nproj, _ptr(P_ptr), _ptr(obs_ptr), _p(info)), entry)
        return info

    def tdse_split(self, l, c0, dt, nsteps, G=None, Q=None, lam=None, f=None, W=None, w=None, P=None, obs_every=0, snap_every=0):
        """nsteps split Crank-Nicolson steps dt of i S dc/dt = (sum_c (H_l[c] - i W_w[c]) + f(t) A (x) G) c in the B-spline basis
        (bspatom_tdse_split): ONE operator term, A = Q diag(lam) Q^T the constant real symmetric angular matrix (host.split_angular), G
        one full band (2k-1, nfun) (dipole_bands()[0] for the length gauge).  Every substep is nch independent systems of half-width
        k - 1: the cost is linear in nch, and nch has no limit; k <= 16, else BspAtomError(-5).  l, w: (nch,); W as in tdse_spline; f:
        COMPLEX (nsteps, nscan), the field at every step's MIDPOINT (host.spline_midpoints), broadcast from (nsteps,).  c0: complex
        (nscan, nch, nfun) or (nch, nfun).  Returns what tdse_spline returns: (c, info), then obs if obs_every >= 1, then snaps if
        snap_every >= 1, in its shapes.  Second order in dt like tdse_spline, not equal to it: another splitting of the same equation."""
        return self._tdse_split(l, c0, dt, nsteps, G, Q, lam, f, W, w, P, obs_every, snap_every, None)

    def tdse_split_observe(self, l, c0, dt, nsteps, G=None, Q=None, lam=None, f=None, W=None, w=None, P=None, obs_every=0, snap_every=0,
                           expect=None):
        """tdse_split with expectation values along the run (bspatom_tdse_split_observe): expect = (B, GE) as spline_expect takes them
        (host.split_expect_dipole, host.split_expect_accel; stack several with numpy.stack).  The rows are nch + 2 nproj + 2 nexp wide:
        behind tdse_split's entries come Re, Im of <c| B_o (x) G_o |c>, o ascending, of the packets the row's N_ch are taken from
        (host.split_expect_rows extracts them).  Everything else has the bits of tdse_split; expect=None is that call."""
        return self._tdse_split(l, c0, dt, nsteps, G, Q, lam, f, W, w, P, obs_every, snap_every, expect)

    def _expect_operators(self, nch, expect):
        """(nexp, B (nexp, nch, nch), GE (nexp, 2k-1, nfun)) of an expect=(B, GE) argument; None: (0, None, None)"""
        if expect is None:
            return 0, None, None
        B, GE = expect
        B = np.ascontiguousarray(np.asarray(B, dtype=np.float64).reshape(-1, nch, nch))
        GE = np.ascontiguousarray(np.asarray(GE, dtype=np.float64).reshape(-1, 2 * self.k - 1, self.nfun))
        assert B.shape[0] == GE.shape[0], (B.shape, GE.shape)
        return B.shape[0], B, GE

    def spline_expect(self, c, B, GE):
        """e(q, o) = sum_c conj(c_c)^T G_o (sum_c' B_o(c, c') c_c') of packets in the spline basis (bspatom_spline_expect): c complex
        (nscan, nch, nfun) or (nch, nfun) -- tdse_spline's and tdse_split's packets, their snapshots --; B (nexp, nch, nch) or (nch, nch)
        real angular matrices of any pattern; GE (nexp, 2k-1, nfun) or (2k-1, nfun) real full bands, symmetric or not (dipole_bands,
        operator_bands, host.band_symmetric(SB)).  Returns complex (nscan, nexp), or (nexp,) for one packet.  The summation order is
        fixed (include/bspatom_spline_expect.h): the same bits from run to run and whatever else is in the call."""
        n = self.nfun
        B = np.asarray(B, dtype=np.float64)
        nch = B.shape[-1]
        nexp, B, GE = self._expect_operators(nch, (B, GE))
        c = np.asarray(c, dtype=np.complex128)
        one = c.ndim == 2
        c = np.ascontiguousarray(c.reshape(-1, nch, n))
        e = np.zeros((c.shape[0], nexp), dtype=np.complex128)
        _chk(lib().bspatom_spline_expect(self._h, c.shape[0], nch, nexp, _p(B), _p(GE), _p(c), _p(e)), "bspatom_spline_expect")
        return e[0] if one else e

    def spline_expect_dev(self, nscan, c_ptr, B, GE_ptr, e_ptr):
        """spline_expect with the packets (nscan * nch * nfun complex at c_ptr), the bands (nexp * (2k-1) * nfun doubles at GE_ptr)
        and the result (nscan * nexp complex at e_ptr) in device memory of this problem's device; B (nexp, nch, nch) is a host array."""
        B = np.asarray(B, dtype=np.float64)
        nch = B.shape[-1]
        B = np.ascontiguousarray(B.reshape(-1, nch, nch))
        _chk(lib().bspatom_spline_expect_dev(self._h, nscan, nch, B.shape[0], _p(B), _ptr(GE_ptr), _ptr(c_ptr), _ptr(e_ptr)),
             "bspatom_spline_expect_dev")

    def spline_window(self, l, c, z):
        """N(q, c, e) = x^H S x with x = prod_j (H_l[c] - z[e, j] S)^-1 S applied to packet (q, c) (bspatom_spline_window): the window
        operator of the grid codes in the spline basis, P_m(E) = gamma^(2m) N with the shifts of host.window_shifts(E, gamma, m)
        (host.window_spectrum does both).  l: (nch,) channels among the assembled bands; c: complex (nscan, nch, nfun) or (nch, nfun),
        tdse_split's packets; z: complex (ne, nfac), or (ne,) for one stage, nfac = 0 .. WINDOW_MAX_FAC, any values; (ne, 0) measures
        the S-norm.  Returns (N (nscan, nch, ne) -- (nch, ne) for one packet --, info (ne,) replaced pivots, 0 whenever Im z != 0).
        One factorisation per (distinct l, e, j) serves the packets of every scan and channel with that l; the arithmetic is
        resolvent's and tdse_split's, bit for bit (include/bspatom_spline_window.h, W1 - W6)."""
        l = np.ascontiguousarray(np.asarray(l, dtype=np.int32).reshape(-1))
        nch, n = l.size, self.nfun
        z = np.asarray(z, dtype=np.complex128)
        z = np.ascontiguousarray(z.reshape(-1, 1) if z.ndim == 1 else z)
        assert z.ndim == 2, z.shape
        ne, nfac = z.shape
        c = np.asarray(c, dtype=np.complex128)
        one = c.ndim == 2
        c = np.ascontiguousarray(c.reshape(-1, nch, n))
        N = np.zeros((c.shape[0], nch, ne))
        info = np.zeros(ne, dtype=np.int32)
        _chk(lib().bspatom_spline_window(self._h, c.shape[0], nch, _p(l), ne, nfac, _p(z) if nfac else None, _p(c), _p(N), _p(info)),
             "bspatom_spline_window")
        return (N[0] if one else N), info

    def spline_window_dev(self, l, nscan, c_ptr, z, N_ptr):
        """spline_window with the packets (nscan * nch * nfun complex at c_ptr) and the result (nscan * nch * ne doubles at N_ptr) in
        device memory of this problem's device; l and z are host values.  Returns info (ne,) when the result is there."""
        l = np.ascontiguousarray(np.asarray(l, dtype=np.int32).reshape(-1))
        z = np.asarray(z, dtype=np.complex128)
        z = np.ascontiguousarray(z.reshape(-1, 1) if z.ndim == 1 else z)
        ne, nfac = z.shape
        info = np.zeros(ne, dtype=np.int32)
        _chk(lib().bspatom_spline_window_dev(self._h, nscan, l.size, _p(l), ne, nfac, _p(z) if nfac else None, _ptr(c_ptr), _ptr(N_ptr),
                                             _p(info)), "bspatom_spline_window_dev")
        return info

    def _tdse_split(self, l, c0, dt, nsteps, G, Q, lam, f, W, w, P, obs_every, snap_every, expect):
        """the body of tdse_split and tdse_split_observe: the arrays of the call; expect None: bspatom_tdse_split"""
        nch, l, w, Q, lam = self._split_system(l, w, Q, lam)
        nexp, B, GE = self._expect_operators(nch, expect if obs_every > 0 else None)
        nabs, W, nscan, c, nproj, P, snaps, obs, info, result = self._spline_run(nch, c0, W, P, nsteps, obs_every, snap_every, nexp)
        G = None if G is None else np.ascontiguousarray(np.asarray(G, dtype=np.float64).reshape(2 * self.k - 1, self.nfun))
        if f is not None and nsteps > 0:
            f = np.asarray(f, dtype=np.complex128)
            f = f[:, None] if f.ndim == 1 else f
            assert f.ndim == 2 and f.shape[0] == nsteps, (f.shape, nsteps)
            f = np.ascontiguousarray(np.broadcast_to(f, (nsteps, nscan)))
        else:
            f = None
        args = (self._h, nscan, nch, _p(l), nabs, _p(W), _p(w), _p(G), _p(Q), _p(lam), nsteps, float(dt), _p(f), _p(c), snap_every, _p(snaps),
                obs_every, nproj, _p(P), _p(obs), _p(info))
        if expect is None:
            _chk(lib().bspatom_tdse_split(*args), "bspatom_tdse_split")
        else:
            _chk(lib().bspatom_tdse_split_observe(*args, nexp, _p(B), _p(GE)), "bspatom_tdse_split_observe")
        return result()

    def tdse_split_dev(self, l, nscan, nsteps, dt, c_ptr, G_ptr=None, Q=None, lam=None, f_ptr=None, nabs=0, W_ptr=None, w=None, nproj=0,
                       P_ptr=None, obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None):
        """tdse_split with the packets (nscan * nch * nfun complex at c_ptr, advanced in place), G, W, the field table (nsteps * nscan
        complex), P, the rows and the snapshots in device memory of this problem's device, e.g. torch tensors' data_ptr(); l, w, Q and
        lam are host values.  Returns info (nscan,) when the result is there."""
        nch, l, w, Q, lam = self._split_system(l, w, Q, lam)
        info = np.zeros(nscan, dtype=np.int32)
        _chk(lib().bspatom_tdse_split_dev(self._h, nscan, nch, _p(l), nabs, _ptr(W_ptr), _p(w), _ptr(G_ptr), _p(Q), _p(lam), nsteps, float(dt),
                                          _ptr(f_ptr), _ptr(c_ptr), snap_every, _ptr(snap_ptr), obs_every, nproj, _ptr(P_ptr), _ptr(obs_ptr),
                                          _p(info)), "bspatom_tdse_split_dev")
        return info

    def tdse_split_observe_dev(self, l, nscan, nsteps, dt, c_ptr, G_ptr=None, Q=None, lam=None, f_ptr=None, nabs=0, W_ptr=None, w=None, nproj=0,
                               P_ptr=None, obs_every=0, obs_ptr=None, snap_every=0, snap_ptr=None, expect=None):
        """tdse_split_dev with expectation values along the run (bspatom_tdse_split_observe_dev): expect = (B, GE_ptr), B a host array
        (nexp, nch, nch), GE_ptr nexp * (2k-1) * nfun doubles in device memory; the rows at obs_ptr are nch + 2 nproj + 2 nexp wide."""
        nch, l, w, Q, lam = self._split_system(l, w, Q, lam)
        B, GE_ptr = (None, None) if expect is None else expect
        B = None if B is None else np.ascontiguousarray(np.asarray(B, dtype=np.float64).reshape(-1, nch, nch))
        info = np.zeros(nscan, dtype=np.int32)
        _chk(lib().bspatom_tdse_split_observe_dev(self._h, nscan, nch, _p(l), nabs, _ptr(W_ptr), _p(w), _ptr(G_ptr), _p(Q), _p(lam), nsteps,
                                                  float(dt), _ptr(f_ptr), _ptr(c_ptr), snap_every, _ptr(snap_ptr), obs_every, nproj,
                                                  _ptr(P_ptr), _ptr(obs_ptr), _p(info), 0 if B is None else B.shape[0], _p(B), _ptr(GE_ptr)),
             "bspatom_tdse_split_observe_dev")
        return info

    def early_vector_state(self):
        """0: the last solve computed no early vector; 1: computed and kept; -1: computed, failed its check, dropped (include/bspatom.h)."""
        st = C.c_int32(0)
        _chk(lib().bspatom_early_vector_state(self._h, C.byref(st)), "bspatom_early_vector_state")
        return st.value

    def route(self):
        """2 = band route (csrc/crawford.hip), 1 = dense route: what solve() takes under the current switches"""
        r = lib().bspatom_problem_route(self._h)
        _chk(min(r, 0), "bspatom_problem_route")
        return r

    def last_timing(self):
        ms = np.zeros(6)
        _chk(lib().bspatom_last_timing(self._h, _p(ms)), "bspatom_last_timing")
        return dict(zip(("assemble", "chol_std", "sy2sb", "sb2st", "bisect", "total"), ms.tolist()))


# ---- stage-level helpers (parity tests) ------------------------------------------------------
def _flat(x):
    base = x
    while base.base is not None:
        base = base.base
    return base


def stage_gemm(A, B, C_, alpha=1.0, beta=0.0, transA=False, transB=False):
    """C = alpha*op(A)@op(B) + beta*C on the MFMA kernel.  A, B, C_: (batch, rows, cols) numpy views whose
    element strides are passed through unchanged (so both C- and F-ordered matrices can be exercised)."""
    assert A.ndim == 3 and B.ndim == 3 and C_.ndim == 3
    opA = A.transpose(0, 2, 1) if transA else A
    opB = B.transpose(0, 2, 1) if transB else B
    batch, M, K = opA.shape
    N = opB.shape[2]
    es = 8
    fa, fb, fc = _flat(A), _flat(B), _flat(C_)
    rc = lib().bspatom_stage_gemm(M, N, K, batch,
                                  _p(fa), opA.strides[1] // es, opA.strides[2] // es, opA.strides[0] // es, fa.size,
                                  _p(fb), opB.strides[1] // es, opB.strides[2] // es, opB.strides[0] // es, fb.size,
                                  _p(fc), C_.strides[1] // es, C_.strides[2] // es, C_.strides[0] // es, fc.size,
                                  alpha, beta)
    _chk(rc, "bspatom_stage_gemm")
    return C_


def stage_standard_form(SB, HB):
    k, n = SB.shape
    nl = HB.shape[0]
    npad = (n + 63) // 64 * 64
    UB = np.zeros((k, n)); Cm = np.zeros((nl, npad, npad)); info = np.zeros(1, dtype=np.int32)
    _chk(lib().bspatom_stage_standard_form(n, k, nl, _p(np.ascontiguousarray(SB)), _p(np.ascontiguousarray(HB)),
                                           _p(UB), _p(Cm), _p(info)), "bspatom_stage_standard_form")
    # device layout is column-major per channel: C[l][j*npad + i] = C(i,j) -> transpose view
    return UB, Cm.transpose(0, 2, 1), int(info[0])


def stage_sy2sb(A):
    """A: (batch, npad, npad) symmetric.  Returns AB (batch, npad, 128): AB[b, j, d] = band(j+d, j)."""
    batch, npad, _ = A.shape
    Af = np.ascontiguousarray(A.transpose(0, 2, 1))      # column-major per channel
    AB = np.zeros((batch, npad, 128))
    _chk(lib().bspatom_stage_sy2sb(npad, batch, _p(Af), _p(AB)), "bspatom_stage_sy2sb")
    return AB


def stage_panel(A, c0):
    """Panel factorisation of sy2sb alone.  A: (batch, npad, npad), any matrix (only the panel A[:, c0+64:, c0:c0+64] is touched).
    Returns (A with the panel replaced by [R; 0], V (batch, m, 64), W (batch, m, 64))."""
    batch, npad, _ = A.shape
    m = npad - c0 - 64
    Af = np.ascontiguousarray(A.transpose(0, 2, 1))      # column-major per matrix
    V = np.zeros((batch, 64, m)); W = np.zeros((batch, 64, m))
    _chk(lib().bspatom_stage_panel(npad, c0, batch, _p(Af), _p(V), _p(W)), "bspatom_stage_panel")
    return Af.transpose(0, 2, 1), V.transpose(0, 2, 1), W.transpose(0, 2, 1)


def stage_sb2st(AB, n):
    batch, npad, _ = AB.shape
    d = np.zeros((batch, npad)); e = np.zeros((batch, npad))
    _chk(lib().bspatom_stage_sb2st(n, npad, batch, _p(np.ascontiguousarray(AB)), _p(d), _p(e)), "bspatom_stage_sb2st")
    return d[:, :n], e[:, :n - 1]


def stage_sb2sb(AB, n):
    """First half of the two-step route: band 64 -> band 16 (returns the band array, same layout)."""
    batch, npad, _ = AB.shape
    out = np.ascontiguousarray(AB).copy()
    _chk(lib().bspatom_stage_sb2sb(n, npad, batch, _p(out)), "bspatom_stage_sb2sb")
    return out


def stage_crawford(SB, HB):
    """Band route, first stage: upper bands SB (k, n), HB (nl, k, n) -> (AB (nl, npad, 128) with AB[l, j, d] = A_l(j + d, j), info)."""
    nl, k, n = HB.shape
    npad = (n + 63) // 64 * 64
    AB = np.zeros((nl, npad, 128))
    info = C.c_int32(0)
    _chk(lib().bspatom_stage_crawford(n, k, nl, _p(np.ascontiguousarray(SB, dtype=np.float64)),
                                      _p(np.ascontiguousarray(HB, dtype=np.float64)), _p(AB), C.byref(info)), "bspatom_stage_crawford")
    return AB, info.value


def stage_band_eigenvalue(SB, HB, m):
    """Eigenvalue m (0-based, ascending) of the banded pencil (HB, SB) (upper bands (k, n)) from inertia counts (csrc/bandsect.hip)."""
    k, n = HB.shape
    lam = np.zeros(1)
    _chk(lib().bspatom_stage_band_eigenvalue(n, k, _p(np.ascontiguousarray(SB, dtype=np.float64)),
                                             _p(np.ascontiguousarray(HB, dtype=np.float64)), m, _p(lam)), "bspatom_stage_band_eigenvalue")
    return lam[0]


def stage_bisect(d, e):
    batch, n = d.shape
    ee = np.zeros((batch, n)); ee[:, :n - 1] = e
    w = np.zeros((batch, n))
    _chk(lib().bspatom_stage_bisect(n, batch, _p(np.ascontiguousarray(d)), _p(ee), _p(w)), "bspatom_stage_bisect")
    return w


def dsygv(A, B, jobz="V", uplo="U", lda=None, ldb=None, sentinel=-777.0):
    """bsp_dsygv_ through its Fortran-77 ABI.  A, B: (n,n) arrays; returns w, Z (columns), factor of B, info.
    lda / ldb (optional, >= n): leading dimensions of the arrays handed over; the rows beyond n hold `sentinel` on entry and the
    arrays come back whole, (lda, n) and (ldb, n), so that a caller can see that those rows were left alone."""
    n = A.shape[0]
    def padded(M, ld):
        if ld is None:
            return np.array(M, dtype=np.float64, order="F")
        m = np.full((ld, n), sentinel, dtype=np.float64, order="F")
        m[:n, :] = M
        return m
    a = padded(A, lda); b = padded(B, ldb)
    w = np.zeros(n); work = np.zeros(max(1, 4 * n))
    it = C.c_int(1); nn = C.c_int(n); la = C.c_int(n if lda is None else lda); lb = C.c_int(n if ldb is None else ldb)
    lw = C.c_int(4 * n); info = C.c_int(0)
    lib().bsp_dsygv_(C.byref(it), C.c_char_p(jobz.encode()), C.c_char_p(uplo.encode()), C.byref(nn), _p(a), C.byref(la),
                     _p(b), C.byref(lb), _p(w), _p(work), C.byref(lw), C.byref(info), C.c_size_t(1), C.c_size_t(1))
    return w, a, b, info.value


def set_option(name, value):
    """Flip one of the library's run-time switches (BSP_* variables of DESIGN.md 4.4) in this process."""
    _chk(lib().bspatom_set_option(name.encode(), int(value)), "bspatom_set_option(%s)" % name)


def kernel_times():
    """Launch durations recorded since the last call while option "ktime" was 1: {slot name: (sum of ms, launches)}."""
    ms = np.zeros(16); cnt = np.zeros(16, dtype=np.int32)
    ns = lib().bspatom_kernel_times(_p(ms), _p(cnt), 16)
    if ns < 0:
        raise BspAtomError(ns, "bspatom_kernel_times")
    return {lib().bspatom_kernel_slot_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(ns)}


def get_option(name):
    v = C.c_int(0)
    _chk(lib().bspatom_get_option(name.encode(), C.byref(v)), "bspatom_get_option(%s)" % name)
    return v.value
