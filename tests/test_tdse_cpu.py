"""bspatom_tdse_propagate without a GPU: the entry points are bound and in the header, the kernels of csrc/tdse.hip are in the
library with no scratch and no spilled VGPRs, the tableau's order conditions as exact fractions, the host helpers (rk_nodes,
field_table, tdse_system, write_/read_tdse_coeffs), and the order of the NumPy restatement the GPU tests measure against."""
import os
import sys
from fractions import Fraction as F
import numpy as np
import pytest
from conftest import ROOT

import tdse_ref
from bspatom_amd import capi, host

NAMES = ("bspatom_tdse_propagate", "bspatom_tdse_propagate_dev")


def test_tdse_entry_points_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 16
        assert hasattr(capi.Problem, name[len("bspatom_"):])
        assert "int %s(" % name in header
    names = [L.bspatom_kernel_slot_name(i) for i in range(16)]
    assert names[10] is not None and b"tdse_stage_kernel" in names[10] and names[11] is None
    capi.set_option("tdse_stage_mb", 3)
    assert capi.get_option("tdse_stage_mb") == 3
    capi.set_option("tdse_stage_mb", 0)


def test_tdse_kernels_in_library_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    want = {"tdse_stage_kernel": 12, "tdse_step_kernel": 1, "tdse_pack_kernel": 1, "tdse_unpack_kernel": 1}    # 6 stages x 2 widths
    for key, num in want.items():
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == num, (key, [n for n in ks if "tdse" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


def test_tableau_order_conditions_exact():
    A, B, C, D = host.RK_A, host.RK_B, host.RK_C, host.RK_D
    assert all(isinstance(x, F) for row in A for x in row) and len(A) == len(B) == len(C) == len(D) == 6
    assert C == (F(0), F(2, 9), F(1, 3), F(3, 4), F(1), F(5, 6))
    assert D == (F(47, 450), F(0), F(12, 25), F(32, 225), F(1, 30), F(6, 25))
    assert B == (F(1, 9), F(0), F(9, 20), F(16, 45), F(1, 12), F(0))
    for s in range(6):
        assert len(A[s]) == s and sum(A[s], F(0)) == C[s]
    assert sum(D) == 1 and sum(B) == 1
    for m in range(1, 5):
        assert sum(d * c ** m for d, c in zip(D, C)) == F(1, m + 1), m
    for m in range(1, 4):
        assert sum(b * c ** m for b, c in zip(B, C)) == F(1, m + 1), m
    # the restatement of the tests carries the same numbers
    assert (tdse_ref.A, tdse_ref.B, tdse_ref.C, tdse_ref.D5) == (A, B, C, D)


def test_rk_nodes_and_field_table():
    t = host.rk_nodes(1.5, 0.25, 7)
    assert t.shape == (7, 6) and t.dtype == np.float64
    c = np.array([0.0, 2.0 / 9.0, 1.0 / 3.0, 0.75, 1.0, 5.0 / 6.0])
    for n in range(7):
        assert np.array_equal(t[n], 1.5 + (n + c) * 0.25)
    arr = np.arange(42, dtype=np.float64).reshape(7, 6) * (1 - 2j)
    tab = host.field_table([lambda x: np.sin(x), arr, lambda x: -1j * np.cos(x)], 1.5, 0.25, 7)
    assert tab.shape == (7, 6, 3) and tab.dtype == np.complex128
    assert np.array_equal(tab[:, :, 0], np.sin(t).astype(np.complex128))
    assert np.array_equal(tab[:, :, 1], arr)
    assert np.array_equal(tab[:, :, 2], -1j * np.cos(t))
    with pytest.raises(ValueError):
        host.field_table([np.zeros((7, 5))], 1.5, 0.25, 7)
    assert host.field_table([], 0.0, 0.1, 3).shape == (3, 6, 0)


class _FakeProblem:
    """dipole_matrix / dipole_elements of a problem whose element <lf, f| a . (r, 1/r, d/dr) |li, i> is a fixed formula; records calls"""

    def __init__(self, with_matrix=True):
        self.calls = []
        self.last_E = np.arange(3 * 40, dtype=np.float64).reshape(3, 40) / 7.0
        self.last_l0 = 0
        if with_matrix:
            self.dipole_matrix = self._dipole_matrix

    @staticmethod
    def _elem(li, i, lf, f, a):
        return (a[0] + 2.0 * a[1] - 0.5 * a[2]) * (1.0 + li + 0.25 * lf) / (1.0 + abs(i - f) + 0.125 * i)

    def _dipole_matrix(self, pairs, n0_ini, count_ini, n0_fin, count_fin, a):
        pairs = [tuple(p) for p in pairs]
        self.calls.append(("dipole_matrix", tuple(pairs), n0_ini, count_ini, n0_fin, count_fin))
        a = np.asarray(a)
        return np.array([[[self._elem(li, n0_ini + i, lf, n0_fin + f, a[p]) for f in range(count_fin)] for i in range(count_ini)]
                         for p, (li, lf) in enumerate(pairs)])

    def dipole_elements(self, l_ini, n0_ini, l_fin, n0_fin, count, a):
        self.calls.append(("dipole_elements",))
        return np.array([self._elem(l_ini, n0_ini, l_fin, n0_fin + f, a) for f in range(count)])


@pytest.mark.parametrize("kind_pi", [1, 2])
def test_tdse_system_one_call_and_matelem_unchanged(kind_pi):
    channels = [(0, 0), (1, 0), (2, 0)]
    prob = _FakeProblem()
    E, pairs, D = host.tdse_system(prob, channels, 3, 5, kind_pi=kind_pi)
    assert prob.calls == [("dipole_matrix", ((1, 0), (2, 1)), 3, 5, 3, 5)]
    assert pairs == [(1, 0), (2, 1)] and D.shape == (2, 5, 5)
    assert np.array_equal(E, prob.last_E[:, 2:7])
    # the blocks are the ones dipole_matelem puts into MatElem_All.dat: z[bra f, ket i] = D[p, i, f]
    z = host.dipole_matelem(_FakeProblem(), channels, 7, kind_pi=kind_pi)
    for p, (ket, bra) in enumerate(pairs):
        assert np.array_equal(z[bra * 7 + 2: bra * 7 + 7, ket * 7 + 2: ket * 7 + 7, 0].real, D[p].T)
    # dipole_matelem through the block call equals the per-state route, and the angular factor of s -> p is the known one
    z1 = host.dipole_matelem(_FakeProblem(with_matrix=False), channels, 7, kind_pi=kind_pi)
    assert np.array_equal(z, z1)
    assert np.count_nonzero(z[7:14, 7:14]) == 0 and np.count_nonzero(z[0:7, 14:21]) == 0 and np.count_nonzero(z[7:, :7]) == 0
    if kind_pi == 1:
        blocks = host.dipole_blocks(channels, 1, 0)
        assert [(b[0], b[1], b[2], b[3]) for b in blocks] == [(0, 1, 1, 0), (1, 2, 2, 1)]
        assert abs(abs(blocks[0][5][0]) - 1.0 / np.sqrt(3.0)) < 1e-15 and blocks[0][4] == 1.0
        assert abs(abs(blocks[1][5][0]) - 2.0 / np.sqrt(15.0)) < 1e-15
    with pytest.raises(ValueError):
        host.tdse_system(object(), channels, 1, 2)


def test_tdse_coeffs_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((3, 11)) + 1j * rng.standard_normal((3, 11))) * 10.0 ** rng.integers(-30, 3, size=(3, 11))
    a[0, 0], a[1, 1] = 0.0, complex(np.nextafter(1.0, 2.0), -5e-324)
    path = str(tmp_path / "TDSE_COEFFs.dat")
    host.write_tdse_coeffs(path, a)
    lines = open(path).read().splitlines()
    assert len(lines) == 33 and all(len(ln.split()) == 3 for ln in lines)
    assert [int(ln.split()[0]) for ln in lines[:12]] == list(range(1, 12)) + [1]
    b = host.read_tdse_coeffs(path, 33)
    assert np.array_equal(b.view(np.uint64), a.reshape(-1).view(np.uint64))
    with pytest.raises(ValueError):
        host.read_tdse_coeffs(path, 34)


def test_restatement_is_fifth_order():
    """2 x 2 constant-field problem against the closed form from eigh: halving the step divides the error by 24 .. 40."""
    errs = []
    for nsteps in (50, 100, 200):
        E, pairs, D, a0, field, dt, exact = tdse_ref.two_by_two(nsteps)
        a, est = tdse_ref.propagate(E, pairs, D, a0, field, dt)
        errs.append(float(np.max(np.abs(a - exact))))
    for lo, hi in zip(errs[1:], errs[:-1]):
        assert 24.0 <= hi / lo <= 40.0, errs
    assert np.finfo(np.longdouble).eps < 2e-19
