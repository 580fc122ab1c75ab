"""Matrix elements of caller-given radial operators (bspatom_operator_bands / bspatom_operator_matrix) without a GPU: the
four entry points are bound, the two kernels of csrc/opmat.hip are in the library with no scratch and no spilled VGPRs, and
host.operator_matrix turns a list of (g, deriv) into exactly one Problem.operator_matrix call."""
import os
import sys
import numpy as np
import pytest
from conftest import ROOT

from bspatom_amd import capi, host

NAMES = ("bspatom_operator_bands", "bspatom_operator_bands_dev", "bspatom_operator_matrix", "bspatom_operator_matrix_dev")


def test_operator_entry_points_bound():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert getattr(L, name).argtypes is not None
        assert hasattr(capi.Problem, name[len("bspatom_"):])
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header


def test_operator_kernels_in_library_without_scratch_or_spills():
    """operator_band_kernel and band_combine_apply_kernel (csrc/opmat.hip) in the code-object notes of libbspatom.so: private
    segment 0, VGPR spills 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    for key in ("operator_band_kernel", "band_combine_apply_kernel"):
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == 1, (key, [n for n in ks if "operator" in n or "combine" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


class _FakeProblem:
    """quadrature() and operator_matrix() of a problem with 24 quadrature points; records its calls"""
    NR = 24

    def __init__(self):
        self.calls = []
        self.r = np.linspace(0.25, 6.0, self.NR)

    def quadrature(self):
        self.calls.append(("quadrature",))
        return self.r.copy(), np.full(self.NR, 0.25)

    def operator_matrix(self, pairs, g, deriv, n0_ini, count_ini, n0_fin, count_fin, a):
        pairs = [tuple(p) for p in pairs]
        self.calls.append(("operator_matrix", tuple(pairs), n0_ini, count_ini, n0_fin, count_fin))
        self.g, self.deriv, self.a = np.array(g), np.array(deriv), np.array(a)
        return np.zeros((len(pairs), count_ini, count_fin))


def test_host_operator_matrix_makes_one_call_with_the_operators_on_the_grid():
    prob = _FakeProblem()
    arr = np.arange(_FakeProblem.NR, dtype=np.float64) - 7.0
    ops = [(lambda r: r ** 2, False), (arr, True), (lambda r: np.exp(-r / 5.0), 1)]
    pairs = [(0, 1), (1, 2)]
    a = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    D = host.operator_matrix(prob, pairs, ops, 2, 5, 3, 7, a)
    assert D.shape == (2, 5, 7)
    om = [c for c in prob.calls if c[0] == "operator_matrix"]
    assert om == [("operator_matrix", ((0, 1), (1, 2)), 2, 5, 3, 7)]
    assert prob.g.shape == (3, _FakeProblem.NR) and prob.g.dtype == np.float64
    assert np.array_equal(prob.g[0], prob.r ** 2)                    # callables on quadrature()[0]
    assert np.array_equal(prob.g[1], arr)                            # arrays passed through
    assert np.array_equal(prob.g[2], np.exp(-prob.r / 5.0))
    assert prob.deriv.tolist() == [0, 1, 1]
    assert np.array_equal(prob.a, a)
    # one coefficient vector for every pair goes through as it is (Problem.operator_matrix broadcasts it)
    host.operator_matrix(prob, pairs, ops, 1, 1, 1, 1, [1.0, 0.5, 0.25])
    assert prob.a.tolist() == [1.0, 0.5, 0.25]
    # a=None: one operator, coefficient 1
    prob = _FakeProblem()
    host.operator_matrix(prob, pairs, [(arr, False)], 1, 2, 1, 2)
    assert len([c for c in prob.calls if c[0] == "operator_matrix"]) == 1
    assert prob.a.tolist() == [1.0] and prob.deriv.tolist() == [0]


def test_host_operator_matrix_value_errors():
    prob = _FakeProblem()
    ok = np.ones(_FakeProblem.NR)
    with pytest.raises(ValueError):
        host.operator_matrix(prob, [(0, 1)], [(np.ones(_FakeProblem.NR + 1), False)], 1, 1, 1, 1)       # wrong-sized array
    with pytest.raises(ValueError):
        host.operator_matrix(prob, [(0, 1)], [(lambda r: r[:-1], False)], 1, 1, 1, 1)                   # wrong-sized callable result
    with pytest.raises(ValueError):
        host.operator_matrix(prob, [(0, 1)], [(ok, False), (ok, True)], 1, 1, 1, 1)                     # a=None with two operators
    with pytest.raises(ValueError):
        host.operator_matrix(prob, [(0, 1)], [(ok, False), (ok, True)], 1, 1, 1, 1, a=[1.0, 2.0, 3.0])  # a of the wrong length
    with pytest.raises(ValueError):
        host.operator_matrix(prob, [(0, 1)], [], 1, 1, 1, 1)                                            # no operator
    assert not [c for c in prob.calls if c[0] == "operator_matrix"]
