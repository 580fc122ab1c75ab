"""Dipole matrix blocks of many channel pairs (bspatom_dipole_matrix) without a GPU: the entry points are bound, the two
kernels are in the library with no scratch and no spilled VGPRs, and host.dipole_matelem takes the one-call path when the
problem has it."""
import os
import sys
import numpy as np
from conftest import ROOT

from bspatom_amd import capi, host


def test_dipole_matrix_entry_points_bound():
    L = capi.lib()
    for name in ("bspatom_dipole_matrix", "bspatom_dipole_matrix_dev"):
        assert name in capi.EXPORTS
        assert hasattr(L, name)
    assert hasattr(capi.Problem, "dipole_matrix") and hasattr(capi.Problem, "dipole_matrix_dev")


def test_dipole_kernels_in_library_without_scratch_or_spills():
    """band_apply_block_kernel and both instances of dipole_block_kernel (csrc/dipole.hip) in the code-object notes of
    libbspatom.so: private segment 0, VGPR spills 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    for key, inst in (("band_apply_block_kernel", 1), ("dipole_block_kernel", 2)):
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == inst, (key, [n for n in ks if "dipole" in n or "band_apply" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


class _PerState:
    """a problem that exposes dipole_elements only: host.dipole_matelem takes its per-state loop"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _block(l_ini, l_fin, a):
        # 12 x 12 "elements" of the pair, spread over many magnitudes, linear in the coefficients as the real ones are
        rng = np.random.default_rng(1000 * l_ini + l_fin)
        B = rng.standard_normal((3, 12, 12)) * 10.0 ** rng.integers(-9, 3, size=(3, 12, 12))
        return a[0] * B[0] + a[1] * B[1] + a[2] * B[2]

    def dipole_elements(self, l_ini, n0_ini, l_fin, n0_fin, count, a):
        self.calls.append(("dipole_elements", l_ini, n0_ini, l_fin, n0_fin, count))
        return self._block(l_ini, l_fin, np.asarray(a, dtype=np.float64))[n0_ini - 1, n0_fin - 1: n0_fin - 1 + count]


class _OneCall(_PerState):
    def dipole_matrix(self, pairs, n0_ini, count_ini, n0_fin, count_fin, a):
        pairs = list(pairs)
        self.calls.append(("dipole_matrix", tuple(pairs), n0_ini, count_ini, n0_fin, count_fin))
        a = np.asarray(a, dtype=np.float64)
        assert a.shape == (len(pairs), 3)
        return np.stack([self._block(li, lf, a[p])[n0_ini - 1: n0_ini - 1 + count_ini, n0_fin - 1: n0_fin - 1 + count_fin]
                         for p, (li, lf) in enumerate(pairs)])


def test_dipole_matelem_one_call_and_per_state_identical():
    """The same z through dipole_matrix as through the dipole_elements loop, both gauges; the problem with dipole_matrix sees
    exactly one call of it, over the pairs b_ >= a_, |li - lj| = 1 (ket = initial, bra = final), and no dipole_elements call."""
    channels = [(0, 0), (1, 0), (2, 0), (1, 1), (3, 1)]
    n1 = 7
    for kind_pi in (1, 2):
        per, one = _PerState(), _OneCall()
        za = host.dipole_matelem(per, channels, n1, kind_pi=kind_pi)
        zb = host.dipole_matelem(one, channels, n1, kind_pi=kind_pi)
        assert np.array_equal(za, zb)
        assert np.max(np.abs(za)) > 0
        want = [(lj, li) for a_, (li, mi) in enumerate(channels) for b_, (lj, mj) in enumerate(channels)
                if b_ >= a_ and abs(li - lj) == 1]
        assert len(one.calls) == 1
        assert one.calls[0] == ("dipole_matrix", tuple(want), 1, n1, 1, n1)
        assert [c[0] for c in per.calls] == ["dipole_elements"] * (len(want) * n1)
