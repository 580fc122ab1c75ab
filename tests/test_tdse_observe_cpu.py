"""bspatom_tdse_observe without a GPU: the entry points are bound and in the header, the kernels of the measuring stage are in the
library with no scratch and no spilled VGPRs, host.obs_steps / tdse_expectations, and the NumPy restatement of the observables
(tests/tdse_obs_ref.py) against a plain triple loop."""
import os
import sys
import numpy as np
import pytest
from conftest import ROOT

import tdse_obs_ref
from bspatom_amd import capi, host

NAMES = ("bspatom_tdse_observe", "bspatom_tdse_observe_dev")


def test_observe_entry_points_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 18
        assert hasattr(capi.Problem, name[len("bspatom_"):])
        assert "int %s(" % name in header
    # the propagate pair keeps its 16 arguments
    assert len(L.bspatom_tdse_propagate.argtypes) == 16 and len(L.bspatom_tdse_propagate_dev.argtypes) == 16


def test_observe_kernels_in_library_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    want = {"tdse_observe_kernel": 2, "tdse_obs_reduce_kernel": 1}            # the two widths of stage 0
    for key, num in want.items():
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == num, (key, [n for n in ks if "tdse" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


def test_obs_steps_and_expectations():
    assert host.obs_steps(0, 1) == [0]
    assert host.obs_steps(10, 5) == [0, 5, 10]
    assert host.obs_steps(10, 4) == [0, 4, 8, 10]
    assert host.obs_steps(1, 7) == [0, 1]
    for nsteps, m in ((0, 1), (0, 3), (1, 1), (1, 7), (10, 5), (10, 4), (40, 7), (60, 1)):
        assert len(host.obs_steps(nsteps, m)) == capi.Problem.tdse_nobs(nsteps, m)
        assert len(host.obs_steps(nsteps, m)) == (1 if nsteps == 0 else (nsteps - 1) // m + 2)
    with pytest.raises(ValueError):
        host.obs_steps(3, 0)
    obs = np.arange(2 * 3 * 5 * 4, dtype=np.float64).reshape(2, 3, 5, 4)
    norm, h0, dre, dim = host.tdse_expectations(obs)
    assert norm.shape == (2, 3)
    assert np.array_equal(norm, obs[..., 0].sum(-1)) and np.array_equal(h0, obs[..., 1].sum(-1))
    assert np.array_equal(dre, 2.0 * obs[..., 2].sum(-1)) and np.array_equal(dim, 2.0 * obs[..., 3].sum(-1))


def test_restatement_against_a_triple_loop():
    """2 channels of 3 states, small integers (every sum is exact in any order): observables equals the definitions written as loops;
    the pair the other way round with the transposed block gives the complex conjugate of z."""
    rng = np.random.default_rng(5)
    E = rng.integers(-4, 5, size=(2, 3)).astype(np.float64)
    D = rng.integers(-4, 5, size=(1, 3, 3)).astype(np.float64)
    a = (rng.integers(-4, 5, size=(2, 2, 3)) + 1j * rng.integers(-4, 5, size=(2, 2, 3))).astype(np.complex128)
    got = tdse_obs_ref.observables(E, [(0, 1)], D, a)
    assert got.shape == (2, 2, 4) and got.dtype == np.float64
    want = np.zeros((2, 2, 4))
    for q in range(2):
        for c in range(2):
            for n in range(3):
                p2 = a[q, c, n].real ** 2 + a[q, c, n].imag ** 2
                want[q, c, 0] += p2
                want[q, c, 1] += E[c, n] * p2
        z = 0.0
        for i in range(3):
            for f in range(3):
                z += np.conj(a[q, 1, f]) * D[0, i, f] * a[q, 0, i]
        want[q, 1, 2], want[q, 1, 3] = z.real, z.imag
    assert np.array_equal(got, want)
    assert np.count_nonzero(got[:, 1, 2:]) > 0 and np.count_nonzero(got[:, 0, 2:]) == 0
    rev = tdse_obs_ref.observables(E, [(1, 0)], np.ascontiguousarray(D.transpose(0, 2, 1)), a)
    zf = got[..., 2].sum(-1) + 1j * got[..., 3].sum(-1)
    zr = rev[..., 2].sum(-1) + 1j * rev[..., 3].sum(-1)
    assert np.array_equal(zr, np.conj(zf)) and np.array_equal(rev[..., :2], got[..., :2])
    # leading dimensions pass through, the long-double form agrees, and the magnitudes dominate
    g2 = tdse_obs_ref.observables(E, [(0, 1)], D, a[None], np.longdouble, np.clongdouble)
    assert g2.shape == (1, 2, 2, 4) and g2.dtype == np.longdouble and np.array_equal(g2[0].astype(np.float64), got)
    M = tdse_obs_ref.magnitudes(E, [(0, 1)], D, a)
    assert M.shape == (4,) and M.dtype == np.longdouble
    assert np.all(np.abs(got).reshape(-1, 4).max(axis=0) <= M)
    assert M[0] == np.max(got[..., 0])
