"""bspatom_tdse_lawson without a GPU: the entry points are bound and in the header, and the Lawson kernels of csrc/tdse.hip are in the
library for every stage and both widths with no scratch and no spilled VGPRs."""
import os
import sys
from conftest import ROOT

from bspatom_amd import capi

NAMES = ("bspatom_tdse_lawson", "bspatom_tdse_lawson_dev")


def test_entry_points_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 18
        assert getattr(L, name).argtypes == L.bspatom_tdse_observe.argtypes
        assert hasattr(capi.Problem, name[len("bspatom_"):])
        assert "int %s(" % name in header


def test_kernels_in_library_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    want = {"tdse_lawson_stage_kernel": 12, "tdse_lawson_observe_kernel": 2, "tdse_lawson_step_kernel": 1, "tdse_phase_kernel": 1}
    for key, num in want.items():
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == num, (key, [n for n in ks if "tdse" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)
