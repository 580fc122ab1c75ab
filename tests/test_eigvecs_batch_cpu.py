"""Eigenvector blocks of a batch of channels (bspatom_eigvecs_batch) without a GPU: the kernel is in the library with no
scratch and no spilled VGPRs, and the Eigenvec_All.dat writer takes the batched call when the problem has it."""
import os
import sys
import numpy as np
from conftest import ROOT

from bspatom_amd import capi, host


def test_batch_kernel_in_library_without_scratch_or_spills():
    """invit_batch_kernel<8> and <15> (csrc/eigvec.hip) in the code-object notes of libbspatom.so: private segment 0,
    VGPR spills 0, and at most 168 VGPRs -- three waves per SIMD, the occupancy the persistent grid is sized by."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    for bt in (8, 15):
        hits = [v for name, v in ks.items() if "invit_batch_kernel<%d>" % bt in name]
        assert len(hits) == 1, (bt, [n for n in ks if "invit_batch" in n])
        v = hits[0]
        assert (v["private_segment_fixed_size"] or 0) == 0, v
        assert (v["vgpr_spill_count"] or 0) == 0, v
        assert v["vgpr_count"] <= 168, v


def test_batch_entry_points_bound():
    L = capi.lib()
    assert "bspatom_eigvecs_batch" in capi.EXPORTS and "bspatom_eigvecs_batch_dev" in capi.EXPORTS
    assert hasattr(L, "bspatom_eigvecs_batch") and hasattr(L, "bspatom_eigvecs_batch_dev")
    assert hasattr(capi.Problem, "eigvecs_batch") and hasattr(capi.Problem, "eigvecs_batch_dev")


class _PerChannel:
    nfun = 6

    def __init__(self):
        self.calls = []

    def eigvecs(self, l, n0, count):
        self.calls.append(("eigvecs", l, n0, count))
        rng = np.random.default_rng(100 + l)
        Z = rng.standard_normal((self.nfun, self.nfun)) * 10.0 ** rng.integers(-12, 3, size=(self.nfun, 1))
        return Z[n0 - 1: n0 - 1 + count]


class _Batched(_PerChannel):
    def eigvecs_batch(self, l0, nl, n0, count):
        self.calls.append(("eigvecs_batch", l0, nl, n0, count))
        return np.stack([_PerChannel.eigvecs(self, l, n0, count) for l in range(l0, l0 + nl)])


def test_write_eigenvec_all_batched_and_per_channel_identical(tmp_path, monkeypatch):
    """The same text through eigvecs_batch as through eigvecs; the batched problem is asked once per group of channels
    (every channel exactly once), the per-channel one once per channel."""
    pa, pb = tmp_path / "a.dat", tmp_path / "b.dat"
    per, bat = _PerChannel(), _Batched()
    host.write_eigenvec_all(str(pa), per, 4, 5)
    host.write_eigenvec_all(str(pb), bat, 4, 5)
    assert open(pa).read() == open(pb).read()
    assert [c[0] for c in per.calls] == ["eigvecs"] * 5
    assert bat.calls[0] == ("eigvecs_batch", 0, 5, 1, 5)
    assert sum(c[2] for c in bat.calls if c[0] == "eigvecs_batch") == 5
    # groups bounded in bytes: 2 channels of 5 x 6 doubles per group -> calls at l = 0, 2, 4
    monkeypatch.setattr(host, "EIGVECS_GROUP_BYTES", 2 * 5 * 6 * 8)
    bat2 = _Batched()
    pc = tmp_path / "c.dat"
    host.write_eigenvec_all(str(pc), bat2, 4, 5)
    assert open(pc).read() == open(pa).read()
    assert [c for c in bat2.calls if c[0] == "eigvecs_batch"] == [("eigvecs_batch", 0, 2, 1, 5), ("eigvecs_batch", 2, 2, 1, 5),
                                                                  ("eigvecs_batch", 4, 1, 1, 5)]
