"""The spline-basis TDSE for wide bands (bspatom_tdse_spline_wide / _dev, csrc/tdse_spline_wide.hip) without a GPU: the names and
where they are declared, host.spline_propagate's choice between the narrow and the wide call, the code-object notes of the two
kernels on the blocked LU, the launch-length rule restated, and the physics the GPU file runs -- the norm under a Hermitian
17-channel coupling -- on the dense restatement tests/tdse_spline_ref.py.  Bands from the oracle on the n65_k4 grid."""
import os
import re
import sys
import numpy as np
import pytest
from conftest import ROOT

import oracle as orc
import tdse_spline_wide_ref as wref
from bspatom_amd import capi, host

EPS = np.finfo(np.float64).eps
KW = dict(kind_grid=0, ra=0.0, rb=40.0, k=4, nfun=65, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)   # n65_k4
WIDE = ["bspatom_tdse_spline_wide", "bspatom_tdse_spline_wide_dev"]
# the dense restatement's own drift of sum_ch N_ch over 5 steps, relative to max(1, norm): a Cayley step is exactly unitary in the
# S-norm, so what is left is rounding -- per step the solve's backward error (LAPACK's, of the order of eps) enters the norm twice
# (c^H S dc and its conjugate), and every row is itself a float64 sum evaluated to about 2 eps of its value: (2 nsteps + 4) eps.
DENSE_DRIFT_BOUND = (2 * wref.NORM_STEPS + 4) * EPS


def test_names_are_bound_and_declared_in_the_spline_part():
    L = capi.lib()
    for name in WIDE:
        assert name in capi.SPLINE_EXPORTS and name not in capi.EXPORTS
        assert hasattr(L, name)
        assert getattr(L, name).argtypes == L.bspatom_tdse_spline.argtypes and len(getattr(L, name).argtypes) == 24
    assert hasattr(capi.Problem, "tdse_spline_wide") and hasattr(capi.Problem, "tdse_spline_wide_dev") and hasattr(host, "spline_propagate")
    assert host.COUPLED_WIDE_MAX_BAND == 255 and host.COUPLED_MAX_BAND == 63
    inc = os.path.join(ROOT, "include")
    part = open(os.path.join(inc, "bspatom_tdse_spline.h")).read()
    main = open(os.path.join(inc, "bspatom.h")).read()
    for name in WIDE:
        assert re.search(r"\b%s\s*\(" % name, part) and not re.search(r"\b%s\s*\(" % name, main)
    assert "#define BSPATOM_COUPLED_WIDE_MAX_BAND 255" in re.sub(r"[ \t]+", " ", main)
    # the comment states what differs
    for text in ("BSPATOM_COUPLED_WIDE_MAX_BAND", "bspatom_resolvent_coupled_wide", "27.6e9", "NOT promised"):
        assert text in part[part.index("blocked LU for wide bands"):], text


class _Stub:
    """a problem that records which of the two calls spline_propagate takes"""
    def __init__(self, k):
        self.k, self.nfun, self.calls = k, 8, []

    def tdse_spline(self, l, c0, dt, nsteps, **kw):
        self.calls.append(("narrow", len(l), dt, nsteps, kw))
        return "narrow"

    def tdse_spline_wide(self, l, c0, dt, nsteps, **kw):
        self.calls.append(("wide", len(l), dt, nsteps, kw))
        return "wide"


def test_spline_propagate_routes_by_half_width():
    """nch k - 1 = 63 is the narrow call's, 64 and 255 the wide one's, 256 a ValueError; the arguments pass through"""
    for k, nch, want in ((16, 4, "narrow"), (8, 8, "narrow"), (5, 13, "wide"), (13, 5, "wide"), (16, 16, "wide"), (4, 64, "wide"), (9, 7, "narrow"), (9, 8, "wide")):
        bw = nch * k - 1
        assert (want == "narrow") == (bw <= 63) and bw <= 255, (k, nch)
        p = _Stub(k)
        got = host.spline_propagate(p, list(range(nch)), np.zeros((nch, 8)), 0.05, 3, obs_every=2, coef=None)
        assert got == want and p.calls == [(want, nch, 0.05, 3, dict(obs_every=2, coef=None))], (k, nch, p.calls)
    assert [nch * k - 1 for k, nch in ((16, 4), (5, 13), (16, 16))] == [63, 64, 255]
    for k, nch in ((1, 257), (16, 17), (257, 1)):                # 256, 271, 256
        p = _Stub(k)
        with pytest.raises(ValueError, match="255"):
            host.spline_propagate(p, list(range(nch)), np.zeros((nch, 8)), 0.05, 1)
        assert p.calls == []


def test_wide_kernels_in_library_without_scratch_or_spills():
    """tdse_spline_wide_kernel and resolvent_wide_kernel (both on csrc/resolvent_wide_lu.h) in the code-object notes of libbspatom.so:
    private segment 0, VGPR spills 0 -- the blocked LU spilled heavily in earlier forms"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    for key in ("tdse_spline_wide_kernel", "resolvent_wide_kernel"):
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == 1, (key, [n for n in ks if "wide" in n])
        v = hits[0]
        assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
        assert (v["vgpr_spill_count"] or 0) == 0, (key, v)
        assert v["vgpr_count"] <= 256, (key, v)                   # 512 threads: one workgroup per CU needs two waves per SIMD


def test_launch_length_rule():
    """the largest g in 1 .. 64 with g ceil(nscan / slots) 16 N bw^2 <= 27.6e9: within 1 .. 64 everywhere; 64 for the GPU test's shapes
    at one scan per slot (its default), except at the limit bw = 255, where 16 N bw^2 = 6.66e8 flop per step give 41 -- still more than
    the two steps of that case, so every case runs as ONE multi-step launch by default; under resolvent_slots = 2 (three scans on a
    slot) 13.  A long run at nfun = 1024 and bw = 255 gets one step per launch."""
    for N in (2, 100, 1105, 28672, 1 << 20):
        for bw in (1, 63, 64, 143, 255):
            for nscan, slots in ((1, 1), (5, 2), (64, 64), (1000, 256)):
                g = wref.launch_group(N, bw, nscan, slots)
                work = -(-nscan // slots) * 16.0 * N * bw * bw
                assert 1 <= g <= 64
                assert g == 1 or g * work <= 27.6e9
                assert g == 64 or (g + 1) * work > 27.6e9
    got = [wref.launch_group(nch * n, nch * k - 1, wref.NSCAN, wref.NSCAN) for _, nch, _, k, n in wref.SHAPES]
    assert got == [64, 64, 64, 64, 41], got
    assert all(g >= nsteps > 1 for g, (_, _, nsteps, _, _) in zip(got, wref.SHAPES))
    assert wref.launch_group(16 * 40, 255, wref.NSCAN, 2) == 13
    assert wref.launch_group(28 * 1024, 251, 1, 1) == 1


def test_norm_under_a_hermitian_coupling_on_the_dense_restatement():
    """n65_k4, nch = 17 (bw = 67), every neighbour pair coupled in both directions (the second the transposed entry with the conjugate
    coefficient), 5 steps: the matrix is Hermitian to the bit, population moves between the channels, and sum_ch N_ch stays within
    DENSE_DRIFT_BOUND = 14 eps of its start (measured: 1.9 eps).  The GPU test allows the kernel 8 times the dense value, floored at 8 eps."""
    import tdse_spline_ref as sref
    c = orc.make_cfg(**KW)
    rt, aind, xg, wg = orc.grid(c)
    SB, HB = orc.assemble_bands(c, rt, aind, xg, wg, 0, 2)
    RB = orc.dipole_bands(c, rt, aind, xg, wg)
    G2 = np.stack([RB[0], RB[2]])
    l, cp, coef = wref.hermitian_system()
    assert len(l) * c.k - 1 == 67
    A = sref.hamiltonian(SB, HB, l, cp, G2, coef[0])
    assert np.array_equal(A, A.conj().T) and np.max(np.abs(A - sref.hamiltonian(SB, HB, l))) > 0.1
    _, _, rows = sref.propagate(SB, HB, l, wref.DT, wref.norm_packet(c.nfun), coef, cp, G2)
    drift, tot = wref.norm_drift(rows)
    assert (drift, tot) == wref.norm_drift_dense(SB, HB, G2)
    print("dense: norm %.15f  drift %.3e = %.2f eps  population moved %.3e" % (tot, drift, drift / EPS, np.max(np.abs(rows[-1] - rows[0]))))
    assert np.max(np.abs(rows[-1, :17] - rows[0, :17])) > 1e-4    # the coupling did move population
    assert drift <= DENSE_DRIFT_BOUND * max(1.0, tot), (drift, tot)
