"""Band reduction with its diagonal blocks stored as packed lower triangles (csrc/crawford.hip): a storage layout, so the band and
the spectra are, bit for bit, what the commit before it computed -- tests/golden/cw_dpack_parent.npz, recorded there by
tools/record_cw_dpack.py on the cases of tools/cw_dpack_cases.py (the smallest shapes at which the layout can go wrong: four blocks,
a ragged last block, waves with four items, narrower pencils, two stream groups)."""
import os
import sys

import numpy as np
import pytest
from conftest import load_golden, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import cw_dpack_cases as cs  # noqa: E402
from bspatom_amd import capi  # noqa: E402
from test_gpu_solve import _Options  # noqa: E402
from test_gpu_stages import _band_eigs, _dense_upper, note  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [cs.tag(*c) for c in cs.CASES]
_cache = {}


def _golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("cw_dpack_parent")
    return _cache["g"]


def _inputs(case):
    """the case's pencil (checked against the digest of what the recorder fed the library) and its hydrogen problem, made once"""
    if case not in _cache:
        n, k, nl = case
        SB, HB = cs.pencil(n, k, nl)
        assert np.array_equal(cs.digest(np.concatenate([SB.ravel(), HB.ravel()])), _golden()[cs.tag(*case) + "/inputs_sha"]), \
            "the random pencil is not the recorded one: the fixture cannot be compared"
        _cache[case] = (SB, HB)
    return _cache[case]


def _run3(case, **opts):
    """band (trimmed) and spectra under the switches, three times over, equal each time"""
    n, k, nl = case
    SB, HB = _inputs(case)
    prob = capi.Problem(capi.make_input(**cs.hydrogen(n, k, nl)))
    try:
        with _Options(**opts):
            assert prob.route() == 2
            out = []
            for _ in range(3):
                AB, info = capi.stage_crawford(SB, HB)
                E, inf = prob.solve(0, nl)
                assert info == 0 and np.all(inf == 0), (case, opts, info, inf)
                out.append((cs.trimmed(AB, n), E))
    finally:
        prob.close()
    for A, E in out[1:]:
        assert np.array_equal(A, out[0][0]) and np.array_equal(E, out[0][1]), ("not the same from run to run", case, opts)
    return out[0]


def _same_as_recorded(case, variant, A, E, what):
    g, t = _golden(), cs.tag(*case)
    n, k, nl = case
    keep, nc = cs.kept_channels(k, nl, variant), cs.band_cols(variant)
    ref, Eref = g["%s/%s/band" % (t, variant)], g["%s/%s/spectra" % (t, variant)]
    assert np.all(A[:, :, nc:] == 0.0), (t, what)
    for i, ch in enumerate(keep):                                         # first where, then whether everywhere
        assert np.array_equal(A[ch, :, :nc], ref[i]), (t, what, "band of channel %d" % ch, np.max(np.abs(A[ch, :, :nc] - ref[i])))
    assert np.array_equal(cs.digest(A), g["%s/%s/band_sha" % (t, variant)]), (t, what, "band, a channel the fixture holds no copy of")
    Ecmp = E if variant == "default" else E[keep]
    assert np.array_equal(Ecmp, Eref), (t, what, "spectra", np.max(np.abs(Ecmp - Eref)))
    assert np.array_equal(cs.digest(E), g["%s/%s/spectra_sha" % (t, variant)]), (t, what, "spectra")


@pytest.mark.parametrize("case", cs.CASES, ids=IDS)
@pytest.mark.parametrize("variant", list(cs.RECORDED))
def test_recorded_bits(case, variant):
    """default switches, one division per reflector, half-width 15 handed over: each against its own recording"""
    A, E = _run3(case, **cs.RECORDED[variant])
    _same_as_recorded(case, variant, A, E, variant)


@pytest.mark.parametrize("case", cs.CASES, ids=IDS)
@pytest.mark.parametrize("name,opts", cs.SAME_BITS, ids=[s[0] for s in cs.SAME_BITS])
def test_switches_that_change_no_bit(case, name, opts):
    """the reflector row through LDS, four waves per workgroup, one or two items per wave: the default's recording"""
    A, E = _run3(case, **opts)
    _same_as_recorded(case, "default", A, E, name)


def test_factor_in_chunks():
    """n = 256 with the S-only part handed over in CW_CHUNKS pieces (from 1024 functions on by default): the same spectra"""
    case = (256, 9, 33)
    A, E = _run3(case, cw_chunk_min=128)
    _same_as_recorded(case, "default", A, E, "cw_chunk_min=128")


@pytest.mark.parametrize("case", cs.CASES, ids=IDS)
def test_one_item_per_wave_to_rounding(case):
    """cw_items4=0 (crawford_item_kernel, the cross-check on the same layout): another summation order, the default's spectra to
    the bound of test_band_route_properties, 1e-13 of |lambda|_max"""
    A, E = _run3(case, cw_items4=0)
    E0 = _golden()[cs.tag(*case) + "/default/spectra"]
    lam = np.max(np.abs(E0))
    err = np.max(np.abs(E - E0)) / lam
    note("packed D, %s: one item per wave vs four, spectra: %.2e of |lambda|_max" % (cs.tag(*case), err))
    assert err <= 1e-13


def test_run_from_both_ends():
    """cw_split=50 at n = 128 (8 blocks a part): the flipped block at the cut is the mirror image of a lower triangle now, its last
    bits may move -- the tolerance of test_crawford_band against scipy's solver on the same pencil, for both item kernels"""
    import scipy.linalg as sla
    case = (128, 9, 5)
    n, k, nl = case
    SB, HB = _inputs(case)
    for kw in (dict(cw_split=50), dict(cw_split=50, cw_items4=0)):
        with _Options(**kw):
            AB, info = capi.stage_crawford(SB, HB)
            AB2, _ = capi.stage_crawford(SB, HB)
        assert info == 0 and np.array_equal(AB, AB2) and np.all(AB[:, :, 9:] == 0.0)
        assert not np.array_equal(cs.digest(cs.trimmed(AB, n)), _golden()[cs.tag(*case) + "/default/band_sha"])   # it did split
        for l in range(nl):
            ref = sla.eigh(_dense_upper(HB[l]), _dense_upper(SB), eigvals_only=True)
            err = np.max(np.abs(_band_eigs(AB[l], n, 8) - ref)) / np.max(np.abs(ref))
            note("packed D, from both ends, n %d l %d %s: band vs scipy eigh(H, S): %.2e of |lambda|_max" % (n, l, kw, err))
            assert err < 2e-14 * np.sqrt(n)
