"""Two problem handles alive at once on one host thread (include/bspatom.h: "one host thread per problem"): every stream, event
and scratch block the launchers of a solve need belongs to the handle (csrc/common.h: LaunchCtx), so creating, solving and
destroying a second problem of another size changes no bit of the first one's spectra.

Problem A: nfun = 256, k = 7, 32 channels; problem B: nfun = 128, k = 9, 16 channels -- nothing sized for one fits the other.
32 channels is the smallest batch at which the band reduction takes a second stream and sy2sb a second lane.  The chase runs
rings of at least two workgroups per channel at these sizes (BSP_SB2ST_DIAG=1 / BSP_SB2ST_CHECK=1 print them: band route 4 (A)
and 2 (B) members, dense route 2 and 2, two-step dense route 8 and 4).  No concurrent threads: the chase kernels size their rings
for the whole chip."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
from bspatom_amd import capi

KW_A = dict(kind_grid=0, ra=0.0, rb=100.0, k=7, nfun=256, l_fin=31, n0_ini=1, l_ini=0, zatom=1.0)
KW_B = dict(kind_grid=0, ra=0.0, rb=50.0, k=9, nfun=128, l_fin=15, n0_ini=1, l_ini=0, zatom=1.0)

CASES = [pytest.param(dict(route=2), id="band-route"),
         pytest.param(dict(route=2, bisect_queue=2), id="band-route-bisect-queue"),
         pytest.param(dict(route=1), id="dense-route"),
         pytest.param(dict(route=1, sb2st_version=9), id="dense-route-two-step-chase")]


def _solve(prob, nl):
    E, info = prob.solve(0, nl)
    assert np.all(info == 0)
    return E


@pytest.mark.parametrize("opts", CASES)
def test_two_problems_alive(opts):
    old = {k: capi.get_option(k) for k in opts}
    A = B = B2 = None
    try:
        for k, v in opts.items():
            capi.set_option(k, v)
        A = capi.Problem(capi.make_input(**KW_A))
        assert A.lmax + 1 == 32 and A.route() == opts["route"]
        E_A = _solve(A, 32)                                      # A alone
        B = capi.Problem(capi.make_input(**KW_B))
        assert B.lmax + 1 == 16 and B.route() == opts["route"]
        E_B = _solve(B, 16)
        assert np.array_equal(_solve(A, 32), E_A), "A after B was created and solved"
        B.close()
        assert np.array_equal(_solve(A, 32), E_A), "A after B was destroyed"
        B2 = capi.Problem(capi.make_input(**KW_B))
        assert np.array_equal(_solve(B2, 16), E_B), "a fresh B beside A"
        A.close()
        assert np.array_equal(_solve(B2, 16), E_B), "the fresh B after A was destroyed"
    finally:
        for k, v in old.items():
            capi.set_option(k, v)
        for p in (A, B, B2):
            if p is not None:
                p.close()
