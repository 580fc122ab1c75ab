"""The band route's chase on tiles of 8 (csrc/sbr2.hip::sbr_rows_kernel<8>) with the reflector and z reaching the FMAs as DPP operands
(option sbr_xdpp: 1 = z of the diagonal-tile wave, 2 = that wave's reflector as well, 3 = the reflector in all three roles): every
product and every rounding is that of the LDS forms, so every spectrum must equal, bit for bit, the one sbr_xdpp=0 gives.  A wrong
broadcast (a bank mask the hardware does not honour on a 64-bit DPP operation, a lane of the other item) gives other numbers."""
import numpy as np
import pytest
from test_gpu_solve import _Options
from test_gpu_chase8_phased import CASES, RINGS, _problem, _solve

pytestmark = pytest.mark.gpu

SETTINGS = (1, 2, 3)
# besides the rings and fall-backs: the general loop (which keeps the LDS forms whatever the switch says) and the two forced lags
OTHERS = [dict(sbr_phased=0), dict(sbr_lag=1), dict(sbr_lag=2)]


@pytest.mark.parametrize("name,nl", CASES, ids=[c[0] for c in CASES])
def test_dpp_forms_are_bit_identical(name, nl):
    """Every setting of the switch, for the default, every ring size, both fall-backs of the handshake, the general loop and both
    lags, against the LDS forms."""
    prob, nl = _problem(name, nl)
    E0 = _solve(prob, nl, sbr_xdpp=0)
    for other in RINGS + OTHERS:
        for x in SETTINGS:
            kw = dict(other, sbr_xdpp=x)
            E = _solve(prob, nl, **kw)
            assert np.array_equal(E, E0), (name, kw, np.max(np.abs(E - E0)))
    prob.close()


def test_lds_forms_did_not_move():
    """sbr_xdpp=0 against the general loop with the long lag: the reference of test_gpu_chase8_phased.py"""
    prob, nl = _problem("c3_1024_l31", 12)
    assert np.array_equal(_solve(prob, nl, sbr_xdpp=0), _solve(prob, nl, sbr_phased=0, sbr_lag=1))
    prob.close()


def test_channel_alone_and_inside_a_batch():
    """A channel's spectrum does not depend on the batch it is solved in, in every setting."""
    prob, nl = _problem("c3_1024_l31", 12)
    E0 = _solve(prob, nl, sbr_xdpp=0)
    for x in SETTINGS:
        E1 = _solve(prob, 1, sbr_xdpp=x)
        E5 = _solve(prob, 5, l0=7, sbr_xdpp=x)
        assert np.array_equal(E1, E0[:1]) and np.array_equal(E5, E0[7:12]), x
    prob.close()


@pytest.mark.parametrize("name,nl", [("c3_1024_l31", 12), ("bc10", None)], ids=["c3_1024_l31", "bc10"])
def test_tiles_of_16_do_not_depend_on_the_switch(name, nl):
    """cw_band8=0 hands the chase a band of half-width 15: tiles of 16, which share the template and keep the LDS forms."""
    prob, nl = _problem(name, nl)
    with _Options(cw_band8=0):
        E0 = _solve(prob, nl, sbr_xdpp=0)
        for x in SETTINGS:
            assert np.array_equal(_solve(prob, nl, sbr_xdpp=x), E0), (name, x)
    prob.close()
