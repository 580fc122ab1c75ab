"""The band route's chase on tiles of 8 (csrc/sbr2.hip::sbr_rows_kernel<8>) with the step loop of its chasing waves in three parts
(option sbr_phased, the default) and with the short lag of its data-moving wave (option sbr_lag): both only change WHEN something
is done, so every spectrum must equal, bit for bit, the one the general loop with the long lag gives (sbr_phased=0, sbr_lag=1)."""
import numpy as np
import pytest
from test_gpu_stages import input_from_case
from test_gpu_solve import _Options

pytestmark = pytest.mark.gpu
from bspatom_amd import capi

# n128: 61 steps in the longest pass, the steady part is never entered (ramp-up meets ramp-down); lin256: a steady part without a
# wrap; bc10, ka_ra, c1_lin: sizes that are not multiples of 8; c3_1024_l31, 12 channels: n > 512, tiles wrap around the ring of
# window columns, and the rings of workgroups are real (63 passes)
CASES = [("n128", None), ("lin256", None), ("bc10", None), ("ka_ra", None), ("c1_lin", None), ("c3_1024_l31", 12)]
OLD = dict(sbr_phased=0, sbr_lag=1)
RINGS = [dict(), dict(sb2st_ring=1), dict(sb2st_ring=2), dict(sb2st_ring=4), dict(sb2st_ring=8), dict(sb2st_force_abort=1),
         dict(sb2st_force_abort=2)]


def _problem(name, nl):
    prob = capi.Problem(input_from_case(name))
    assert prob.route() == 2
    return prob, (prob.lmax + 1 if nl is None else nl)


def _solve(prob, nl, l0=0, **kw):
    with _Options(**kw):
        E, info = prob.solve(l0, nl)
    assert np.all(info == 0), kw
    return E


@pytest.mark.parametrize("name,nl", CASES, ids=[c[0] for c in CASES])
def test_phased_loop_and_lags_are_bit_identical(name, nl):
    """The default (phased loop, lag by pass), and the phased loop with the lag forced long and forced short, for every ring size and
    both fall-backs of the handshake, against the general loop with the long lag."""
    prob, nl = _problem(name, nl)
    E0 = _solve(prob, nl, **OLD)
    for ring in RINGS:
        for lag in (0, 1, 2):
            kw = dict(ring, sbr_phased=1, sbr_lag=lag)
            E = _solve(prob, nl, **kw)
            assert np.array_equal(E, E0), (name, kw, np.max(np.abs(E - E0)))
        # the general loop with the short lag: the two levers apart
        kw = dict(ring, sbr_phased=0, sbr_lag=2)
        E = _solve(prob, nl, **kw)
        assert np.array_equal(E, E0), (name, kw, np.max(np.abs(E - E0)))
    prob.close()


@pytest.mark.parametrize("name,nl", [("c3_1024_l31", 12), ("bc10", None)], ids=["c3_1024_l31", "bc10"])
def test_tiles_of_16_do_not_depend_on_the_switches(name, nl):
    """cw_band8=0 hands the chase a band of half-width 15: tiles of 16, which share the template."""
    prob, nl = _problem(name, nl)
    with _Options(cw_band8=0):
        E0 = _solve(prob, nl, **OLD)
        for kw in (dict(), dict(sbr_lag=2), dict(sb2st_ring=4), dict(sb2st_ring=1, sbr_lag=2), dict(sb2st_force_abort=1)):
            E = _solve(prob, nl, **kw)
            assert np.array_equal(E, E0), (name, kw)
    prob.close()


def test_channel_alone_and_inside_a_batch():
    """A channel's spectrum does not depend on the batch it is solved in (the ring size, and with it the lag of a pass, does)."""
    prob, nl = _problem("c3_1024_l31", 12)
    E0 = _solve(prob, nl, **OLD)
    E = _solve(prob, nl)
    E1 = _solve(prob, 1)
    E5 = _solve(prob, 5, l0=7)
    assert np.array_equal(E, E0) and np.array_equal(E1, E0[:1]) and np.array_equal(E5, E0[7:12])
    prob.close()
