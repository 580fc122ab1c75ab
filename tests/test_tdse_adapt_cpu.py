"""The restatement of bspatom_tdse_adaptive (tests/tdse_adapt_ref.py) and the host helpers host.field_nodes / host.adapt_steps, without
a GPU: the controller against a trace written by hand, the Hermite evaluation against a cubic, the time arithmetic, and the test
system of tests/test_gpu_tdse_adapt.py, which must show what those tests rely on, on the long-double restatement."""
import functools
import numpy as np
import pytest

import tdse_adapt_ref as R
from bspatom_amd import host

EPS = float(np.finfo(np.float64).eps)


def test_controller_follows_the_hand_written_trace():
    """tol = 1, max_level = 2, two coarse steps from level 0; the estimates by attempt, the states worked out by hand:
        (0,0,0) e=5    rejected                  -> (0,1,0)
        (0,1,0) e=0.5  accepted, j=1 odd         -> (0,1,1)
        (0,1,1) e=3    rejected                  -> (0,2,2)
        (0,2,2) e=7    forced (m = max_level)    -> (0,2,3)
        (0,2,3) e=0.01 accepted, j=4 even, small -> coarsened (0,1,2) = wrap -> (1,1,0)
        (1,1,0) e=0.01 accepted, j=1 odd: no coarsening          -> (1,1,1)
        (1,1,1) e=1/64 accepted, j=2 even, e <= tol/64 exactly   -> coarsened (1,0,1) = wrap -> (2,0,0)"""
    es = iter([5.0, 0.5, 3.0, 7.0, 0.01, 0.01, 0.015625])
    log = R.controller(2, 1.0, 2, 0, lambda n, m, j: next(es))
    assert [r[:4] for r in log] == [(0, 0, 0, 0), (0, 1, 0, 1), (0, 1, 1, 0), (0, 2, 2, 2), (0, 2, 3, 1), (1, 1, 0, 1), (1, 1, 1, 1)]
    assert R.stats_of(log, 1.0) == [5, 2, 1, 2, 0, 7]
    assert R.features(log) == (2, 1, 3, 1)                      # the coarsening behind the last attempt has no attempt to show it
    # just above tol / 64: no coarsening; a NaN is rejected above max_level and forced at it; tol = inf never rejects
    assert R.advance(1, 2, 1, 1, np.nextafter(0.015625, 1.0), 1.0) == (1, 2, 2)
    assert R.advance(1, 2, 1, 1, 0.015625, 1.0) == (1, 1, 1)
    assert R.decide(np.nan, 1.0, 0, 2) == 0 and R.decide(np.nan, 1.0, 2, 2) == 2
    assert R.decide(np.inf, np.inf, 0, 2) == 1 and R.decide(1e300, np.inf, 0, 2) == 1
    li = np.array([r[:4] for r in log])
    le = np.array([[r[4], 0.0] for r in log])
    assert R.follows_rule(li, le, 1.0, 2, 0, nsteps=2) == (2, 0, 0)
    bad = li.copy()
    bad[3, 3] = 0
    with pytest.raises(AssertionError):
        R.follows_rule(bad, le, 1.0, 2, 0)


def test_every_level_sequence_terminates_within_the_bound():
    """2^(L+1) + L attempts per coarse step at most, for a controller driven by pseudo-random estimates"""
    rng = np.random.default_rng(5)
    for L in range(5):
        for level0 in range(L + 1):
            log = R.controller(6, 1.0, L, level0, lambda n, m, j: float(rng.choice([1e-3, 0.5, 2.0, 50.0])))
            per = np.bincount([r[0] for r in log], minlength=6)
            assert per.max() <= 2 ** (L + 1) + L, (L, level0, per)
            # the accepted steps tile every coarse step exactly
            cover = np.zeros(6)
            for n, m, j, flag, e in log:
                if flag:
                    cover[n] += 2.0 ** -m
            assert np.all(cover == 1.0)


def test_hermite_reproduces_a_cubic():
    """A cubic polynomial (complex coefficients) and its derivative on the nodes: the interpolant is the polynomial, to rounding"""
    dt, nsub, nsteps = 0.4, 3, 2
    co = np.array([0.3 - 0.2j, -1.1 + 0.4j, 0.7 + 0.9j, -0.25 - 0.6j])
    p = lambda t: ((co[3] * t + co[2]) * t + co[1]) * t + co[0]
    dp = lambda t: (3 * co[3] * t + 2 * co[2]) * t + co[1]
    fn = host.field_nodes([p, lambda t: 2 * p(t)], [dp, lambda t: 2 * dp(t)], 0.0, dt, nsteps, nsub)
    assert fn.shape == (nsteps * nsub + 1, 2, 2)
    scale = float(np.sum(np.abs(co)))
    for n in range(nsteps):
        for m, j in ((0, 0), (1, 1), (3, 5), (4, 15)):
            f = R.attempt_field(fn, dt, nsub, n, m, j)
            t = R.stage_times(0.0, dt, n, m, j)
            assert f.shape == (6, 2)
            assert np.max(np.abs(f[:, 0] - p(t))) <= 32 * EPS * scale and np.max(np.abs(f[:, 1] - 2 * p(t))) <= 64 * EPS * scale
    # at a node the interpolant is the node value exactly (u = 0: h00 = 1, the rest 0), at x = 1 the next node (u = 1 in the last interval)
    f = R.hermite(fn, dt, nsub, 1, np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0, 0.5, 0.25]))
    assert np.array_equal(f[0], fn[3, 0]) and np.array_equal(f[3], fn[6, 0])


def test_time_arithmetic():
    """x_s = ldexp(j + c_s, -m); at level 0 the stage times are host.rk_nodes' (the same doubles c_s); the step ends are exact dyadics"""
    c = R.C64
    assert np.array_equal(R.stage_x(0, 0), c) and np.array_equal(R.stage_x(3, 5), (5.0 + c) / 8.0)
    assert R.stage_x(4, 15)[4] == 1.0 and R.stage_x(16, 0)[1] == np.ldexp(c[1], -16)
    assert np.array_equal(R.stage_times(0.0, 0.05, 7, 0, 0), host.rk_nodes(0.0, 0.05, 8)[7])
    t = R.stage_times(1.0, 0.5, 2, 2, 3)
    assert t[0] == 1.0 + 0.5 * 2.75 and t[4] == 1.0 + 0.5 * 3.0


def test_field_nodes_and_adapt_steps():
    f, df = R.pulse(2.0, 0.3)
    fn = host.field_nodes([f], [df], R.T0, R.DT, R.NSTEPS, R.NSUB)
    assert np.array_equal(fn, R.node_table([2.0], 0.3))
    # without derivatives: centred differences at +- hf / 8
    hf = R.DT / R.NSUB
    t = R.T0 + np.arange(R.NSTEPS * R.NSUB + 1) * hf
    fd = host.field_nodes([f], None, R.T0, R.DT, R.NSTEPS, R.NSUB)
    assert np.array_equal(fd[:, 0], fn[:, 0])
    assert np.array_equal(fd[:, 1, 0], (f(t + hf / 8) - f(t - hf / 8)) / (2 * (hf / 8)))
    assert np.max(np.abs(fd[:, 1] - fn[:, 1])) < 1e-2 * np.max(np.abs(fn[:, 1]))
    assert host.field_nodes([], None, 0.0, 0.1, 0, 1).shape == (1, 2, 0)
    with pytest.raises(ValueError):
        host.field_nodes([f], [df, df], 0.0, 0.1, 2, 1)
    with pytest.raises(ValueError):
        host.field_nodes([f], None, 0.0, 0.1, 2, 0)
    log_i = [[0, 1, 0, 1], [0, 1, 1, 0], [0, 2, 2, 2], [0, 2, 3, 1], [1, 1, 0, 1]]
    ts, hs = host.adapt_steps(log_i, 1.0, 0.5)
    assert np.array_equal(ts, [1.0, 1.25, 1.375, 1.5]) and np.array_equal(hs, [0.25, 0.125, 0.125, 0.25])
    assert np.array_equal(ts[1:], (ts + hs)[:-1])
    e0, h0 = host.adapt_steps(np.zeros((0, 4), dtype=np.int32), 0.0, 0.1)
    assert e0.shape == (0,) and h0.shape == (0,)


@functools.lru_cache(maxsize=None)
def long_run(key, scheme, max_level):
    E, pairs, D, a0, fn, static = R.adapt_system(*key)
    return R.run(E, pairs, D, a0, fn, R.DT, R.NSUB, static, scheme, R.TOL, max_level, R.LEVEL0, np.longdouble, np.clongdouble)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", R.SHAPES)
def test_the_test_system_shows_what_the_gpu_tests_rely_on(key, scheme):
    a, err, log = long_run(key, scheme, R.MAX_LEVEL_TEST)
    rej, coarsen, levels, forced = R.features(log)
    assert rej >= 1 and coarsen >= 1 and levels >= 3, (rej, coarsen, levels)
    assert R.margins(log) >= 1e-3, R.margins(log)
    a2, err2, log2 = long_run(key, scheme, R.MAX_LEVEL_FORCED)
    assert R.features(log2)[3] >= 1 and R.margins(log2) >= 1e-3, (R.features(log2), R.margins(log2))
    # the restated rule reads its own log the same way
    li = np.array([r[:4] for r in log])
    le = np.array([[float(r[4])] for r in log])
    assert R.follows_rule(li, le, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, nsteps=R.NSTEPS)[1] == R.stats_of(log, R.TOL)[4]
    # complex128 along the long-double sequence decides the same (the margin)
    a128, err128, log128 = R.run(*R.adapt_system(*key)[:5], R.DT, R.NSUB, R.adapt_system(*key)[5], scheme, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0)
    assert [r[:4] for r in log128] == [r[:4] for r in log]


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", R.SHAPES)
def test_accuracy_of_the_idea(key, scheme):
    """max |a_adaptive - a_fine| <= accepted * tol, a_fine the fixed-step long-double run at level max_level + 2: the sum of the local
    estimates, for a system whose norm does not grow (absorbers only remove norm)."""
    E, pairs, D, a0, fn, static = R.adapt_system(*key)
    a, err, log = long_run(key, scheme, R.MAX_LEVEL_TEST)
    fine = R.fixed_run(E, pairs, D, a0, fn, R.DT, R.NSUB, static, scheme, R.MAX_LEVEL_TEST + 2)
    assert len(fine[2]) == R.NSTEPS * 2 ** (R.MAX_LEVEL_TEST + 2) and all(r[3] == 1 for r in fine[2])
    accepted = sum(1 for r in log if r[3] > 0)
    d = float(np.max(np.abs(a - fine[0])))
    print("adaptive against fine %s scheme %d: %.3g, bound %.3g (%d accepted)" % (key, scheme, d, accepted * R.TOL, accepted))
    assert d <= accepted * R.TOL, (d, accepted * R.TOL)


def test_an_odd_nsub_tells_a_fused_coordinate_from_the_documented_one():
    """With nsub a power of two x_s nsub is exact and u = fma(x_s, nsub, -i_loc) equals the documented rn(rn(x_s nsub) - i_loc); with
    nsub = 3 and 5 they differ at stage positions the test runs visit (level0 = 1: the attempt (0, 1, 0) is always made), so the GPU
    comparison of log_f at these nsub fails on a contracted coordinate."""
    for nsub in (1, 2, 4, 8):
        for m, j in ((0, 0), (1, 0), (1, 1), (3, 5)):
            assert np.array_equal(R.fused_u(nsub, m, j), R.plain_u(nsub, m, j))
    for nsub in (3, 5):
        assert not np.array_equal(R.fused_u(nsub, R.LEVEL0, 0), R.plain_u(nsub, R.LEVEL0, 0)), nsub
        # and the difference reaches the field: a table whose values make every weight count
        fn = R.node_table([R.AMP], 0.3, nsub)
        f = R.attempt_field(fn, R.DT, nsub, 1, R.LEVEL0, 0)
        assert f.shape == (6, 1) and np.all(np.isfinite(f))
