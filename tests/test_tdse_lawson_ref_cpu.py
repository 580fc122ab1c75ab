"""tests/tdse_lawson_ref.py, the NumPy restatement of bspatom_tdse_lawson, pinned on the CPU: exact free evolution, agreement with the
plain restatement where both are stable, order and error estimate on the closed-form 2 x 2 problem, and the stiff system on which
the plain scheme diverges.  The figures in the docstrings were measured with this file."""
import warnings

import numpy as np

import tdse_lawson_ref
import tdse_ref

EPS = tdse_ref.EPS
DT = 0.05


def test_free_evolution_is_exact():
    """system(1, 20, 1, 40): max|a - a0 exp(-i E t)| 7.2e-16, against 5.3e-9 for the plain restatement"""
    E, pairs, D, a0, field = tdse_ref.system(1, 20, 1, 40, dt=DT)
    a, err = tdse_lawson_ref.propagate(E, pairs, D, a0, field, DT)
    exact = a0 * np.exp(-1j * E[None] * (40 * DT))
    assert float(np.max(np.abs(a - exact))) <= 64.0 * EPS
    assert np.all(err == 0.0)
    plain, _ = tdse_ref.propagate(E, pairs, D, a0, field, DT)
    assert float(np.max(np.abs(plain - exact))) > 1e3 * EPS


def test_against_the_plain_restatement():
    """differences 2.8e-9, 2.6e-9, 3.0e-9: both schemes are 5th-order approximations of the same solution"""
    for shape in ((3, 17, 2, 40), (4, 65, 3, 60), (2, 1, 1, 100)):
        s = tdse_ref.system(*shape, dt=DT)
        a, _ = tdse_lawson_ref.propagate(*s, DT)
        plain, _ = tdse_ref.propagate(*s, DT)
        d = float(np.max(np.abs(a - plain)))
        assert 0.0 < d <= 1e-7, (shape, d)


def test_order_and_error_estimate():
    """two_by_two: error ratio 31.3 from 50 to 100 steps, err / true error 0.70"""
    errs = []
    for nsteps in (50, 100):
        E, pairs, D, a0, field, dt, exact = tdse_ref.two_by_two(nsteps)
        a, est = tdse_lawson_ref.propagate(E, pairs, D, a0, field, dt)
        true = float(np.max(np.abs(a - exact)))
        assert 0.5 * true <= est[0] <= 2.0 * true, (nsteps, true, est[0])
        errs.append(true)
    assert 24.0 <= errs[0] / errs[1] <= 40.0, errs


def test_stiff_system():
    """dt max|E| = 20: the plain complex128 restatement reaches 6.5e191, the Lawson restatement keeps its norm to 4.8e-4 and its
    complex128 run lies 6.5e-16 from its long-double run"""
    s = tdse_lawson_ref.stiff_system()
    assert abs(DT * float(np.max(np.abs(s[0]))) - 20.0) < 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with np.errstate(all="ignore"):
            plain, _ = tdse_ref.propagate(*s, DT)
    big = np.abs(plain)
    assert not np.all(np.isfinite(big)) or float(np.max(big)) > 1e3
    (a, err), (along, errlong) = tdse_lawson_ref.both(*s, DT)
    drift = np.abs(np.sum(np.abs(a) ** 2, axis=(1, 2)) - 1.0)
    assert float(np.max(drift)) <= 5e-3
    assert float(np.max(np.abs(a.astype(np.clongdouble) - along))) <= 1e-13
    assert np.all(np.isfinite(err)) and float(np.max(err)) > 0.0
