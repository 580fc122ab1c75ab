"""bisect3_kernel with its logical workgroups handed out from a device queue (option bisect_queue, csrc/tridiag.hip): the
queue only changes WHICH hardware workgroup searches a block of 1024 eigenvalues and WHEN, never which points it evaluates, so the
spectra must equal those of the plain launch (bisect_queue=0, bisect_pair=0) bit for bit -- also when one hardware workgroup runs many
items of several channels (bisect_queue_grid), when the counters have been used before, and when rows live in global memory."""
import numpy as np
import pytest

from bspatom_amd import capi

OPTIONS = ("bisect_queue", "bisect_queue_grid", "bisect_pair", "bisect_secant", "bisect_tail")

_cache = {}


def graded(n, batch):
    """the graded random tridiagonal matrices of test_gpu_bisect_pairs.py: eigenvalues over 14 decades, both signs (the ones next to
    zero run deep into the multisection tail)"""
    rng = np.random.default_rng(n + batch)
    d = np.zeros((batch, n)); e = np.zeros((batch, n - 1))
    for b in range(batch):
        mag = 10.0 ** rng.uniform(-14, 0, n) * (10.0 ** b)
        mag[rng.integers(0, n, 5)] = 1.0 * (10.0 ** b)
        d[b] = mag * rng.choice([-1.0, 1.0], n)
        e[b] = 1e-3 * np.sqrt(np.abs(d[b, :-1] * d[b, 1:])) * rng.choice([-1.0, 1.0], n - 1)
    return d, e


def spectra(d, e, **opts):
    saved = {k: capi.get_option(k) for k in OPTIONS}
    try:
        for k, v in opts.items():
            capi.set_option(k, v)
        return capi.stage_bisect(d, e)
    finally:
        for k, v in saved.items():
            capi.set_option(k, v)


def case(n, batch, **extra):
    """the matrices and the spectra of the plain launch, computed once per (n, batch, options)"""
    key = (n, batch, tuple(sorted(extra.items())))
    if key not in _cache:
        d, e = graded(n, batch)
        w0 = spectra(d, e, bisect_queue=0, bisect_pair=0, **extra)
        assert np.all(np.isfinite(w0)) and np.all(np.diff(w0, axis=1) >= 0)
        w0.setflags(write=False)
        _cache[key] = (d, e, w0)
    return _cache[key]


# n = 1025: the second quarter of a channel holds one eigenvalue; 2500: three items per channel, the last one ragged; 5000: five
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1025, 2500, 4096, 5000])
def test_queue_launch_bit_identical(n):
    d, e, w0 = case(n, 3)
    assert np.array_equal(spectra(d, e, bisect_queue=2), w0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 2, 5])
def test_few_workgroups_run_all_items(grid):
    """nine items of three channels on 1, 2 and 5 hardware workgroups: a workgroup runs several items, redoes the set-up at every change
    of channel, and claims from the head and the tail of the list are interleaved"""
    d, e, w0 = case(2500, 3)
    assert np.array_equal(spectra(d, e, bisect_queue=2, bisect_queue_grid=grid), w0)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [{"bisect_secant": 0}, {"bisect_tail": 0}], ids=["secant0", "tail0"])
def test_queue_launch_without_secant_rounds_or_tail(extra):
    d, e, w0 = case(2500, 3, **extra)
    assert np.array_equal(spectra(d, e, bisect_queue=2, **extra), w0)


@pytest.mark.gpu
def test_rows_in_global_memory_and_a_change_of_channel():
    """n = 8800: the rows beyond the LDS are in global memory; 18 items of two channels on three hardware workgroups"""
    d, e, w0 = case(8800, 2)
    assert np.array_equal(spectra(d, e, bisect_queue=2, bisect_queue_grid=3), w0)


@pytest.mark.gpu
def test_counters_are_reset_between_launches():
    """the same launch twice in a row, then after a launch of another size on the same stream"""
    d, e, w0 = case(2500, 3)
    assert np.array_equal(spectra(d, e, bisect_queue=2), w0)
    assert np.array_equal(spectra(d, e, bisect_queue=2), w0)
    d2, e2, w2 = case(1025, 3)
    assert np.array_equal(spectra(d2, e2, bisect_queue=2, bisect_queue_grid=2), w2)
    assert np.array_equal(spectra(d, e, bisect_queue=2), w0)


@pytest.mark.gpu
def test_default_rule_below_the_threshold():
    """bisect_queue = 1 fires only when there are more logical workgroups than CUs: 3 x 4 of them are launched as today's default"""
    d, e, w0 = case(4096, 3)
    w1 = spectra(d, e, bisect_queue=1)
    assert np.array_equal(w1, spectra(d, e, bisect_queue=0))
    assert np.array_equal(w1, w0)
