"""bisect3_kernel with two logical workgroups per hardware workgroup (option bisect_pair, csrc/tridiag.hip): the paired
launch only changes WHERE and WHEN a block of 1024 eigenvalues is searched, never which points it evaluates, so the spectra must be
the same bit for bit."""
import numpy as np
import pytest

from bspatom_amd import capi

OPTIONS = ("bisect_pair", "bisect_secant", "bisect_tail")


def graded(n, batch):
    """graded random tridiagonal matrices as in test_gpu_stages.py::test_bisect_relative_accuracy_vs_truth: eigenvalues over 14 decades,
    both signs (the ones next to zero run deep into the multisection tail)"""
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


# n = 1025: two logical workgroups, the second holds one eigenvalue; 2500: three, the last one unpaired; 5000: five
CASES = [(1025, 3, {}), (2048, 3, {}), (2500, 3, {}), (4096, 3, {}), (5000, 3, {}),
         (2500, 3, {"bisect_secant": 0}), (2500, 3, {"bisect_tail": 0}),
         (8800, 1, {})]                                   # rows beyond the LDS in global memory: written once, read by both items


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch,extra", CASES, ids=["-".join(["n%d" % c[0], "b%d" % c[1]] + ["%s%d" % kv for kv in c[2].items()]) for c in CASES])
def test_paired_launch_bit_identical(n, batch, extra):
    d, e = graded(n, batch)
    w0 = spectra(d, e, bisect_pair=0, **extra)
    w2 = spectra(d, e, bisect_pair=2, **extra)
    assert np.all(np.isfinite(w0)) and np.all(np.diff(w0, axis=1) >= 0)
    assert np.array_equal(w0, w2)


@pytest.mark.gpu
def test_default_rule_below_the_threshold():
    """bisect_pair = 1 pairs only when there are more workgroups than CUs: 3 x 4 workgroups are launched as with bisect_pair = 0"""
    d, e = graded(4096, 3)
    assert np.array_equal(spectra(d, e, bisect_pair=1), spectra(d, e, bisect_pair=0))
