"""The cases of tests/golden/cw_dpack_parent.npz: what tools/record_cw_dpack.py records and tests/test_gpu_cw_dpack.py compares.

The fixture holds the outputs of the band reduction (csrc/crawford.hip) as the commit BEFORE the packed diagonal blocks computed
them: the band of random pencils through bspatom_stage_crawford, and the spectra of hydrogen problems of the same sizes through
the whole band route.  A storage layout changes no arithmetic, so every figure is compared with np.array_equal.

Shapes: the smallest at which the layout can go wrong."""
import hashlib

import numpy as np

# (n, k, channels): why
CASES = [
    (32, 9, 1),     # four blocks: the smallest pencil with a chase item, windows at p = 0 only
    (32, 9, 12),
    (44, 9, 3),     # ragged last block
    (128, 9, 5),    # waves with four items, eliminations and chase items in one wave
    (128, 5, 5),    # narrower pencils
    (128, 3, 5),
    (256, 9, 33),   # two stream groups (16 + 17 channels)
]

# switches whose band is recorded on its own: another arithmetic (one division per reflector) or another hand-over (half-width 15)
RECORDED = {"default": {}, "onediv": {"cw_onediv": 1}, "band8_0": {"cw_band8": 0}}
# switches that change no bit of the default's band: (name, options)
SAME_BITS = [("bcast0", {"cw_bcast": 0}), ("nw4", {"cw_nw": 4}), ("ipw1", {"cw_ipw": 1}), ("ipw2", {"cw_ipw": 2})]

COLS = 16           # columns of the band that can hold anything: nothing is stored beyond half-width 15


def band_cols(variant):
    """columns of the band the fixture holds: half-width 8, or 15 where the block tridiagonal is handed over as it stands"""
    return COLS if variant == "band8_0" else 9


def tag(n, k, nl):
    return "n%d_k%d_c%d" % (n, k, nl)


def pencil(n, k, nl):
    """upper bands of a random banded pencil: S diagonally dominant (positive definite), H symmetric and graded like the centrifugal term"""
    rng = np.random.default_rng(1000 * n + 10 * k + nl)
    SB = np.zeros((k, n)); HB = np.zeros((nl, k, n))
    SB[0] = 2.0 * k + rng.random(n)
    grade = np.exp(-4.0 * np.arange(n) / n)
    for d in range(1, k):
        SB[d, :n - d] = rng.standard_normal(n - d)
    for l in range(nl):
        for d in range(k):
            HB[l, d, :n - d] = rng.standard_normal(n - d) * np.sqrt(grade[:n - d] * grade[d:]) * (1 + l)
    return SB, HB


def hydrogen(n, k, nl):
    """keywords of capi.make_input: hydrogen on a linear grid, n functions of order k, l = 0 .. nl - 1"""
    return dict(kind_grid=0, ra=0.0, rb=40.0, k=k, nfun=n, l_fin=nl - 1, n0_ini=1, l_ini=0, zatom=1.0)


def digest(a):
    """SHA-256 of an array's bytes (as uint8, for an .npz): equal digests are equal bits"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8).copy()


def trimmed(AB, n):
    """the part of a band array (nl, npad, 128) that can hold anything: rows of the matrix, columns up to half-width 15"""
    assert np.all(AB[:, :, COLS:] == 0.0) and np.all(AB[:, n:, :] == 0.0)
    return np.ascontiguousarray(AB[:, :n, :COLS])


def kept_channels(k, nl, variant):
    """channels whose band the fixture holds in full, to say WHERE two results differ (the digests cover every channel): all of a
    small default case at k = 9, the first and last at narrower k, the ends of the two stream groups of a large batch, the last one
    of a variant.  The spectra of a variant are kept for the same channels, the default's for all."""
    if variant != "default":
        return [nl - 1]
    if nl > 12:
        h = nl // 2
        return [0, h - 1, h, h + 1, nl - 1]
    return list(range(nl)) if k == 9 else sorted({0, nl - 1})
