"""The twelve bspatom_tdse_* entry points without a GPU: what each returns for bad arguments, in which order the checks come, and
the call of no steps without rows.  Every case returns before the handle is read: a block of zeros stands in for it.  The expected
codes are those of include/bspatom.h."""
import ctypes as C
import numpy as np
import pytest

from bspatom_amd import capi

OK, ARG, UNSUPPORTED = 0, -2, -5
MAX_FIELDS, MAX_LEVEL = 3, 16                                  # BSPATOM_TDSE_MAX_FIELDS, BSPATOM_TDSE_MAX_LEVEL
nch, count, nscan, nsteps = 3, 4, 2, 2

# name -> the number of arguments: 16 common, + obs_every, obs, + scheme and the static lists, + nfield, fidx / + the controller's nine
ENTRIES = {"bspatom_tdse_propagate": 16, "bspatom_tdse_observe": 18, "bspatom_tdse_lawson": 18, "bspatom_tdse_static": 24,
           "bspatom_tdse_fields": 26, "bspatom_tdse_adaptive": 33}
ENTRIES.update({k + "_dev": v for k, v in list(ENTRIES.items())})
STATIC = sorted(k for k, v in ENTRIES.items() if v >= 24)
FIELDS = sorted(k for k, v in ENTRIES.items() if v == 26)
ADAPTIVE = sorted(k for k, v in ENTRIES.items() if v == 33)

p_ = lambda x: x.ctypes.data_as(C.c_void_p)
i32 = lambda *v: np.array(v, dtype=np.int32)
handle = C.create_string_buffer(1 << 16)
E, D = np.zeros((nch, count)), np.zeros((2, count, count))
ci, cf = i32(0, 1), i32(1, 2)
field, a = np.zeros((nsteps, 6, 2, nscan), dtype=np.complex128), np.zeros((nscan, nch, count), dtype=np.complex128)
snap, err, obs = np.zeros((2, nscan, nch, count), dtype=np.complex128), np.zeros(nscan), np.zeros((3, nscan, nch, 8))
si, sf, sk, W = i32(0, 2), i32(0, 1), i32(1, 0), np.zeros((2, count, count))
fidx = i32(0, 1)
stats, log_i = np.zeros(6, dtype=np.int64), np.zeros((4, 4), dtype=np.int32)
log_e, log_f = np.zeros((4, nscan)), np.zeros((4, 6, nscan), dtype=np.complex128)


def good(name):
    """arguments that pass every check of the entry point (never passed on as they are: that call would go to the GPU)"""
    g = [C.addressof(handle), nch, count, p_(E), 2, p_(ci), p_(cf), p_(D), nscan, nsteps, 0.05, p_(field), p_(a), 1, p_(snap), p_(err),
         1, p_(obs), 1, 2, p_(si), p_(sf), p_(sk), p_(W)]
    if name in FIELDS:
        g += [2, p_(fidx)]
    if name in ADAPTIVE:
        g += [2, 1e-6, 4, 1, p_(stats), 4, p_(log_i), p_(log_e), p_(log_f)]    # nsub, tol, max_level, level0, stats, log_cap, logs
    return g[:ENTRIES[name]] if ENTRIES[name] < 24 else g


def call(name, *subs):
    """the entry point on its good arguments with (position, value) pairs put in"""
    args = good(name)
    for pos, v in subs:
        args[pos] = v
    assert len(args) == len(getattr(capi.lib(), name).argtypes) == ENTRIES[name]
    return getattr(capi.lib(), name)(*args)


def test_all_twelve_are_here():
    assert sorted(ENTRIES) == sorted(n for n in capi.EXPORTS if n.startswith("bspatom_tdse_")) and len(ENTRIES) == 12


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_common_argument_checks(name):
    for pos in (0, 3, 5, 6, 7, 11, 12):                            # p, E, ci, cf, D, field, a
        assert call(name, (pos, None)) == ARG, pos
    for pos in (1, 2, 8):                                          # nch, count, nscan < 1
        assert call(name, (pos, 0)) == ARG and call(name, (pos, -1)) == ARG, pos
    for pos in (9, 4, 13):                                         # nsteps, npairs, snap_every < 0
        assert call(name, (pos, -1)) == ARG, pos
    assert call(name, (13, 0)) == ARG                              # snap given with snap_every = 0
    for bad in (i32(0, 3), i32(-1, 1)):
        assert call(name, (5, p_(bad))) == ARG and call(name, (6, p_(bad))) == ARG
    assert call(name, (5, p_(cf))) == ARG                          # ci == cf
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(name, (10, bad)) == ARG
    if ENTRIES[name] >= 18:
        assert call(name, (16, -1)) == ARG                         # obs_every < 0
        assert call(name, (16, 0)) == ARG                          # obs given with obs_every = 0
        assert call(name, (17, None)) == ARG                       # obs_every >= 1 without obs


@pytest.mark.parametrize("name", STATIC)
def test_static_argument_checks(name):
    for bad in (-1, 2):                                            # scheme outside {0, 1}
        assert call(name, (18, bad)) == ARG
    assert call(name, (19, -1)) == ARG                             # nstat < 0
    for pos in (20, 21, 22, 23):                                   # nstat > 0 without si, sf, skind, W
        assert call(name, (pos, None)) == ARG, pos
    for bad in (i32(0, 3), i32(-1, 1)):
        assert call(name, (20, p_(bad))) == ARG and call(name, (21, p_(bad))) == ARG
    for bad in (i32(1, 2), i32(-1, 0)):
        assert call(name, (22, p_(bad))) == ARG                    # skind outside {0, 1}


@pytest.mark.parametrize("name", FIELDS)
def test_fields_checks_and_their_order(name):
    for bad in (0, -1):
        assert call(name, (24, bad)) == ARG                        # nfield < 1
    assert call(name, (24, 2), (25, None)) == ARG                  # several fields, pairs, no fidx
    for bad in (i32(0, 2), i32(-1, 1)):
        assert call(name, (25, p_(bad))) == ARG                    # an entry outside 0 .. nfield-1
    # too many fields: UNSUPPORTED before fidx is looked at, but behind every ARG check of the arguments in front
    for fx in (p_(fidx), None, p_(i32(0, 7)), p_(i32(-1, 0))):
        assert call(name, (24, MAX_FIELDS + 1), (25, fx)) == UNSUPPORTED
    assert call(name, (24, MAX_FIELDS + 1), (1, 0)) == ARG
    assert call(name, (24, MAX_FIELDS + 1), (17, None)) == ARG
    assert call(name, (24, MAX_FIELDS + 1), (18, 2)) == ARG
    assert call(name, (24, MAX_FIELDS + 1), (22, p_(i32(1, 2)))) == ARG


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_checks_and_their_order(name):
    for bad in (0.0, -1.0, float("nan")):
        assert call(name, (25, bad)) == ARG                        # tol not positive
    assert call(name, (26, -1), (27, -1)) == ARG                   # max_level < 0
    assert call(name, (27, -1)) == ARG and call(name, (27, 5)) == ARG          # level0 outside 0 .. max_level
    assert call(name, (24, 0)) == ARG                              # nsub < 1
    assert call(name, (28, None)) == ARG                           # stats
    assert call(name, (29, -1)) == ARG                             # log_cap < 0
    for pos in (30, 31, 32):                                       # log_cap > 0 without a log array
        assert call(name, (pos, None)) == ARG, pos
    # a legal max_level above the limit: UNSUPPORTED, behind every ARG clause
    assert call(name, (26, MAX_LEVEL + 1)) == UNSUPPORTED
    assert call(name, (26, MAX_LEVEL + 1), (27, MAX_LEVEL + 1)) == UNSUPPORTED
    assert call(name, (26, MAX_LEVEL + 1), (27, MAX_LEVEL + 2)) == ARG
    assert call(name, (26, MAX_LEVEL + 1), (25, 0.0)) == ARG
    assert call(name, (26, MAX_LEVEL + 1), (28, None)) == ARG
    assert call(name, (26, MAX_LEVEL + 1), (31, None)) == ARG
    assert call(name, (26, MAX_LEVEL + 1), (11, None)) == ARG      # fn with nsteps > 0
    assert call(name, (26, MAX_LEVEL + 1), (2, 0)) == ARG
    assert call(name, (26, MAX_LEVEL + 1), (19, -1)) == ARG


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_no_steps_and_no_rows_is_done_at_once(name):
    """nsteps = 0 without observing: BSP_OK with err zeroed before the handle is read; no field is needed"""
    subs = [(9, 0), (11, None)]
    if ENTRIES[name] >= 18:
        subs += [(16, 0), (17, None)]
    err[:] = 7.0
    stats[:] = -1
    assert call(name, *subs) == OK
    assert np.array_equal(err, np.zeros(nscan))
    if name in ADAPTIVE:
        assert tuple(stats) == (0, 0, 0, 0, 1, 0)                  # level0 = 1 in its place
        stats[:] = -1
        assert call(name, *subs, (27, 3)) == OK and tuple(stats) == (0, 0, 0, 0, 3, 0)
    assert call(name, *subs, (15, None)) == OK                     # err may be null
