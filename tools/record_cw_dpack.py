#!/usr/bin/env python
"""Record tests/golden/cw_dpack_parent.npz (cases: tools/cw_dpack_cases.py) from the library as it is built in this tree.

Run it on the commit whose results are the reference -- the one before the packed diagonal blocks -- on a GPU:
    python tools/record_cw_dpack.py [output.npz]
Per case and recorded variant: the digests of the whole band and of the spectra of the hydrogen problem, and both in full for the
channels that cw_dpack_cases.kept_channels names."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cw_dpack_cases as cs  # noqa: E402
from bspatom_amd import capi  # noqa: E402


def with_options(kw, fn):
    old = {k: capi.get_option(k) for k in kw}
    for k, v in kw.items():
        capi.set_option(k, v)
    try:
        return fn()
    finally:
        for k, v in old.items():
            capi.set_option(k, v)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cw_dpack_parent.npz")
    rec = {}
    for n, k, nl in cs.CASES:
        t = cs.tag(n, k, nl)
        SB, HB = cs.pencil(n, k, nl)
        rec[t + "/inputs_sha"] = cs.digest(np.concatenate([SB.ravel(), HB.ravel()]))
        prob = capi.Problem(capi.make_input(**cs.hydrogen(n, k, nl)))
        assert prob.route() == 2, (t, prob.route())
        for name, kw in cs.RECORDED.items():
            AB, info = with_options(kw, lambda: capi.stage_crawford(SB, HB))
            assert info == 0, (t, name, info)
            A = cs.trimmed(AB, n)
            rec["%s/%s/band_sha" % (t, name)] = cs.digest(A)
            keep, nc = cs.kept_channels(k, nl, name), cs.band_cols(name)
            assert np.all(A[:, :, nc:] == 0.0), (t, name)
            rec["%s/%s/band" % (t, name)] = A[keep][:, :, :nc]
            E, inf = with_options(kw, lambda: prob.solve(0, nl))
            assert np.all(inf == 0), (t, name, inf)
            rec["%s/%s/spectra_sha" % (t, name)] = cs.digest(E)
            rec["%s/%s/spectra" % (t, name)] = E if name == "default" else E[keep]
            print("%s %s: band %s, |band| max %.3e, E[0, 0] = %.15f" % (t, name, A.shape, np.max(np.abs(A)), E[0, 0]))
        prob.close()
    np.savez(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main()
