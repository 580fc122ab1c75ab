#!/usr/bin/env python3
"""resolvent_wide_bits.py -- X, R and info of bspatom_resolvent_coupled_wide on the T1 cases of tests/test_gpu_resolvent_wide.py (the
seven shapes from half-width 11 to 255, nrhs / nproj = (1, 0) and (3, 2), every matrix of the case) into one .npz, and the bitwise
comparison of two such files.  The check by hand that goes with a change that must keep the wide call's bits (the split of
resolvent_wide_kernel into csrc/resolvent_wide_lu.h): dump from a build of the commit before, dump from the new build, compare.

    python tools/resolvent_wide_bits.py dump OUT.npz [--tree DIR]     DIR: the checkout whose bspatom_amd (with its built library) is
                                                                      loaded; default: this one.  Inputs and cases are always this
                                                                      checkout's tests/.
    python tools/resolvent_wide_bits.py compare A.npz B.npz           exit status 0 and "bit-identical" if every array has the same bits
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(out, tree):
    import torch                           # noqa: F401  first: its HIP runtime is the one the process uses
    sys.path.insert(0, os.path.abspath(tree))
    import bspatom_amd
    from bspatom_amd import capi
    assert os.path.dirname(os.path.dirname(os.path.abspath(bspatom_amd.__file__))) == os.path.abspath(tree), bspatom_amd.__file__
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.append(p)
    import test_gpu_resolvent_coupled as coupled
    import test_gpu_resolvent_wide as wide
    arrays = {}
    for name, nch, mats in wide.T1_CASES:
        prob, SB, HB, WB, G = wide._assembled(name)
        n = prob.nfun
        l = [c % 2 for c in range(nch)]
        z = np.array([[zb + 0.01 * c for c in range(nch)] for zb, _, _ in mats])
        w = np.array([[wm] * nch for _, wm, _ in mats], dtype=np.int32)
        a = np.stack([wide._coefficients(nch, s) for _, _, s in mats])
        for nrhs, nproj in ((1, 0), (3, 2)):
            B, P = coupled._vectors(n, nch, nrhs, nproj, 7 + nrhs)
            X, R, info = prob.resolvent_coupled_wide(l, z, B, couplings=wide._topology(nch), G=G, a=a, W=WB, w=w, P=P)
            key = "%s_nch%d_rhs%d" % (name, nch, nrhs)
            arrays[key + "_X"], arrays[key + "_info"] = X, info
            if R is not None:
                arrays[key + "_R"] = R
        prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, library=np.array(capi.lib()._name), **arrays)
    print("wrote %s: %d arrays from %s" % (out, len(arrays), capi.lib()._name))


def compare(fa, fb):
    A, B = np.load(fa), np.load(fb)
    keys = sorted(k for k in A.files if k != "library")
    assert keys == sorted(k for k in B.files if k != "library"), (A.files, B.files)
    print("%s: %s\n%s: %s" % (fa, A["library"], fb, B["library"]))
    bad = 0
    for k in keys:
        x, y = np.ascontiguousarray(A[k]), np.ascontiguousarray(B[k])
        eq = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        bad += not eq
        print("%-28s %-18s %s" % (k, x.shape, "same bits" if eq else "DIFFERS"))
    print("bit-identical: %d arrays" % len(keys) if not bad else "%d of %d arrays differ" % (bad, len(keys)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--tree", default=ROOT)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(dump(args.out, args.tree) if args.cmd == "dump" else compare(args.a, args.b))


if __name__ == "__main__":
    main()
