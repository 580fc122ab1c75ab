#!/usr/bin/env python3
"""resolvent_chain_rate.py -- the rate of bspatom_resolvent_chain_dev (csrc/resolvent.hip: resolvent_chain_kernel) in one process on
one GPU, against the same factorisations and solves without the coupling and against the only route there was for a product of two
resolvents.  Workload (tools/resolvent_rate.py's, one order higher): hydrogen, linear grid, k = 9, nfun = 1024 and 4096; 256 chains
b^T G_0(E_1s + 2 omega) r G_1(E_1s + omega) b, omega in [0.55, 1.5], b = r |1s>, the absorber cap_profile(r, 0.75 rb, 1e-3) on both
stages; one right-hand side, one projection, R only.

  (a) Problem.resolvent_chain_dev: 256 chains of 2 stages in ONE call;
  (b) two Problem.resolvent_dev calls, on the 256 stage-0 and the 256 stage-1 matrices, both with the shared right-hand side b: the
      same 512 factorisations and solves without the band apply and without the chain's serial order -- a lower bound that existed
      before the chains (it does not compute the product);
  (c) the route there was: Problem.resolvent on the stage-0 matrices with X returned to the host, host.band_apply in NumPy, then 256
      Problem.resolvent calls with nmat = 1, each with its own right-hand side.  Whether its R equals (a)'s bit for bit is reported, with the largest relative difference
      (C5 of bspatom.h states it for the header's band arithmetic; NumPy's real-times-complex product can differ in a zero's sign).

One untimed run of each, then REPS repetitions of (a), (b), (c) alternating.  Every time is wall time between synchronised points.
The ratios are the medians'; the bracket beside a ratio is the range of the per-repetition ratios (repetition i of one over
repetition i of the other), the spread the ratio is to be read against.
Writes a text report (default profiles/r19_resolvent_chain.txt) and prints one JSON line.

Measured on one MI355X (profiles/r19_resolvent_chain.txt), medians of five: nfun = 1024: (a) 4.80 ms, (b) 4.95 ms ((max - min) / median
0.7 %), (c) 594 ms; (a)/(b) = 0.969 [0.965 .. 1.016], (c)/(a) = 124.  nfun = 4096: (a) 18.05 ms, (b) 18.18 ms (3.0 %), (c) 2285 ms; (a)/(b) =
0.993 [0.981 .. 1.000], (c)/(a) = 127.  (c)'s R equalled (a)'s bit for bit at both sizes.  (DESIGN.md 4.7 reads the ratios.)

    timeout -k 10 600 python tools/resolvent_chain_rate.py [--out FILE] [--sizes 1024,4096]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                               # first: its HIP runtime is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspatom_amd import capi, host          # noqa: E402

NCHAIN, K, REPS = 256, 9, 5


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_resolvent_chain.txt"))
    ap.add_argument("--sizes", default="1024,4096")
    args = ap.parse_args()
    dev = "cuda:0"
    out = {"workload": "%d chains of 2 stages (l = 1, then l = 0), k = %d, absorber on, nrhs = 1, nproj = 1, R only" % (NCHAIN, K)}
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        rb = 0.25 * n
        prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=1, n0_ini=1, l_ini=0, zatom=1.0))
        E, info = prob.solve(0, 2)
        assert np.all(info == 0)
        RB = prob.dipole_bands()
        b = host.band_apply(RB[0], prob.eigvecs(0, 1, 1))[0].astype(np.complex128)
        WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
        om = np.linspace(0.55, 1.5, NCHAIN)
        z = np.stack([E[0, 0] + om, E[0, 0] + 2.0 * om], axis=1).astype(np.complex128)
        l = np.broadcast_to(np.array([1, 0], dtype=np.int32), (NCHAIN, 2))
        G, a = np.ascontiguousarray(RB[:1]), np.ones((NCHAIN, 1, 1))
        bd, Wd, Gd = torch.from_numpy(b).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(G).to(dev)
        Rd = torch.zeros((NCHAIN, 2, 1, 1), dtype=torch.complex128, device=dev)
        Rb = torch.zeros((2, NCHAIN, 1, 1), dtype=torch.complex128, device=dev)
        z0, z1 = np.ascontiguousarray(z[:, 0]), np.ascontiguousarray(z[:, 1])
        l0, l1 = np.ones(NCHAIN, dtype=np.int32), np.zeros(NCHAIN, dtype=np.int32)

        def run_a():
            return prob.resolvent_chain_dev(l, z, 1, bd.data_ptr(), nop=1, G_ptr=Gd.data_ptr(), a=a, nabs=1, W_ptr=Wd.data_ptr(), nproj=1,
                                            P_ptr=bd.data_ptr(), R_ptr=Rd.data_ptr())

        def run_b():
            i0 = prob.resolvent_dev(l0, z0, 1, bd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=bd.data_ptr(), R_ptr=Rb[0].data_ptr())
            i1 = prob.resolvent_dev(l1, z1, 1, bd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=bd.data_ptr(), R_ptr=Rb[1].data_ptr())
            return i0, i1

        def run_c():
            X0, _, _ = prob.resolvent(l0, z0, b, W=WB)
            Y = host.band_apply(RB[0], X0[:, 0])
            return np.array([prob.resolvent(0, z1[c], Y[c], W=WB, P=b, want_x=False)[1][0, 0, 0] for c in range(NCHAIN)])

        assert np.all(run_a() == 0)                                    # untimed: first launches
        run_b()
        R_c = run_c()
        R_a = Rd.cpu().numpy()[:, :, 0, 0]
        assert np.array_equal(Rb[0].cpu().numpy()[:, 0, 0], R_a[:, 0])  # stage 0 is bspatom_resolvent (C4, C5)
        t = {"a": [], "b": [], "c": []}
        for _ in range(REPS):
            for key, run in (("a", run_a), ("b", run_b), ("c", run_c)):
                t[key].append(wall(run)[0])
        assert np.array_equal(Rd.cpu().numpy()[:, :, 0, 0], R_a)        # the same bits after every repetition
        med = {k_: statistics.median(v) for k_, v in t.items()}
        ab = [x / y for x, y in zip(t["a"], t["b"])]
        ca = [x / y for x, y in zip(t["c"], t["a"])]
        bspread = (max(t["b"]) - min(t["b"])) / med["b"]
        r = {"nfun": n, "chain_ms": [round(1e3 * x, 3) for x in t["a"]], "two_batches_ms": [round(1e3 * x, 3) for x in t["b"]],
             "staged_route_ms": [round(1e3 * x, 3) for x in t["c"]],
             "chain_median_ms": round(1e3 * med["a"], 3), "two_batches_median_ms": round(1e3 * med["b"], 3),
             "staged_route_median_ms": round(1e3 * med["c"], 3), "chain_us_per_chain": round(1e6 * med["a"] / NCHAIN, 2),
             "chain_over_two_batches": round(med["a"] / med["b"], 3), "chain_over_two_batches_range": [round(min(ab), 3), round(max(ab), 3)],
             "two_batches_relative_spread": round(bspread, 4),
             "staged_over_chain": round(med["c"] / med["a"], 1), "staged_over_chain_range": [round(min(ca), 1), round(max(ca), 1)],
             "staged_equals_chain_bitwise": bool(np.array_equal(R_c, R_a[:, 1])),
             "max_rel_diff_staged": float(np.max(np.abs(R_c - R_a[:, 1]) / np.abs(R_a[:, 1]))),
             "R_first_last": [[R_a[0, 1].real, R_a[0, 1].imag], [R_a[-1, 1].real, R_a[-1, 1].imag]]}
        out["nfun_%d" % n] = r
        ms = lambda v: " ".join("%.3f" % x for x in v)
        lines.append("nfun = %d: (a) resolvent_chain_dev, 2 stages: %s ms (median %.3f, %.2f us per chain); (b) two resolvent_dev calls, 2 x %d "
                     "matrices, shared right-hand side: %s ms (median %.3f, (max - min) / median = %.1f %%); (c) resolvent with X, host.band_apply, "
                     "%d resolvent calls with nmat = 1: %s ms (median %.3f); (a)/(b) = %.3f [%.3f .. %.3f]; (c)/(a) = %.1f [%.1f .. %.1f]; "
                     "(c)'s R equals (a)'s bit for bit: %s; R(0.55) = %.6e %+.6e i, R(1.5) = %.6e %+.6e i"
                     % (n, ms(r["chain_ms"]), r["chain_median_ms"], r["chain_us_per_chain"], NCHAIN, ms(r["two_batches_ms"]),
                        r["two_batches_median_ms"], 100.0 * bspread, NCHAIN, ms(r["staged_route_ms"]), r["staged_route_median_ms"],
                        r["chain_over_two_batches"], min(ab), max(ab), r["staged_over_chain"], min(ca), max(ca),
                        r["staged_equals_chain_bitwise"], R_a[0, 1].real, R_a[0, 1].imag, R_a[-1, 1].real, R_a[-1, 1].imag))
        prob.close()
        del bd, Wd, Gd, Rd, Rb
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/resolvent_chain_rate.py: bspatom_resolvent_chain_dev against two bspatom_resolvent_dev batches (no coupling) and "
                "against the staged route through the host, alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
