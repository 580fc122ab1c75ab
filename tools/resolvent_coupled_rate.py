#!/usr/bin/env python3
"""resolvent_coupled_rate.py -- the rate of bspatom_resolvent_coupled_dev (csrc/resolvent_coupled.hip) in one process on one GPU,
against the only route there was for a coupling to all orders -- the dense complex matrix in torch -- and against the same channels
without the coupling.  Workload: hydrogen, linear grid, k = 9, nfun = 1024 and 4096; four channels l = 0..3 in a static field
F = 0.01 (host.stark_system: six coupling entries on the band of r), the absorber cap_profile(r, 0.75 rb, 1e-3) on every channel,
64 energies E_1s + omega, omega in [0.55, 1.5]; one right-hand side (r |1s> in channel 1), one projection, R only.

  (a) Problem.resolvent_coupled_dev: the 64 matrices of order 4 nfun, half-width 35, in ONE call;
  (b) torch.linalg.solve on the dense complex128 matrices of the same systems on the same GPU, one matrix at a time (order 16384 is
      4.3 GB a matrix); the matrix is formed on the device as A - z S from two resident dense matrices and only the solve is timed.
      At nfun = 1024 all 64 are solved per repetition; at nfun = 4096 NDENSE_BIG of them, and the time for 64 is that times
      64 / NDENSE_BIG (each costs the same: the order decides);
  (c) Problem.resolvent_dev on the 4 x 64 single-channel matrices (the same l, z, absorber, one shared right-hand side) in one
      call: the uncoupled lower bound -- it does not solve the coupled system.

One untimed run of each, then REPS repetitions of (a) and (c) alternating and REPS_DENSE of (b).  Every time is wall time between
synchronised points.  The ratios are the medians'; the bracket beside a ratio is the range of the per-repetition ratios.  The R of
(b) are compared with (a)'s, and the backward errors of both solutions of the first system say whose error a difference is.
Writes a text report (default profiles/r20_resolvent_coupled.txt) and prints one JSON line.

Measured on one MI355X (profiles/r20_resolvent_coupled.txt): nfun = 1024: (a) 13.52 ms, (b) 2773 ms, (c) 2.44 ms; (b)/(a) = 205,
(a)/(c) = 5.54.  nfun = 4096: (a) 53.45 ms, (b) 28803 ms for 64 (4 timed), (c) 8.94 ms; (b)/(a) = 539, (a)/(c) = 5.98.  (DESIGN.md 4.7
reads the ratios.)

    timeout -k 10 900 python tools/resolvent_coupled_rate.py [--out FILE] [--sizes 1024,4096]
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

NE, NCH, K, F, REPS, REPS_DENSE, NDENSE_BIG = 64, 4, 9, 0.01, 5, 3, 4


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def dense_parts(SB, HB, WB, G, couplings, a, dev):
    """(A, S) on the device, channel-major: A = sum_c (H_c - i W) + V and S = sum_c S, so that M(z) = A - z S; block by block"""
    n = SB.shape[1]
    A = torch.zeros((NCH * n, NCH * n), dtype=torch.complex128, device=dev)
    S = torch.zeros_like(A)
    for c in range(NCH):
        blk = host.coupled_dense(SB, HB, [c], [0.0], None, None, None, W=WB)
        A[c * n:(c + 1) * n, c * n:(c + 1) * n] = torch.from_numpy(blk).to(dev)
        S[c * n:(c + 1) * n, c * n:(c + 1) * n] = torch.from_numpy(-host.coupled_dense(SB, 0.0 * HB, [c], [1.0], None, None, None)).to(dev)
    Gd = host._full_to_dense(G, np.float64)
    for p, (cr, cc, ctr) in enumerate(couplings):
        A[cr * n:(cr + 1) * n, cc * n:(cc + 1) * n] += torch.from_numpy(a[p] * (Gd.T if ctr else Gd)).to(dev)
    return A, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_resolvent_coupled.txt"))
    ap.add_argument("--sizes", default="1024,4096")
    args = ap.parse_args()
    dev = "cuda:0"
    out = {"workload": "%d energies, %d channels l = 0..%d coupled by F z (F = %g), k = %d, absorber on, nrhs = 1, nproj = 1, R only"
                       % (NE, NCH, NCH - 1, F, K)}
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        rb = 0.25 * n
        prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=NCH - 1, n0_ini=1, l_ini=0, zatom=1.0))
        E, info = prob.solve(0, NCH)
        assert np.all(info == 0)
        RB = prob.dipole_bands()
        b = np.zeros((NCH, n), dtype=np.complex128)
        b[1] = host.band_apply(RB[0], prob.eigvecs(0, 1, 1))[0]
        WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
        couplings, a = host.stark_system([(l, 0) for l in range(NCH)], F)
        G = np.ascontiguousarray(RB[0])
        zs = (E[0, 0] + np.linspace(0.55, 1.5, NE)).astype(np.complex128)
        l = np.arange(NCH, dtype=np.int32)
        z = np.repeat(zs[:, None], NCH, axis=1)
        bd, Wd, Gd = torch.from_numpy(b).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(G).to(dev)
        Rd = torch.zeros((NE, 1, 1), dtype=torch.complex128, device=dev)
        Rs = torch.zeros((NE * NCH, 1, 1), dtype=torch.complex128, device=dev)
        ls, zs_rep = np.tile(l, NE), np.repeat(zs, NCH)
        b1 = bd[1].contiguous()

        def run_a():
            return prob.resolvent_coupled_dev(l, z, 1, bd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a, nabs=1,
                                              W_ptr=Wd.data_ptr(), nproj=1, P_ptr=bd.data_ptr(), R_ptr=Rd.data_ptr())

        def run_c():
            return prob.resolvent_dev(ls, zs_rep, 1, b1.data_ptr(), nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=b1.data_ptr(), R_ptr=Rs.data_ptr())

        assert np.all(run_a() == 0)                                    # untimed: first launches
        assert np.all(run_c() == 0)
        R_a = Rd.cpu().numpy()[:, 0, 0]
        t = {"a": [], "c": [], "b": []}
        for _ in range(REPS):
            for key, run in (("a", run_a), ("c", run_c)):
                t[key].append(wall(run)[0])
        assert np.array_equal(Rd.cpu().numpy()[:, 0, 0], R_a)          # the same bits after every repetition
        # the dense route; the bands of the last solve are read back through assemble, which ends the state of the solve
        SB, HB = prob.assemble(0, NCH)
        A, S = dense_parts(SB, HB, WB, G, couplings, a, dev)
        bf = bd.reshape(-1, 1)
        nd = NE if NCH * n <= 4096 else NDENSE_BIG
        R_b = np.zeros(nd, dtype=np.complex128)

        def run_b():
            for m in range(nd):
                M = A - complex(zs[m]) * S
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = torch.linalg.solve(M, bf)
                torch.cuda.synchronize()
                run_b.t += time.perf_counter() - t0
                R_b[m] = complex(torch.sum(bf * x))
                del M, x

        run_b.t = 0.0
        run_b()                                                        # untimed
        for _ in range(REPS_DENSE):
            run_b.t = 0.0
            run_b()
            t["b"].append(run_b.t * NE / nd)
        rel = float(np.max(np.abs(R_b - R_a[:nd]) / np.abs(R_a[:nd])))
        # whose error the difference is: the backward errors of both solutions of the first system, in complex128 on the device
        M = A - complex(zs[0]) * S
        Xd = torch.zeros((1, 1, NCH, n), dtype=torch.complex128, device=dev)
        prob.resolvent_coupled_dev(l, z[0], 1, bd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a, nabs=1,
                                   W_ptr=Wd.data_ptr(), X_ptr=Xd.data_ptr())
        scale = float(torch.max(torch.sum(torch.abs(M), dim=1)))
        omega = lambda x: float(torch.max(torch.abs(bf - M @ x)) / (scale * float(torch.max(torch.abs(x))) + float(torch.max(torch.abs(bf)))))
        om_a, om_b = omega(Xd.reshape(-1, 1)), omega(torch.linalg.solve(M, bf))
        del M, Xd
        med = {k_: statistics.median(v) for k_, v in t.items()}
        ac = [x / y for x, y in zip(t["a"], t["c"])]
        ba = [x / med["a"] for x in t["b"]]
        spread = lambda v: (max(v) - min(v)) / statistics.median(v)
        r = {"nfun": n, "order": NCH * n, "half_width": NCH * K - 1,
             "coupled_ms": [round(1e3 * x, 3) for x in t["a"]], "uncoupled_ms": [round(1e3 * x, 3) for x in t["c"]],
             "dense_ms_for_64": [round(1e3 * x, 1) for x in t["b"]], "dense_matrices_timed": nd,
             "coupled_median_ms": round(1e3 * med["a"], 3), "uncoupled_median_ms": round(1e3 * med["c"], 3),
             "dense_median_ms_for_64": round(1e3 * med["b"], 1), "coupled_ms_per_matrix": round(1e3 * med["a"] / NE, 3),
             "coupled_relative_spread": round(spread(t["a"]), 4), "dense_relative_spread": round(spread(t["b"]), 4),
             "dense_over_coupled": round(med["b"] / med["a"], 1), "dense_over_coupled_range": [round(min(ba), 1), round(max(ba), 1)],
             "coupled_over_uncoupled": round(med["a"] / med["c"], 2), "coupled_over_uncoupled_range": [round(min(ac), 2), round(max(ac), 2)],
             "max_rel_diff_dense": rel, "backward_error_coupled": om_a, "backward_error_dense": om_b, "R_first_last": [[R_a[0].real, R_a[0].imag], [R_a[-1].real, R_a[-1].imag]]}
        out["nfun_%d" % n] = r
        ms = lambda v: " ".join("%.3f" % x for x in v)
        lines.append("nfun = %d (order %d, half-width %d): (a) resolvent_coupled_dev, %d matrices: %s ms (median %.3f, %.3f ms per matrix, "
                     "(max - min) / median = %.1f %%); (b) torch.linalg.solve, dense complex128, one matrix at a time, %d timed, for 64: %s ms "
                     "(median %.1f, (max - min) / median = %.1f %%); (c) resolvent_dev, %d single-channel matrices: %s ms (median %.3f); "
                     "(b)/(a) = %.1f [%.1f .. %.1f]; (a)/(c) = %.2f [%.2f .. %.2f]; max relative difference of R, dense against (a): %.1e (backward error of the first system in complex128: (a) %.1e, dense "
                     "%.1e); R(0.55) = %.6e %+.6e i, R(1.5) = %.6e %+.6e i"
                     % (n, NCH * n, NCH * K - 1, NE, ms(r["coupled_ms"]), r["coupled_median_ms"], r["coupled_ms_per_matrix"],
                        100.0 * spread(t["a"]), nd, " ".join("%.1f" % x for x in r["dense_ms_for_64"]), r["dense_median_ms_for_64"],
                        100.0 * spread(t["b"]), NE * NCH, ms(r["uncoupled_ms"]), r["uncoupled_median_ms"], r["dense_over_coupled"], min(ba),
                        max(ba), r["coupled_over_uncoupled"], min(ac), max(ac), rel, om_a, om_b, R_a[0].real, R_a[0].imag, R_a[-1].real, R_a[-1].imag))
        prob.close()
        del bd, Wd, Gd, Rd, Rs, A, S, bf, b1
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/resolvent_coupled_rate.py: bspatom_resolvent_coupled_dev against torch.linalg.solve on the dense matrices of the same "
                "systems and against the uncoupled single-channel solves, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
