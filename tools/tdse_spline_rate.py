#!/usr/bin/env python3
"""tdse_spline_rate.py -- the rate of bspatom_tdse_spline_dev (csrc/tdse_spline.hip) in one process on one GPU, against the same
factorisations without the time stepping and against the route there was.  Workload: tools/resolvent_coupled_rate.py's -- hydrogen,
linear grid, k = 9, nfun = 1024 and 4096; four channels l = 0..3 coupled by F(t) z (host.stark_system on the band of r), the absorber
cap_profile(r, 0.75 rb, 1e-3) on every channel -- with nscan = 64 packets (1s, each scan its own peak field) and nsteps = 32 steps
dt = 0.05 of a sin^2 pulse.

  (a) Problem.tdse_spline_dev: 64 packets x 32 steps in one call, no rows, no snapshots;
  (b) the same number of matrices, nscan * nsteps = 2048, each with its step's coefficients at z = 2i/dt, through
      Problem.resolvent_coupled_dev with nrhs = 1 and X only: the same assembly, factorisation and solve (the kernel that was there),
      WITHOUT the dependence of a step on the step before -- all 2048 matrices are independent work;
  (b64) the same call under resolvent_slots = 64: as many resident workgroups as (a) has packets.  (a)/(b64) is what a step adds to a
      factorisation (b = S c, the update, the barriers); (a)/(b) also contains what the sequence of steps costs in parallelism;
  (c) the route there was, on NSTEPS_C steps, scaled to 32: per step and scan host.band_apply on the packet, one
      Problem.resolvent_coupled call with nmat = 1 (host arrays), the update in NumPy.

One untimed run of each, then REPS repetitions of (a), (b), (b64) alternating and REPS_C of (c).  Wall time between synchronised
points; medians, and (max - min) / median as the spread.  (a) restarts from the same packets every repetition and must return the
same bits.  Writes a text report (default profiles/r22_tdse_spline.txt) and prints one JSON line.

Measured on one MI355X (profiles/r22_tdse_spline.txt): nfun = 1024: (a) 413.5 ms, (b) 105.7 ms, (b64) 418.9 ms, (c) 27.9 s; (a)/(b) =
3.91, (a)/(b64) = 0.987, (c)/(a) = 67.5.  nfun = 4096: (a) 1685.1 ms, (b) 1438.6 ms (73 slots: the scratch bound), (b64) 1701.2 ms,
(c) 108.8 s; (a)/(b) = 1.17, (a)/(b64) = 0.991, (c)/(a) = 64.6.  (DESIGN.md 4.7 reads the ratios: 64 packets are 64 workgroups.)

    timeout -k 10 900 python tools/tdse_spline_rate.py [--out FILE] [--sizes 1024,4096]
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

NSCAN, NSTEPS, NCH, K, DT, REPS, REPS_C, NSTEPS_C = 64, 32, 4, 9, 0.05, 5, 3, 2


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_tdse_spline.txt"))
    ap.add_argument("--sizes", default="1024,4096")
    args = ap.parse_args()
    dev = "cuda:0"
    out = {"workload": "%d packets x %d steps dt = %g, %d channels l = 0..%d coupled by F(t) z, k = %d, absorber on, no rows"
                       % (NSCAN, NSTEPS, DT, NCH, NCH - 1, K)}
    lines = []
    for n in [int(s) for s in args.sizes.split(",")]:
        rb = 0.25 * n
        prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=NCH - 1, n0_ini=1, l_ini=0, zatom=1.0))
        E, info = prob.solve(0, NCH)
        assert np.all(info == 0)
        chans = [(l, 0) for l in range(NCH)]
        G = np.ascontiguousarray(prob.dipole_bands()[0])
        WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
        c0 = np.ascontiguousarray(np.broadcast_to(host.spline_packet(prob, chans, 0, prob.eigvecs(0, 1, 1)[0]), (NSCAN, NCH, n)))
        couplings, a1 = host.stark_system(chans, 1.0)
        tm = host.spline_midpoints(0.0, DT, NSTEPS)
        F = np.linspace(0.01, 0.1, NSCAN)[None, :] * (np.sin(np.pi * tm / (NSTEPS * DT)) ** 2)[:, None]
        coef = host.spline_coefficients((couplings, a1), F)            # (NSTEPS, NSCAN, ncoup, 1)
        l = np.arange(NCH, dtype=np.int32)
        put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        c0d, Gd, Wd, coefd = put(c0), put(G), put(WB), put(coef)
        cd = torch.empty_like(c0d)
        Xd = torch.zeros((NSCAN * NSTEPS, 1, NCH, n), dtype=torch.complex128, device=dev)
        z = np.full((NSCAN * NSTEPS, NCH), 2j / DT)
        a_b = coef.reshape(NSCAN * NSTEPS, len(couplings), 1)

        def run_a():
            cd.copy_(c0d)
            return prob.tdse_spline_dev(l, NSCAN, NSTEPS, DT, cd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(),
                                        coef_ptr=coefd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr())

        def run_b():
            return prob.resolvent_coupled_dev(l, z, 1, c0d.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a_b, nabs=1,
                                              W_ptr=Wd.data_ptr(), X_ptr=Xd.data_ptr())

        def run_b64():
            capi.set_option("resolvent_slots", NSCAN)
            try:
                return run_b()
            finally:
                capi.set_option("resolvent_slots", 0)

        assert np.all(run_a() == 0)                                    # untimed: first launches
        c_first = cd.cpu().numpy()
        assert np.all(run_b() == 0) and np.all(run_b64() == 0)
        t = {"a": [], "b": [], "b64": [], "c": []}
        for _ in range(REPS):
            for key, run in (("a", run_a), ("b", run_b), ("b64", run_b64)):
                t[key].append(wall(run)[0])
        assert np.array_equal(cd.cpu().numpy().view(np.uint64), c_first.view(np.uint64))   # the same bits after every repetition
        # the route there was: band_apply, one coupled call with nmat = 1 and the update, per step and scan, on the host's arrays
        SBf = host.band_symmetric(prob.assemble(0, NCH)[0])
        g = 4.0 / DT

        def run_c():
            c = np.array(c0)
            for s in range(NSTEPS_C):
                for q in range(NSCAN):
                    b = host.band_apply(SBf, c[q].real) + 1j * host.band_apply(SBf, c[q].imag)
                    x = prob.resolvent_coupled(l, 2j / DT, b, couplings=couplings, G=G, a=coef[s, q], W=WB)[0][0, 0]
                    c[q] = (g * x.imag - c[q].real) + 1j * (-(g * x.real) - c[q].imag)
            return c

        run_c()                                                        # untimed
        for _ in range(REPS_C):
            tc, cc = wall(run_c)
            t["c"].append(tc * NSTEPS / NSTEPS_C)
        # the first NSTEPS_C steps of (a) are (c) bit for bit (guarantee S3)
        cd.copy_(c0d)
        prob.tdse_spline_dev(l, NSCAN, NSTEPS_C, DT, cd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), coef_ptr=coefd.data_ptr(),
                             nabs=1, W_ptr=Wd.data_ptr())
        assert np.array_equal(cd.cpu().numpy().view(np.uint64), np.ascontiguousarray(cc).view(np.uint64))
        rows = prob.tdse_spline(l, c_first, DT, 0, obs_every=1)[2]
        norm = rows[0].sum(-1)
        med = {k_: statistics.median(v) for k_, v in t.items()}
        spread = lambda v: (max(v) - min(v)) / statistics.median(v)
        ratio = lambda x, y: [p / q for p, q in zip(t[x], t[y])]
        r = {"nfun": n, "order": NCH * n, "half_width": NCH * K - 1, "matrices": NSCAN * NSTEPS}
        for key, name in (("a", "spline"), ("b", "coupled"), ("b64", "coupled_64_slots"), ("c", "host_route_for_32_steps")):
            r[name + "_ms"] = [round(1e3 * x, 3) for x in t[key]]
            r[name + "_median_ms"] = round(1e3 * med[key], 3)
            r[name + "_relative_spread"] = round(spread(t[key]), 4)
        r["spline_over_coupled"] = round(med["a"] / med["b"], 3)
        r["spline_over_coupled_range"] = [round(min(ratio("a", "b")), 3), round(max(ratio("a", "b")), 3)]
        r["spline_over_coupled_64_slots"] = round(med["a"] / med["b64"], 3)
        r["spline_over_coupled_64_slots_range"] = [round(min(ratio("a", "b64")), 3), round(max(ratio("a", "b64")), 3)]
        r["host_route_over_spline"] = round(med["c"] / med["a"], 1)
        r["spline_ms_per_step_and_packet"] = round(1e3 * med["a"] / (NSCAN * NSTEPS), 4)
        r["norm_after_run_first_last"] = [float(norm[0]), float(norm[-1])]
        out["nfun_%d" % n] = r
        ms = lambda v: " ".join("%.3f" % x for x in v)
        lines.append("nfun = %d (order %d, half-width %d), %d packets x %d steps: (a) tdse_spline_dev: %s ms (median %.3f, (max - min) / median "
                     "= %.1f %%); (b) resolvent_coupled_dev, %d independent matrices, X only: %s ms (median %.3f, %.1f %%); (b64) the same "
                     "under resolvent_slots = %d: %s ms (median %.3f, %.1f %%); (c) band_apply + resolvent_coupled(nmat = 1) + update per "
                     "step and scan on the host, %d steps timed, for %d: %s ms (median %.1f, %.1f %%); (a)/(b) = %.3f [%.3f .. %.3f]; "
                     "(a)/(b64) = %.3f [%.3f .. %.3f]; (c)/(a) = %.1f; norm left after the run: %.6f (weakest field) .. %.6f (strongest)"
                     % (n, NCH * n, NCH * K - 1, NSCAN, NSTEPS, ms(r["spline_ms"]), r["spline_median_ms"], 100 * spread(t["a"]), NSCAN * NSTEPS,
                        ms(r["coupled_ms"]), r["coupled_median_ms"], 100 * spread(t["b"]), NSCAN, ms(r["coupled_64_slots_ms"]),
                        r["coupled_64_slots_median_ms"], 100 * spread(t["b64"]), NSTEPS_C, NSTEPS, " ".join("%.1f" % (1e3 * x) for x in t["c"]),
                        1e3 * med["c"], 100 * spread(t["c"]), r["spline_over_coupled"], *r["spline_over_coupled_range"],
                        r["spline_over_coupled_64_slots"], *r["spline_over_coupled_64_slots_range"], r["host_route_over_spline"], norm[0], norm[-1]))
        prob.close()
        del c0d, Gd, Wd, coefd, cd, Xd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_spline_rate.py: bspatom_tdse_spline_dev against the same matrices through bspatom_resolvent_coupled_dev and against "
                "the host route there was, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
