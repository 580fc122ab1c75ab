#!/usr/bin/env python3
"""tdse_adapt_rate.py -- what step-size control on the device buys and costs inside bspatom_tdse_adaptive_dev, in one process on one
GPU, on the workload of tools/tdse_static_rate.py: 32 channels in a chain, 256 states each, one in-channel absorber per channel
(symmetric positive, norm 0.5), Lawson steps, at nscan = 1 and nscan = 16.  The pulse is a sin^2 envelope over the whole run
(T = nsteps dt, 64 coarse steps of 0.16 and amplitude 3 (1 + 0.05 q) by default) on a carrier, given as a node table of 4 intervals per coarse step.  Writes a text
report (default profiles/r17_tdse_adapt.txt) and prints one JSON line.

  (a) bspatom_tdse_adaptive_dev at tol (default 1e-6), max_level 4, from level 0;
  (b) bspatom_tdse_static_dev at the fixed step of the deepest level that (a) reached: nsteps 2^deep steps of dt / 2^deep;
  (c) bspatom_tdse_adaptive_dev with tol = +inf and max_level 0 on (b)'s grid -- the same steps as (b), every one an attempt: the price
      of an attempt's extra launches (the controller and the commit: 9 launches against 7).

(a), (b) and (c) alternate, three repetitions each after one untimed run of each; every time is wall time between synchronised points.
The report quotes every repetition, the medians, the step counts of (a), (a)/(b), (c)/(b) and the launches of slot 10 per attempt.

    timeout -k 10 900 python tools/tdse_adapt_rate.py [--out FILE] [--steps N] [--tol TOL] [--amp A]
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

NCH, COUNT, DT, NSUB, MAX_LEVEL, REPS = 32, 256, 0.16, 4, 4, 3


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def tdse_slot():
    return next(v for k, v in capi.kernel_times().items() if "tdse_stage_kernel" in k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_tdse_adapt.txt"))
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--amp", type=float, default=3.0)
    args = ap.parse_args()
    nsteps, tol = args.steps, args.tol
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=20.0, k=4, nfun=8, l_fin=0, n0_ini=1, l_ini=0, zatom=1.0))
    rng = np.random.default_rng(9)
    E = np.sort(rng.uniform(-0.5, 2.0, size=(NCH, COUNT)), axis=1)
    pairs = [(c, c + 1) for c in range(NCH - 1)]
    D = rng.standard_normal((NCH - 1, COUNT, COUNT)) / np.sqrt(COUNT)
    G = rng.standard_normal((NCH, COUNT, COUNT))
    W = G @ G.transpose(0, 2, 1) + 0.1 * np.eye(COUNT)[None]
    W *= (0.5 / np.linalg.norm(W, 2, axis=(1, 2)))[:, None, None]
    W = np.ascontiguousarray(W)
    spairs, skind = [(c, c) for c in range(NCH)], np.ones(NCH, dtype=np.int32)
    dev = "cuda:0"
    Ed, Dd, Wd = torch.from_numpy(E).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(W).to(dev)
    static = (spairs, skind, Wd.data_ptr())
    T = nsteps * DT
    out, lines = {"workload": "%d channels in a chain, %d states, %d absorbers of norm 0.5, Lawson steps; %d coarse steps of %g, %d node "
                  "intervals each, sin^2 pulse of amplitude %g (1 + 0.05 q) over the run, tol %g, max_level %d"
                  % (NCH, COUNT, NCH, nsteps, DT, NSUB, args.amp, tol, MAX_LEVEL)}, []
    for nscan in (1, 16):
        a0 = rng.standard_normal((nscan, NCH, COUNT)) + 1j * rng.standard_normal((nscan, NCH, COUNT))
        a0 /= np.sqrt(np.sum(np.abs(a0) ** 2, axis=(1, 2)))[:, None, None]
        amps = args.amp * (1.0 + 0.05 * np.arange(nscan))
        fns = [(lambda t, A_=A_: A_ * np.sin(np.pi * t / T) ** 2 * np.cos(1.1 * t)) for A_ in amps]
        fnd = torch.from_numpy(host.field_nodes(fns, None, 0.0, DT, nsteps, NSUB)).to(dev)
        ad = torch.from_numpy(a0).to(dev)
        a0d = ad.clone()

        def run_a():
            return prob.tdse_adaptive_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, nsteps, DT, fnd.data_ptr(), ad.data_ptr(),
                                          static, tol, MAX_LEVEL, NSUB, 0, 1)

        ad.copy_(a0d)
        err_a, stats = run_a()                                        # untimed: the first launches, and the deepest level for (b), (c)
        deep = int(stats[3])
        nfine, hfine = nsteps << deep, float(np.ldexp(DT, -deep))
        fd = torch.from_numpy(host.field_table(fns, 0.0, hfine, nfine)).to(dev)
        fnfd = torch.from_numpy(host.field_nodes(fns, None, 0.0, hfine, nfine, 1)).to(dev)
        run_b = lambda: prob.tdse_static_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, nfine, hfine, fd.data_ptr(), ad.data_ptr(),
                                             static, scheme=1)
        run_c = lambda: prob.tdse_adaptive_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, nfine, hfine, fnfd.data_ptr(),
                                               ad.data_ptr(), static, float("inf"), 0, 1, 0, 1)
        runs = (("a", run_a), ("b", run_b), ("c", run_c))
        for _, run in runs[1:]:
            ad.copy_(a0d)
            run()
        t, res, ret = {"a": [], "b": [], "c": []}, {}, {}
        for _ in range(REPS):
            for key, run in runs:
                ad.copy_(a0d)
                dt_, ret[key] = wall(run)
                t[key].append(dt_)
                res[key] = ad.cpu().numpy()
        stats_a, stats_c = ret["a"][1], ret["c"][1]
        # the launches of slot 10 of one run of (a): the phase tables, the field of the first attempt, then the attempts
        capi.set_option("ktime", 1)
        capi.kernel_times()
        ad.copy_(a0d)
        run_a()
        ms_a, launches_a = tdse_slot()
        capi.set_option("ktime", 0)
        med = {k: statistics.median(v) for k, v in t.items()}
        r = {"nscan": nscan, "deepest_level": deep, "fine_steps": nfine,
             "adaptive": {"accepted": int(stats_a[0]), "rejected": int(stats_a[1]), "forced": int(stats_a[2]), "attempts": int(stats_a[5]),
                          "level_at_end": int(stats_a[4])}}
        for k, name in (("a", "adaptive"), ("b", "static_fine"), ("c", "adaptive_inf")):
            r[name + "_ms"] = [round(1e3 * x, 3) for x in t[k]]
            r[name + "_median_ms"] = round(1e3 * med[k], 3)
        r.update({"a_over_b": round(med["a"] / med["b"], 3), "c_over_b": round(med["c"] / med["b"], 3),
                  "adaptive_ms_per_attempt": round(1e3 * med["a"] / int(stats_a[5]), 4),
                  "static_ms_per_step": round(1e3 * med["b"] / nfine, 4), "inf_ms_per_attempt": round(1e3 * med["c"] / int(stats_c[5]), 4),
                  "slot10_launches_of_a": int(launches_a), "slot10_launches_per_attempt_of_a": round(launches_a / int(stats_a[5]), 2),
                  "max_abs_diff_a_b": float(np.max(np.abs(res["a"] - res["b"]))), "max_abs_diff_c_b": float(np.max(np.abs(res["c"] - res["b"]))),
                  "err_adaptive": float(np.max(ret["a"][0])), "err_static_fine": float(np.max(ret["b"]))})
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: (a) adaptive %s ms (median %.3f): %d accepted, %d rejected, %d forced of %d attempts, deepest level %d, "
                     "largest estimate %.3g; (b) static at level %d, %d steps: %s ms (median %.3f), estimate %.3g; (c) adaptive, tol = inf, on (b)'s "
                     "grid: %s ms (median %.3f); (a)/(b) = %.3f, (c)/(b) = %.3f (9/7 = 1.286); per attempt %.4f ms (a), %.4f ms (c), per step "
                     "%.4f ms (b); slot 10 of one run of (a): %d launches = %.2f per attempt (9 an attempt, %d phase tables, the first field, "
                     "and the launches enqueued behind the end, which return at once); max|a_(a) - a_(b)| %.3g, max|a_(c) - a_(b)| %.3g"
                     % (nscan, " ".join("%.3f" % x for x in r["adaptive_ms"]), r["adaptive_median_ms"], stats_a[0], stats_a[1], stats_a[2],
                        stats_a[5], deep, r["err_adaptive"], deep, nfine, " ".join("%.3f" % x for x in r["static_fine_ms"]),
                        r["static_fine_median_ms"], r["err_static_fine"], " ".join("%.3f" % x for x in r["adaptive_inf_ms"]),
                        r["adaptive_inf_median_ms"], r["a_over_b"], r["c_over_b"], r["adaptive_ms_per_attempt"], r["inf_ms_per_attempt"],
                        r["static_ms_per_step"], launches_a, r["slot10_launches_per_attempt_of_a"], MAX_LEVEL + 1, r["max_abs_diff_a_b"],
                        r["max_abs_diff_c_b"]))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_adapt_rate.py: bspatom_tdse_adaptive_dev against bspatom_tdse_static_dev at the fixed step of its deepest level, "
                "alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
