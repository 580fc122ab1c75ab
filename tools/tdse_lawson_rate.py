#!/usr/bin/env python3
"""tdse_lawson_rate.py -- what the rotations of bspatom_tdse_lawson_dev cost per step, in one process on one GPU, on the workload of
tools/tdse_rate.py: 32 channels in a chain, 256 states each, 500 steps, at nscan = 1 and nscan = 16.  Writes a text report (default
profiles/r14_tdse_lawson.txt) and prints one JSON line.

  (a) bspatom_tdse_propagate_dev: the plain steps (seven launches per step);
  (b) bspatom_tdse_lawson_dev without observables: the same launches with the rotation in the operand load and in the epilogue, plus
      the phase-table kernel once per call.

(a) and (b) alternate, three repetitions each after one untimed short run of both; every time is wall time between synchronised
points.  The report quotes every repetition, the medians, (b)/(a) and (b)-(a), the stage slot of (b) under option "ktime", and the
phase-table kernel's own time: the slot's sum of a one-step call (six stages and the table) less six stages at the per-launch time
of an eleven-step call.  The workload's spectrum lies in (-0.5, 2) with dt = 0.01, so both schemes are stable on it and the
difference of their results is reported as well (both are 5th-order approximations of the same solution).

    timeout -k 10 600 python tools/tdse_lawson_rate.py [--out FILE] [--steps N]
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

NCH, COUNT, DT, REPS = 32, 256, 0.01, 3


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def stage_slot():
    return next(v for k, v in capi.kernel_times().items() if "tdse_stage_kernel" in k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_tdse_lawson.txt"))
    ap.add_argument("--steps", type=int, default=500)
    args = ap.parse_args()
    nsteps = args.steps
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=20.0, k=4, nfun=8, l_fin=0, n0_ini=1, l_ini=0, zatom=1.0))
    rng = np.random.default_rng(9)
    E = np.sort(rng.uniform(-0.5, 2.0, size=(NCH, COUNT)), axis=1)
    pairs = [(c, c + 1) for c in range(NCH - 1)]
    D = rng.standard_normal((NCH - 1, COUNT, COUNT)) / np.sqrt(COUNT)
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(D).to(dev)
    out, lines = {"workload": "%d channels in a chain, %d states, %d steps, dt %g" % (NCH, COUNT, nsteps, DT)}, []
    for nscan in (1, 16):
        a0 = rng.standard_normal((nscan, NCH, COUNT)) + 1j * rng.standard_normal((nscan, NCH, COUNT))
        a0 /= np.sqrt(np.sum(np.abs(a0) ** 2, axis=(1, 2)))[:, None, None]
        T = nsteps * DT
        amps = 0.2 + 0.05 * np.arange(nscan)
        field = host.field_table([(lambda t, A_=A_: A_ * np.sin(np.pi * t / T) ** 2 * np.cos(1.1 * t)) for A_ in amps], 0.0, DT, nsteps)
        fd = torch.from_numpy(field).to(dev)
        ad = torch.from_numpy(a0).to(dev)
        a0d = ad.clone()
        run_a = lambda n: prob.tdse_propagate_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr())
        run_b = lambda n: prob.tdse_lawson_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr())
        runs = (("a", run_a), ("b", run_b))
        for _, run in runs:                                          # the first launches outside the timing
            ad.copy_(a0d)
            run(2)
        t, res, err = {"a": [], "b": []}, {}, {}
        for _ in range(REPS):
            for key, run in runs:
                ad.copy_(a0d)
                dt_, err[key] = wall(lambda: run(nsteps))
                t[key].append(dt_)
                res[key] = ad.cpu().numpy()
        diff = float(np.max(np.abs(res["a"] - res["b"])))
        capi.set_option("ktime", 1)
        capi.kernel_times()
        ad.copy_(a0d)
        run_b(1)
        ms1, n1 = stage_slot()
        ad.copy_(a0d)
        run_b(11)
        ms11, n11 = stage_slot()
        capi.set_option("ktime", 0)
        per_stage = (ms11 - ms1) / (n11 - n1)
        ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
        r = {"nscan": nscan, "propagate_ms_per_step": [round(1e3 * x / nsteps, 4) for x in t["a"]],
             "lawson_ms_per_step": [round(1e3 * x / nsteps, 4) for x in t["b"]],
             "propagate_median": round(1e3 * ma / nsteps, 4), "lawson_median": round(1e3 * mb / nsteps, 4),
             "b_over_a": round(mb / ma, 3), "b_minus_a_us_per_step": round(1e6 * (mb - ma) / nsteps, 2),
             "stage_slot_launches_11_steps": n11, "stage_slot_us_per_launch": round(1e3 * per_stage, 2),
             "phase_kernel_us": round(1e3 * (ms1 - 6 * per_stage), 2), "max_abs_diff_a_b": diff,
             "max_err_propagate": float(np.max(err["a"])), "max_err_lawson": float(np.max(err["b"]))}
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: (a) propagate %s ms/step (median %.4f), (b) lawson %s ms/step (median %.4f); (b)/(a) = %.3f, "
                     "(b)-(a) = %.2f us/step; stage slot of (b): %d launches in 11 steps (66 stages + the phase table), %.2f us per stage "
                     "under events, phase-table kernel %.2f us; max|a_(a) - a_(b)| %.3g; err %.3g (a), %.3g (b)"
                     % (nscan, " ".join("%.4f" % x for x in r["propagate_ms_per_step"]), r["propagate_median"],
                        " ".join("%.4f" % x for x in r["lawson_ms_per_step"]), r["lawson_median"], r["b_over_a"], r["b_minus_a_us_per_step"],
                        n11, r["stage_slot_us_per_launch"], r["phase_kernel_us"], diff, r["max_err_propagate"], r["max_err_lawson"]))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_lawson_rate.py: bspatom_tdse_lawson_dev against bspatom_tdse_propagate_dev, alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
