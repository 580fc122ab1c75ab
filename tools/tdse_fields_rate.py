#!/usr/bin/env python3
"""tdse_fields_rate.py -- what a second drive field costs per step inside bspatom_tdse_fields_dev, in one process on one GPU, on the
workload of tools/tdse_static_rate.py: 32 channels in a chain, 256 states each, 500 steps, one in-channel kind-1 block per channel
(symmetric positive, norm 0.5), at nscan = 1 and nscan = 16.  Writes a text report (default profiles/r16_tdse_fields.txt) and prints
one JSON line.

  (a) bspatom_tdse_static_dev, scheme = 1: one field on all 31 pairs;
  (b) bspatom_tdse_fields_dev, scheme = 1, on the same blocks with every second pair moved to field 1 and both fields given the same
      table: the same reads and the same matrix instructions, two pairs of accumulators, the kernels of csrc/tdse_fields.hip.

(a) and (b) alternate, three repetitions each after one untimed short run of each; every time is wall time between synchronised
points.  The report quotes every repetition, the medians, (b)/(a), the stage slot of both under option "ktime", and how far the results
are apart (the same equation in another order of the epilogue's sums).

    timeout -k 10 600 python tools/tdse_fields_rate.py [--out FILE] [--steps N]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_tdse_fields.txt"))
    ap.add_argument("--steps", type=int, default=500)
    args = ap.parse_args()
    nsteps = args.steps
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=20.0, k=4, nfun=8, l_fin=0, n0_ini=1, l_ini=0, zatom=1.0))
    rng = np.random.default_rng(9)
    E = np.sort(rng.uniform(-0.5, 2.0, size=(NCH, COUNT)), axis=1)
    pairs = [(c, c + 1) for c in range(NCH - 1)]
    fidx = [p % 2 for p in range(NCH - 1)]
    D = rng.standard_normal((NCH - 1, COUNT, COUNT)) / np.sqrt(COUNT)
    G = rng.standard_normal((NCH, COUNT, COUNT))
    W = G @ G.transpose(0, 2, 1) + 0.1 * np.eye(COUNT)[None]
    W *= (0.5 / np.linalg.norm(W, 2, axis=(1, 2)))[:, None, None]
    W = np.ascontiguousarray(W)
    spairs, skind = [(c, c) for c in range(NCH)], np.ones(NCH, dtype=np.int32)
    dev = "cuda:0"
    Ed, Dd, Wd = torch.from_numpy(E).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(W).to(dev)
    out, lines = {"workload": "%d channels in a chain, %d states, %d steps, dt %g, %d absorbers of norm 0.5; (b): pairs 1, 3, .. on field 1"
                  % (NCH, COUNT, nsteps, DT, NCH)}, []
    for nscan in (1, 16):
        a0 = rng.standard_normal((nscan, NCH, COUNT)) + 1j * rng.standard_normal((nscan, NCH, COUNT))
        a0 /= np.sqrt(np.sum(np.abs(a0) ** 2, axis=(1, 2)))[:, None, None]
        T = nsteps * DT
        amps = 0.2 + 0.05 * np.arange(nscan)
        field = host.field_table([(lambda t, A_=A_: A_ * np.sin(np.pi * t / T) ** 2 * np.cos(1.1 * t)) for A_ in amps], 0.0, DT, nsteps)
        field2 = np.ascontiguousarray(np.stack([field, field], axis=2))         # (nsteps, 6, 2, nscan): both fields the same table
        fd, f2d = torch.from_numpy(field).to(dev), torch.from_numpy(field2).to(dev)
        ad = torch.from_numpy(a0).to(dev)
        a0d = ad.clone()
        static = (spairs, skind, Wd.data_ptr())
        run_a = lambda n: prob.tdse_static_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr(),
                                               static, scheme=1)
        run_b = lambda n: prob.tdse_fields_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), fidx, 2, nscan, n, DT, f2d.data_ptr(),
                                               ad.data_ptr(), static, scheme=1)
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
        diff = float(np.max(np.abs(res["b"] - res["a"])))
        capi.set_option("ktime", 1)
        capi.kernel_times()
        slot = {}
        for key, run in runs:
            ad.copy_(a0d)
            run(1)
            ms1, n1 = stage_slot()
            ad.copy_(a0d)
            run(11)
            ms11, n11 = stage_slot()
            slot[key] = (round(1e3 * (ms11 - ms1) / (n11 - n1), 2), n11)
        capi.set_option("ktime", 0)
        med = {k: statistics.median(v) for k, v in t.items()}
        r = {"nscan": nscan}
        for k, name in (("a", "static"), ("b", "fields")):
            r[name + "_ms_per_step"] = [round(1e3 * x / nsteps, 4) for x in t[k]]
            r[name + "_median"] = round(1e3 * med[k] / nsteps, 4)
            r[name + "_stage_us_per_launch"] = slot[k][0]
        r.update({"b_over_a": round(med["b"] / med["a"], 3), "b_minus_a_us_per_step": round(1e6 * (med["b"] - med["a"]) / nsteps, 2),
                  "stage_slot_launches_11_steps": slot["b"][1], "max_abs_diff_a_b": diff, "max_err_fields": float(np.max(err["b"])),
                  "max_err_static": float(np.max(err["a"]))})
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: (a) static, one field %s ms/step (median %.4f), (b) fields, two fields %s ms/step (median %.4f); "
                     "(b)/(a) = %.3f, (b)-(a) = %.2f us/step; stage slot under events: %.2f us per stage launch of (a), %.2f of (b), "
                     "%d launches of (b) in 11 steps; max|a_(a) - a_(b)| %.3g; err %.3g (a), %.3g (b)"
                     % (nscan, " ".join("%.4f" % x for x in r["static_ms_per_step"]), r["static_median"],
                        " ".join("%.4f" % x for x in r["fields_ms_per_step"]), r["fields_median"], r["b_over_a"], r["b_minus_a_us_per_step"],
                        slot["a"][0], slot["b"][0], slot["b"][1], diff, r["max_err_static"], r["max_err_fields"]))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_fields_rate.py: bspatom_tdse_fields_dev (two fields with the same table) against bspatom_tdse_static_dev on the "
                "same blocks, alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
