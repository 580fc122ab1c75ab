#!/usr/bin/env python3
"""tdse_static_rate.py -- what an absorber costs per step inside bspatom_tdse_static_dev, in one process on one GPU, on the workload of
tools/tdse_rate.py: 32 channels in a chain, 256 states each, 500 steps, at nscan = 1 and nscan = 16, one in-channel kind-1 block per
channel (symmetric positive, norm 0.5).  Writes a text report (default profiles/r15_tdse_static.txt) and prints one JSON line.

  (a) bspatom_tdse_lawson_dev: the Lawson steps without any static block;
  (b) bspatom_tdse_static_dev, scheme = 1, with the 32 absorbers: the same launches, every stage with 32 more blocks to read;
  (c) the route without the call: one single-step bspatom_tdse_lawson_dev call per step, followed by exp(-W dt) applied to every
      channel with torch (the propagators matrix_exp(-W dt) are built once, outside the timing): a split step, first order in dt.

(a), (b) and (c) alternate, three repetitions each after one untimed short run of each; every time is wall time between synchronised
points.  The report quotes every repetition, the medians, (b)/(a), (c)/(b), the stage slot of (b) under option "ktime", and how far
the results of (b) and (c) are apart (the splitting error of (c) and nothing else: both use the same blocks).

    timeout -k 10 900 python tools/tdse_static_rate.py [--out FILE] [--steps N]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_tdse_static.txt"))
    ap.add_argument("--steps", type=int, default=500)
    args = ap.parse_args()
    nsteps = args.steps
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
    Pd = torch.linalg.matrix_exp(-DT * Wd).to(torch.complex128)          # (c)'s propagators, once
    out, lines = {"workload": "%d channels in a chain, %d states, %d steps, dt %g, %d absorbers of norm 0.5"
                  % (NCH, COUNT, nsteps, DT, NCH)}, []
    for nscan in (1, 16):
        a0 = rng.standard_normal((nscan, NCH, COUNT)) + 1j * rng.standard_normal((nscan, NCH, COUNT))
        a0 /= np.sqrt(np.sum(np.abs(a0) ** 2, axis=(1, 2)))[:, None, None]
        T = nsteps * DT
        amps = 0.2 + 0.05 * np.arange(nscan)
        field = host.field_table([(lambda t, A_=A_: A_ * np.sin(np.pi * t / T) ** 2 * np.cos(1.1 * t)) for A_ in amps], 0.0, DT, nsteps)
        fd = torch.from_numpy(field).to(dev)
        ad = torch.from_numpy(a0).to(dev)
        a0d = ad.clone()
        fstep = 6 * nscan * 16                                           # bytes of one step of the field table
        static = (spairs, skind, Wd.data_ptr())
        run_a = lambda n: prob.tdse_lawson_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr())
        run_b = lambda n: prob.tdse_static_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr(),
                                               static, scheme=1)

        def run_c(n):
            err = np.zeros(nscan)
            for i in range(n):
                e = prob.tdse_lawson_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, 1, DT, fd.data_ptr() + i * fstep, ad.data_ptr())
                ad.copy_(torch.einsum("cij,qcj->qci", Pd, ad))
                err = np.maximum(err, e)
            return err

        runs = (("a", run_a), ("b", run_b), ("c", run_c))
        for _, run in runs:                                          # the first launches outside the timing
            ad.copy_(a0d)
            run(2)
        t, res, err = {"a": [], "b": [], "c": []}, {}, {}
        for _ in range(REPS):
            for key, run in runs:
                ad.copy_(a0d)
                dt_, err[key] = wall(lambda: run(nsteps))
                t[key].append(dt_)
                res[key] = ad.cpu().numpy()
        norm = {k: float(np.min(np.sum(np.abs(v) ** 2, axis=(1, 2)))) for k, v in res.items()}
        diff = float(np.max(np.abs(res["b"] - res["c"])))
        capi.set_option("ktime", 1)
        capi.kernel_times()
        ad.copy_(a0d)
        run_b(1)
        ms1, n1 = stage_slot()
        ad.copy_(a0d)
        run_b(11)
        ms11, n11 = stage_slot()
        ad.copy_(a0d)
        run_a(1)
        ma1, m1 = stage_slot()
        ad.copy_(a0d)
        run_a(11)
        ma11, m11 = stage_slot()
        capi.set_option("ktime", 0)
        med = {k: statistics.median(v) for k, v in t.items()}
        r = {"nscan": nscan}
        for k, name in (("a", "lawson"), ("b", "static"), ("c", "split")):
            r[name + "_ms_per_step"] = [round(1e3 * x / nsteps, 4) for x in t[k]]
            r[name + "_median"] = round(1e3 * med[k] / nsteps, 4)
        r.update({"b_over_a": round(med["b"] / med["a"], 3), "b_minus_a_us_per_step": round(1e6 * (med["b"] - med["a"]) / nsteps, 2),
                  "c_over_b": round(med["c"] / med["b"], 3), "stage_slot_launches_11_steps": n11,
                  "static_stage_us_per_launch": round(1e3 * (ms11 - ms1) / (n11 - n1), 2),
                  "lawson_stage_us_per_launch": round(1e3 * (ma11 - ma1) / (m11 - m1), 2),
                  "max_abs_diff_b_c": diff, "min_norm": norm, "max_err_static": float(np.max(err["b"]))})
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: (a) lawson %s ms/step (median %.4f), (b) static %s ms/step (median %.4f), (c) split %s ms/step "
                     "(median %.4f); (b)/(a) = %.3f, (b)-(a) = %.2f us/step, (c)/(b) = %.3f; stage slot under events: %.2f us per stage "
                     "launch of (b), %.2f of (a), %d launches of (b) in 11 steps; smallest norm left %.4f (a), %.4f (b), %.4f (c); "
                     "max|a_(b) - a_(c)| %.3g; err of (b) %.3g"
                     % (nscan, " ".join("%.4f" % x for x in r["lawson_ms_per_step"]), r["lawson_median"],
                        " ".join("%.4f" % x for x in r["static_ms_per_step"]), r["static_median"],
                        " ".join("%.4f" % x for x in r["split_ms_per_step"]), r["split_median"], r["b_over_a"], r["b_minus_a_us_per_step"],
                        r["c_over_b"], r["static_stage_us_per_launch"], r["lawson_stage_us_per_launch"], n11, norm["a"], norm["b"],
                        norm["c"], diff, r["max_err_static"]))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_static_rate.py: bspatom_tdse_static_dev (32 absorbers) against bspatom_tdse_lawson_dev and against single-step "
                "calls with torch propagators, alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
