#!/usr/bin/env python3
"""tdse_split_rate.py -- the rate of bspatom_tdse_split_dev (csrc/tdse_split.hip) in one process on one GPU, beside the unsplit call on
the same workload IN THE SAME RUN.  Hydrogen, linear grid, k = 9, channels l = 0.. at m = 0 coupled by F(t) z (the unsplit calls:
host.stark_system on the band of r; the split call: host.split_angular and the same band), the absorber cap_profile(r, 0.75 rb, 1e-3) on
every channel, packets 1s with each scan its own peak field, a sin^2 pulse, dt = 0.05, no rows, no snapshots.

  (1) tools/tdse_spline_rate.py's workload: four channels, nfun = 1024 and 4096, 64 packets x 32 steps; beside bspatom_tdse_spline_dev;
  (2) tools/tdse_spline_wide_rate.py's first: eight channels, nfun = 1024, as many packets as the wide call has work slots, 8 steps;
      beside bspatom_tdse_spline_wide_dev;
  (3) its second: ONE packet of sixteen channels, nfun = 1024, 8 steps; beside bspatom_tdse_spline_wide_dev;
  (4) ONE packet of 64 channels at nfun = 4096, 8 steps: half-width 575 for a coupled matrix, which no other call can run.

One untimed run of each route, then REPS repetitions alternating between the two.  Wall time between synchronised points; medians, and
(max - min) / median as the spread.  Every repetition restarts from the same packets and must return the same bits.  Beside the times:
the largest difference between the two routes' final packets at that dt -- two second-order approximations of one equation, O(dt^2)
apart -- and the norm left.  Not measured: hardware counters; any workload with rows or snapshots.  Writes a text report (default
profiles/r24_tdse_split.txt) and prints one JSON line.

    timeout -k 10 600 python tools/tdse_split_rate.py [--out FILE] [--only 1,2,3,4]
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

K, DT, REPS = 9, 0.05, 5
STAGE_BYTES = 2048 << 20                   # the scratch bound of the resolvent calls (resolvent_stage_mb's default)
DEV = "cuda:0"
spread = lambda v: (max(v) - min(v)) / statistics.median(v)
ms = lambda v: " ".join("%.3f" % (1e3 * x) for x in v)
put = lambda v: torch.from_numpy(np.array(v, order="C")).to(DEV)
bits = lambda t: t.cpu().numpy().view(np.uint64)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def wide_slots(nch, n):
    """tools/tdse_spline_wide_rate.py's packet count: the work slots of a wide call with one right-hand side"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, min(cus, STAGE_BYTES // (16 * nch * n * (3 * (nch * K - 1) + 2))))


def workload(name, nch, n, nscan, nsteps, other):
    """times of the split call and of `other` (None, "tdse_spline_dev" or "tdse_spline_wide_dev") on one workload: (dict, text line)"""
    rb = 0.25 * n
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=nch - 1, n0_ini=1, l_ini=0, zatom=1.0))
    E, info = prob.solve(0, 1)
    assert np.all(info == 0)
    v1s = prob.eigvecs(0, 1, 1)[0]
    prob.assemble(0, nch)                                              # the bands of every channel, for both routes
    chans = [(l, 0) for l in range(nch)]
    G = np.ascontiguousarray(prob.dipole_bands()[0])
    WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
    c0 = np.ascontiguousarray(np.broadcast_to(host.spline_packet(prob, chans, 0, v1s), (nscan, nch, n)))
    tm = host.spline_midpoints(0.0, DT, nsteps)
    F = np.linspace(0.01, 0.1, nscan)[None, :] * (np.sin(np.pi * tm / (nsteps * DT)) ** 2)[:, None]
    Q, lam = host.split_angular(chans)
    l = np.arange(nch, dtype=np.int32)
    c0d, Gd, Wd, fd = put(c0), put(G), put(WB), put(F.astype(np.complex128))
    cs, cu = torch.empty_like(c0d), torch.empty_like(c0d)

    def run_split():
        cs.copy_(c0d)
        return prob.tdse_split_dev(l, nscan, nsteps, DT, cs.data_ptr(), G_ptr=Gd.data_ptr(), Q=Q, lam=lam, f_ptr=fd.data_ptr(), nabs=1,
                                   W_ptr=Wd.data_ptr())

    runs = [("split", run_split)]
    if other:
        couplings, a1 = host.stark_system(chans, 1.0)
        coefd = put(host.spline_coefficients((couplings, a1), F))

        def run_other():
            cu.copy_(c0d)
            return getattr(prob, other)(l, nscan, nsteps, DT, cu.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(),
                                        coef_ptr=coefd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr())
        runs.append(("other", run_other))
    first = {}
    for key, run in runs:                                              # untimed: first launches
        assert np.all(run() == 0), key
        first[key] = bits(cs if key == "split" else cu)
    t = {key: [] for key, _ in runs}
    for _ in range(REPS):
        for key, run in runs:
            t[key].append(wall(run)[0])
    for key, _ in runs:                                                # the same bits after every repetition
        assert np.array_equal(bits(cs if key == "split" else cu), first[key]), key
    c_split = cs.cpu().numpy()
    norm = prob.tdse_split(l, c_split, DT, 0, obs_every=1)[2][0].sum(-1)
    med = {key: statistics.median(v) for key, v in t.items()}
    r = {"channels": nch, "nfun": n, "packets": nscan, "steps": nsteps, "systems_per_substep": nscan * nch,
         "split_ms": [round(1e3 * x, 3) for x in t["split"]], "split_median_ms": round(1e3 * med["split"], 3),
         "split_relative_spread": round(spread(t["split"]), 4), "split_ms_per_step": round(1e3 * med["split"] / nsteps, 4),
         "norm_after_run_first_last": [float(norm[0]), float(norm[-1])]}
    line = ("%s: l = 0..%d, nfun = %d, %d packets x %d steps (%d one-wave systems per substep): tdse_split_dev: %s ms (median %.3f, (max - min) / "
            "median = %.1f %%; %.3f ms per step)" % (name, nch - 1, n, nscan, nsteps, nscan * nch, ms(t["split"]), 1e3 * med["split"],
                                                   100 * spread(t["split"]), 1e3 * med["split"] / nsteps))
    if other:
        ratios = [p / q for p, q in zip(t["other"], t["split"])]
        diff = float(np.max(np.abs(c_split - cu.cpu().numpy())))
        r.update({"other": other, "other_ms": [round(1e3 * x, 3) for x in t["other"]], "other_median_ms": round(1e3 * med["other"], 3),
                  "other_relative_spread": round(spread(t["other"]), 4), "other_ms_per_step": round(1e3 * med["other"] / nsteps, 4),
                  "other_over_split": round(med["other"] / med["split"], 3), "other_over_split_range": [round(min(ratios), 3), round(max(ratios), 3)],
                  "largest_difference_of_final_packets": diff})
        verdict = "the split call is faster" if med["other"] > med["split"] else "the split call is NOT faster here"
        line += ("; %s (half-width %d): %s ms (median %.3f, %.1f %%; %.3f ms per step); unsplit / split = %.3f [%.3f .. %.3f]: %s; largest "
                 "difference between the two routes' final packets at dt = %g: %.3e" % (other, nch * K - 1, ms(t["other"]), 1e3 * med["other"],
                 100 * spread(t["other"]), 1e3 * med["other"] / nsteps, r["other_over_split"], min(ratios), max(ratios), verdict, DT, diff))
    else:
        line += "; no other call runs it (a coupled matrix would have half-width %d)" % (nch * K - 1)
    line += "; norm left after the run: %.6f (weakest field) .. %.6f (strongest)" % (norm[0], norm[-1])
    prob.close()
    torch.cuda.empty_cache()
    return r, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_tdse_split.txt"))
    ap.add_argument("--only", default="1,2,3,4")
    args = ap.parse_args()
    only = [int(s) for s in args.only.split(",")]
    jobs = []
    if 1 in only:
        jobs += [("(1) nfun = 1024", 4, 1024, 64, 32, "tdse_spline_dev"), ("(1) nfun = 4096", 4, 4096, 64, 32, "tdse_spline_dev")]
    if 2 in only:
        jobs += [("(2)", 8, 1024, wide_slots(8, 1024), 8, "tdse_spline_wide_dev")]
    if 3 in only:
        jobs += [("(3)", 16, 1024, 1, 8, "tdse_spline_wide_dev")]
    if 4 in only:
        jobs += [("(4)", 64, 4096, 1, 8, None)]
    out = {"workload": "channels l = 0.. at m = 0 coupled by F(t) z, k = %d, dt = %g, absorber on, no rows; %d repetitions, alternating" % (K, DT, REPS)}
    lines = []
    for job in jobs:
        r, line = workload(*job)
        out[job[0]] = r
        lines.append(line)
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_split_rate.py: bspatom_tdse_split_dev beside bspatom_tdse_spline_dev / bspatom_tdse_spline_wide_dev on the same workload in "
                "the same run, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
        f.write("Not measured: hardware counters; any workload with rows or snapshots.\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
