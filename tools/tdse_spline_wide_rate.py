#!/usr/bin/env python3
"""tdse_spline_wide_rate.py -- the rate of bspatom_tdse_spline_wide_dev (csrc/tdse_spline_wide.hip) in one process on one GPU, against
the same factorisations without the time stepping and against the route there was; tools/tdse_spline_rate.py's method.  Workload:
hydrogen, linear grid, k = 9, nfun = 1024; eight channels l = 0..7 (half-width 71, order 8192) coupled by F(t) z (host.stark_system on
the band of r), the absorber cap_profile(r, 0.75 rb, 1e-3) on every channel; as many packets (1s, each scan its own peak field) as
bspatom_resolvent_coupled_wide gets work slots for this shape -- one resident workgroup per CU within the scratch bound --, 8 steps
dt = 0.05 of a sin^2 pulse.

  (a) Problem.tdse_spline_wide_dev: the packets x 8 steps in one call, no rows, no snapshots;
  (b) the same number of matrices, packets * 8, each with its step's coefficients at z = 2i/dt, through
      Problem.resolvent_coupled_wide_dev with nrhs = 1 and X only, under resolvent_slots = packets: the same assembly, factorisation
      and solve on the same number of resident workgroups, WITHOUT the dependence of a step on the step before.  (a)/(b) is what a
      step adds to a factorisation (b = S c, the update, the barriers);
  (c) the route there was, on NSTEPS_C steps, scaled to 8: per step and scan host.band_apply on the packet, one
      Problem.resolvent_coupled_wide call with nmat = 1 (host arrays), the update in NumPy.
  second line: ONE packet of sixteen channels l = 0..15 (half-width 143, order 16384), 8 steps: time per step (one workgroup, one CU).

One untimed run of each, then REPS repetitions of (a) and (b) alternating and REPS_C of (c).  Wall time between synchronised points;
medians, and (max - min) / median as the spread.  (a) restarts from the same packets every repetition and must return the same bits;
its first NSTEPS_C steps must have the bits of (c) (guarantee S3).  Not measured: hardware counters, and any workload with rows or
snapshots.  Writes a text report (default profiles/r23_tdse_spline_wide.txt) and prints one JSON line.

    timeout -k 10 600 python tools/tdse_spline_wide_rate.py [--out FILE] [--no-second]
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

NSTEPS, K, NFUN, DT, REPS, REPS_C, NSTEPS_C = 8, 9, 1024, 0.05, 5, 3, 2
STAGE_BYTES = 2048 << 20                   # the scratch bound of the resolvent calls (resolvent_stage_mb's default)
DEV = "cuda:0"


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def slots_of(nch, n):
    """the work slots of a wide call with one right-hand side: one resident workgroup per CU, within the scratch bound"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, min(cus, STAGE_BYTES // (16 * nch * n * (3 * (nch * K - 1) + 2))))


def setup(nch, nscan):
    n, rb = NFUN, 0.25 * NFUN
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=nch - 1, n0_ini=1, l_ini=0, zatom=1.0))
    E, info = prob.solve(0, nch)
    assert np.all(info == 0)
    chans = [(l, 0) for l in range(nch)]
    G = np.ascontiguousarray(prob.dipole_bands()[0])
    WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
    c0 = np.ascontiguousarray(np.broadcast_to(host.spline_packet(prob, chans, 0, prob.eigvecs(0, 1, 1)[0]), (nscan, nch, n)))
    couplings, a1 = host.stark_system(chans, 1.0)
    tm = host.spline_midpoints(0.0, DT, NSTEPS)
    F = np.linspace(0.01, 0.1, nscan)[None, :] * (np.sin(np.pi * tm / (NSTEPS * DT)) ** 2)[:, None]
    coef = host.spline_coefficients((couplings, a1), F)                # (NSTEPS, nscan, ncoup, 1)
    return prob, G, WB, c0, couplings, coef, np.arange(nch, dtype=np.int32)


spread = lambda v: (max(v) - min(v)) / statistics.median(v)
ms = lambda v: " ".join("%.3f" % (1e3 * x) for x in v)
put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def first(lines, out):
    nch = 8
    n, nscan = NFUN, slots_of(nch, NFUN)
    prob, G, WB, c0, couplings, coef, l = setup(nch, nscan)
    c0d, Gd, Wd, coefd = put(c0), put(G), put(WB), put(coef)
    cd = torch.empty_like(c0d)
    Xd = torch.zeros((nscan * NSTEPS, 1, nch, n), dtype=torch.complex128, device=DEV)
    z = np.full((nscan * NSTEPS, nch), 2j / DT)
    a_b = coef.reshape(nscan * NSTEPS, len(couplings), 1)

    def run_a(nsteps=NSTEPS):
        cd.copy_(c0d)
        return prob.tdse_spline_wide_dev(l, nscan, nsteps, DT, cd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(),
                                         coef_ptr=coefd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr())

    def run_b():
        capi.set_option("resolvent_slots", nscan)
        try:
            return prob.resolvent_coupled_wide_dev(l, z, 1, c0d.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a_b, nabs=1,
                                                   W_ptr=Wd.data_ptr(), X_ptr=Xd.data_ptr())
        finally:
            capi.set_option("resolvent_slots", 0)

    assert np.all(run_a() == 0)                                        # untimed: first launches
    c_first = cd.cpu().numpy()
    assert np.all(run_b() == 0)
    t = {"a": [], "b": [], "c": []}
    for _ in range(REPS):
        for key, run in (("a", run_a), ("b", run_b)):
            t[key].append(wall(run)[0])
    assert np.array_equal(cd.cpu().numpy().view(np.uint64), c_first.view(np.uint64))   # the same bits after every repetition
    SBf = host.band_symmetric(prob.assemble(0, nch)[0])
    g = 4.0 / DT

    def run_c():
        c = np.array(c0)
        for s in range(NSTEPS_C):
            for q in range(nscan):
                b = host.band_apply(SBf, c[q].real) + 1j * host.band_apply(SBf, c[q].imag)
                x = prob.resolvent_coupled_wide(l, 2j / DT, b, couplings=couplings, G=G, a=coef[s, q], W=WB)[0][0, 0]
                c[q] = (g * x.imag - c[q].real) + 1j * (-(g * x.real) - c[q].imag)
        return c

    run_c()                                                            # untimed
    for _ in range(REPS_C):
        tc, cc = wall(run_c)
        t["c"].append(tc * NSTEPS / NSTEPS_C)
    run_a(NSTEPS_C)                                                    # the first NSTEPS_C steps of (a) are (c) bit for bit (S3)
    assert np.array_equal(cd.cpu().numpy().view(np.uint64), np.ascontiguousarray(cc).view(np.uint64))
    norm = prob.tdse_spline_wide(l, c_first, DT, 0, obs_every=1)[2][0].sum(-1)
    med = {k_: statistics.median(v) for k_, v in t.items()}
    ratio = lambda x, y: [p / q for p, q in zip(t[x], t[y])]
    r = {"nfun": n, "order": nch * n, "half_width": nch * K - 1, "packets": nscan, "steps": NSTEPS, "matrices": nscan * NSTEPS}
    for key, name in (("a", "spline_wide"), ("b", "coupled_wide_same_slots"), ("c", "host_route_for_8_steps")):
        r[name + "_ms"] = [round(1e3 * x, 3) for x in t[key]]
        r[name + "_median_ms"] = round(1e3 * med[key], 3)
        r[name + "_relative_spread"] = round(spread(t[key]), 4)
    r["a_over_b"] = round(med["a"] / med["b"], 3)
    r["a_over_b_range"] = [round(min(ratio("a", "b")), 3), round(max(ratio("a", "b")), 3)]
    r["c_over_a"] = round(med["c"] / med["a"], 1)
    r["ms_per_step"] = round(1e3 * med["a"] / NSTEPS, 3)
    r["norm_after_run_first_last"] = [float(norm[0]), float(norm[-1])]
    out["l0_7"] = r
    lines.append("l = 0..7, nfun = %d (order %d, half-width %d), %d packets = work slots x %d steps: (a) tdse_spline_wide_dev: %s ms (median %.3f, "
                 "(max - min) / median = %.1f %%; %.2f ms per step); (b) resolvent_coupled_wide_dev, %d independent matrices under resolvent_slots "
                 "= %d, X only: %s ms (median %.3f, %.1f %%); (c) band_apply + resolvent_coupled_wide(nmat = 1) + update per step and scan on "
                 "the host, %d steps timed, for %d: %s ms (median %.1f, %.1f %%); (a)/(b) = %.3f [%.3f .. %.3f]; (c)/(a) = %.1f; the first %d "
                 "steps of (a) have the bits of (c); norm left after the run: %.6f (weakest field) .. %.6f (strongest)"
                 % (n, nch * n, nch * K - 1, nscan, NSTEPS, ms(t["a"]), 1e3 * med["a"], 100 * spread(t["a"]), r["ms_per_step"], nscan * NSTEPS, nscan,
                    ms(t["b"]), 1e3 * med["b"], 100 * spread(t["b"]), NSTEPS_C, NSTEPS, " ".join("%.1f" % (1e3 * x) for x in t["c"]), 1e3 * med["c"],
                    100 * spread(t["c"]), r["a_over_b"], *r["a_over_b_range"], r["c_over_a"], NSTEPS_C, norm[0], norm[-1]))
    prob.close()


def second(lines, out):
    nch = 16
    prob, G, WB, c0, couplings, coef, l = setup(nch, 1)
    c0d, Gd, Wd, coefd = put(c0), put(G), put(WB), put(coef)
    cd = torch.empty_like(c0d)

    def run():
        cd.copy_(c0d)
        return prob.tdse_spline_wide_dev(l, 1, NSTEPS, DT, cd.data_ptr(), couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), coef_ptr=coefd.data_ptr(),
                                         nabs=1, W_ptr=Wd.data_ptr())

    assert np.all(run() == 0)
    c_first = cd.cpu().numpy()
    t = [wall(run)[0] for _ in range(REPS)]
    assert np.array_equal(cd.cpu().numpy().view(np.uint64), c_first.view(np.uint64))
    med = statistics.median(t)
    out["l0_15"] = {"nfun": NFUN, "order": nch * NFUN, "half_width": nch * K - 1, "packets": 1, "steps": NSTEPS, "spline_wide_ms": [round(1e3 * x, 3) for x in t],
                    "spline_wide_median_ms": round(1e3 * med, 3), "spline_wide_relative_spread": round(spread(t), 4), "ms_per_step": round(1e3 * med / NSTEPS, 3)}
    lines.append("l = 0..15, nfun = %d (order %d, half-width %d), ONE packet x %d steps (one workgroup): tdse_spline_wide_dev: %s ms (median %.3f, "
                 "(max - min) / median = %.1f %%): %.2f ms per step" % (NFUN, nch * NFUN, nch * K - 1, NSTEPS, ms(t), 1e3 * med, 100 * spread(t), 1e3 * med / NSTEPS))
    prob.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_tdse_spline_wide.txt"))
    ap.add_argument("--no-second", action="store_true")
    args = ap.parse_args()
    out = {"workload": "packets x %d steps dt = %g, channels l = 0.. coupled by F(t) z, k = %d, nfun = %d, absorber on, no rows" % (NSTEPS, DT, K, NFUN)}
    lines = []
    first(lines, out)
    torch.cuda.empty_cache()
    if not args.no_second:
        second(lines, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_spline_wide_rate.py: bspatom_tdse_spline_wide_dev against the same matrices through bspatom_resolvent_coupled_wide_dev "
                "on the same work slots and against the host route there was, one MI355X; %d repetitions, alternating\n" % REPS)
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
        f.write("Not measured: hardware counters; any workload with rows or snapshots.\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
