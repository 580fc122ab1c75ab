#!/usr/bin/env python3
"""resolvent_wide_rate.py -- the rate of bspatom_resolvent_coupled_wide_dev (csrc/resolvent_wide.hip) in one process on one GPU.
Five repetitions, alternating between the things compared; medians with (max - min) / median.

  (a) resolvent_coupled_rate.py's own workload (64 energies, l = 0..3 coupled by a static field, k = 9, absorber, nrhs = 1, R only,
      nfun = 1024 and 4096: half-width 35) through the wide call and through bspatom_resolvent_coupled_dev, the baseline;
  (b) a 14-block Floquet batch (nphot = 3, l = 0..3, nfun = 1024: order 14336, half-width 125, 64 quasi-energies) against
      torch.linalg.solve on the dense complex128 matrices of the same systems, a few timed and scaled to 64; both backward errors;
  (c) scaling in the number of blocks: nch = 8, 12, 16, 24, 28 channels l = 0..nch-1 in a static field at nfun = 1024, k = 9, as many
      matrices as work slots: ms per matrix beside the model 8 N bw (2 bw) real flop, and the fraction of the fp64 matrix peak of
      the CUs in use (one workgroup per matrix: one CU each).

Writes a text report (default profiles/r21_resolvent_wide.txt; with --parts the chosen parts only) and prints one JSON line.

    timeout -k 10 1100 python tools/resolvent_wide_rate.py [--out FILE] [--parts a,b,c] [--sizes 1024,4096] [--blocks 8,12,16,24,28]
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

NE, K, F, REPS, NDENSE = 64, 9, 0.01, 5, 2
STAGE_BYTES = 2048 << 20                   # the default bound on a call's scratch ("resolvent_stage_mb")
PEAK_FP64_MATRIX = 78.6e12                 # MI355X, all CUs (public specification)
DEV = "cuda:0"


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


spread = lambda v: (max(v) - min(v)) / statistics.median(v)
ms = lambda v: " ".join("%.3f" % (1e3 * x) for x in v)


def slots_of(nch, n, nrhs=1):
    """the work slots of a wide call: one resident workgroup per CU, within the scratch bound (include/bspatom.h)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_slot = 16 * nch * n * (3 * (nch * K - 1) + 1 + nrhs)
    return max(1, min(cus, STAGE_BYTES // per_slot)), cus


def problem(n, nl):
    rb = 0.25 * n
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=nl - 1, n0_ini=1, l_ini=0, zatom=1.0))
    E, info = prob.solve(0, nl)
    assert np.all(info == 0)
    RB = prob.dipole_bands()
    c1s = prob.eigvecs(0, 1, 1)[0]
    WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
    return prob, E, np.ascontiguousarray(RB[0]), c1s, WB


def part_a(sizes, lines, out):
    nch = 4
    for n in sizes:
        prob, E, G, c1s, WB = problem(n, nch)
        b = np.zeros((nch, n), dtype=np.complex128)
        b[1] = host.band_apply(G, c1s[None])[0]
        couplings, a = host.stark_system([(l, 0) for l in range(nch)], F)
        zs = (E[0, 0] + np.linspace(0.55, 1.5, NE)).astype(np.complex128)
        l, z = np.arange(nch, dtype=np.int32), np.repeat(zs[:, None], nch, axis=1)
        bd, Wd, Gd = torch.from_numpy(b).to(DEV), torch.from_numpy(WB).to(DEV), torch.from_numpy(G).to(DEV)
        R = {key: torch.zeros((NE, 1, 1), dtype=torch.complex128, device=DEV) for key in ("wide", "old")}
        kw = dict(couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a, nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=bd.data_ptr())
        run = {"wide": lambda: prob.resolvent_coupled_wide_dev(l, z, 1, bd.data_ptr(), R_ptr=R["wide"].data_ptr(), **kw),
               "old": lambda: prob.resolvent_coupled_dev(l, z, 1, bd.data_ptr(), R_ptr=R["old"].data_ptr(), **kw)}
        for key in run:                                                # untimed: first launches
            assert np.all(run[key]() == 0)
        t = {"wide": [], "old": []}
        for _ in range(REPS):
            for key in ("wide", "old"):
                t[key].append(wall(run[key])[0])
        Rw, Ro = R["wide"].cpu().numpy().ravel(), R["old"].cpu().numpy().ravel()
        rel = float(np.max(np.abs(Rw - Ro) / np.abs(Ro)))
        ratio = [x / y for x, y in zip(t["wide"], t["old"])]
        med = {key: statistics.median(v) for key, v in t.items()}
        r = {"nfun": n, "order": nch * n, "half_width": nch * K - 1, "wide_ms": [round(1e3 * x, 3) for x in t["wide"]],
             "old_ms": [round(1e3 * x, 3) for x in t["old"]], "wide_median_ms": round(1e3 * med["wide"], 3),
             "old_median_ms": round(1e3 * med["old"], 3), "wide_spread": round(spread(t["wide"]), 4), "old_spread": round(spread(t["old"]), 4),
             "wide_over_old": round(med["wide"] / med["old"], 3), "wide_over_old_range": [round(min(ratio), 3), round(max(ratio), 3)],
             "max_rel_diff_R": rel}
        out["a_nfun_%d" % n] = r
        lines.append("(a) nfun = %d (order %d, half-width %d), %d matrices: wide %s ms (median %.3f, (max - min) / median = %.1f %%); "
                     "bspatom_resolvent_coupled_dev, the baseline: %s ms (median %.3f, %.1f %%); wide / baseline = %.3f [%.3f .. %.3f]; "
                     "max relative difference of R between the two: %.1e"
                     % (n, nch * n, nch * K - 1, NE, ms(t["wide"]), 1e3 * med["wide"], 100 * spread(t["wide"]), ms(t["old"]), 1e3 * med["old"],
                        100 * spread(t["old"]), r["wide_over_old"], min(ratio), max(ratio), rel))
        prob.close()
        del bd, Wd, Gd, R
        torch.cuda.empty_cache()


def part_b(lines, out):
    n, om, Ff = 1024, 0.2, 0.005
    prob, E, G, c1s, WB = problem(n, 4)
    blocks, zoff, couplings, a = host.floquet_system([(0, 0), (1, 0), (2, 0), (3, 0)], 3, om, Ff)
    nch = len(blocks)
    N = nch * n
    l = np.array([b_[0][0] for b_ in blocks], dtype=np.int32)
    b = np.zeros((nch, n), dtype=np.complex128)
    b[blocks.index(((1, 0), 1))] = host.band_apply(G, c1s[None])[0]
    zs = (E[0, 0] + np.linspace(0.55, 1.5, NE)).astype(np.complex128)
    z = zs[:, None] + zoff[None, :]
    bd, Wd, Gd = torch.from_numpy(b).to(DEV), torch.from_numpy(WB).to(DEV), torch.from_numpy(G).to(DEV)
    Rd = torch.zeros((NE, 1, 1), dtype=torch.complex128, device=DEV)
    kw = dict(couplings=couplings, nop=1, G_ptr=Gd.data_ptr(), a=a, nabs=1, W_ptr=Wd.data_ptr())
    run = lambda: prob.resolvent_coupled_wide_dev(l, z, 1, bd.data_ptr(), nproj=1, P_ptr=bd.data_ptr(), R_ptr=Rd.data_ptr(), **kw)
    assert np.all(run() == 0)
    R_w = Rd.cpu().numpy().ravel()
    Xd = torch.zeros((1, 1, nch, n), dtype=torch.complex128, device=DEV)
    prob.resolvent_coupled_wide_dev(l, z[0], 1, bd.data_ptr(), X_ptr=Xd.data_ptr(), **kw)
    # the dense matrices of the same systems, block by block: M(z) = A - sum_c z_c S_c
    SB, HB = prob.assemble(0, 4)
    A = torch.zeros((N, N), dtype=torch.complex128, device=DEV)
    S1 = torch.from_numpy(-host.coupled_dense(SB, 0.0 * HB, [0], [1.0], None, None, None)).to(DEV)
    for c in range(nch):
        A[c * n:(c + 1) * n, c * n:(c + 1) * n] = torch.from_numpy(host.coupled_dense(SB, HB, [int(l[c])], [0.0], None, None, None, W=WB)).to(DEV)
    Gdn = host._full_to_dense(G, np.float64)
    for p, (cr, cc, ctr) in enumerate(couplings):
        A[cr * n:(cr + 1) * n, cc * n:(cc + 1) * n] += torch.from_numpy(a[p] * (Gdn.T if ctr else Gdn)).to(DEV)
    bf = bd.reshape(-1, 1)

    def matrix(m):
        M = A.clone()
        for c in range(nch):
            M[c * n:(c + 1) * n, c * n:(c + 1) * n] -= complex(z[m, c]) * S1
        return M

    tw, td, R_d = [], [], np.zeros(NDENSE, dtype=np.complex128)
    M = matrix(0)
    x = torch.linalg.solve(M, bf)                                      # untimed
    scale = float(torch.max(torch.sum(torch.abs(M), dim=1)))
    omega = lambda v: float(torch.max(torch.abs(bf - M @ v)) / (scale * float(torch.max(torch.abs(v))) + float(torch.max(torch.abs(bf)))))
    om_w, om_d = omega(Xd.reshape(-1, 1)), omega(x)
    del M, x
    for _ in range(REPS):
        tw.append(wall(run)[0])
        tt = 0.0
        for m in range(NDENSE):
            M = matrix(m)
            dt, x = wall(lambda: torch.linalg.solve(M, bf))
            tt += dt
            R_d[m] = complex(torch.sum(bf * x))
            del M, x
        td.append(tt * NE / NDENSE)
    rel = float(np.max(np.abs(R_d - R_w[:NDENSE]) / np.abs(R_w[:NDENSE])))
    slots, cus = slots_of(nch, n)
    ratio = [x_ / statistics.median(tw) for x_ in td]
    r = {"order": N, "half_width": nch * K - 1, "slots": slots, "wide_ms": [round(1e3 * x_, 2) for x_ in tw],
         "dense_ms_for_64": [round(1e3 * x_, 1) for x_ in td], "wide_median_ms": round(1e3 * statistics.median(tw), 2),
         "dense_median_ms_for_64": round(1e3 * statistics.median(td), 1), "wide_spread": round(spread(tw), 4), "dense_spread": round(spread(td), 4),
         "dense_over_wide": round(statistics.median(td) / statistics.median(tw), 2), "dense_over_wide_range": [round(min(ratio), 2), round(max(ratio), 2)],
         "backward_error_wide": om_w, "backward_error_dense": om_d, "max_rel_diff_R": rel}
    out["b"] = r
    lines.append("(b) 14 Floquet blocks (nphot = 3, l = 0..3, omega = %g, F = %g, absorber on), nfun = %d: order %d, half-width %d, %d quasi-energies, "
                 "%d work slots: wide %s ms (median %.2f, (max - min) / median = %.1f %%); torch.linalg.solve, dense complex128, one matrix at a "
                 "time, %d timed, for 64: %s ms (median %.1f, %.1f %%); dense / wide = %.2f [%.2f .. %.2f]; backward error of the first system in "
                 "complex128: wide %.1e, dense %.1e; max relative difference of R: %.1e"
                 % (om, Ff, n, N, nch * K - 1, NE, slots, " ".join("%.2f" % (1e3 * x_) for x_ in tw), 1e3 * statistics.median(tw), 100 * spread(tw),
                    NDENSE, " ".join("%.1f" % (1e3 * x_) for x_ in td), 1e3 * statistics.median(td), 100 * spread(td), r["dense_over_wide"],
                    min(ratio), max(ratio), om_w, om_d, rel))
    prob.close()
    del A, S1, bd, Wd, Gd, Rd, Xd
    torch.cuda.empty_cache()


def part_c(nblocks, lines, out):
    n = 1024
    prob, E, G, c1s, WB = problem(n, max(nblocks))
    Wd, Gd = torch.from_numpy(WB).to(DEV), torch.from_numpy(G).to(DEV)
    setup, t = {}, {}
    for nch in nblocks:
        slots, cus = slots_of(nch, n)
        b = np.zeros((nch, n), dtype=np.complex128)
        b[1] = host.band_apply(G, c1s[None])[0]
        couplings, a = host.stark_system([(l, 0) for l in range(nch)], F)
        zs = (E[0, 0] + np.linspace(0.55, 1.5, slots)).astype(np.complex128)
        setup[nch] = dict(slots=slots, l=np.arange(nch, dtype=np.int32), z=np.repeat(zs[:, None], nch, axis=1), bd=torch.from_numpy(b).to(DEV),
                          Rd=torch.zeros((slots, 1, 1), dtype=torch.complex128, device=DEV), couplings=couplings, a=a)
        t[nch] = []

    def run(nch):
        s = setup[nch]
        return prob.resolvent_coupled_wide_dev(s["l"], s["z"], 1, s["bd"].data_ptr(), couplings=s["couplings"], nop=1, G_ptr=Gd.data_ptr(), a=s["a"],
                                               nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=s["bd"].data_ptr(), R_ptr=s["Rd"].data_ptr())
    for nch in nblocks:
        assert np.all(run(nch) == 0)                                   # untimed
    for _ in range(REPS):
        for nch in nblocks:
            t[nch].append(wall(lambda: run(nch))[0])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    base = None
    for nch in nblocks:
        N, bw, slots = nch * n, nch * K - 1, setup[nch]["slots"]
        med = statistics.median(t[nch])
        flop = 8.0 * N * bw * 2 * bw
        frac = flop / med / (PEAK_FP64_MATRIX / cus)
        base = base or (med, N * bw * bw)
        rel_model = (med / base[0]) / (N * bw * bw / base[1])
        out["c_nch_%d" % nch] = {"order": N, "half_width": bw, "matrices": slots, "ms": [round(1e3 * x_, 2) for x_ in t[nch]],
                                 "median_ms_per_matrix": round(1e3 * med, 2), "spread": round(spread(t[nch]), 4), "model_gflop": round(flop / 1e9, 2),
                                 "gflops_per_cu": round(flop / med / 1e9, 1), "fraction_of_fp64_matrix_peak_of_a_cu": round(frac, 4),
                                 "time_over_N_bw2_relative_to_first": round(rel_model, 3)}
        lines.append("(c) nch = %d (order %d, half-width %d), %d matrices = work slots, one CU each: %s ms (median %.2f ms per matrix, (max - min) / "
                     "median = %.1f %%); model 8 N bw (2 bw) = %.2f Gflop: %.1f Gflop/s per CU, %.2f %% of a CU's fp64 matrix peak (%.0f Gflop/s); "
                     "time / (N bw^2) relative to nch = %d: %.3f"
                     % (nch, N, bw, slots, " ".join("%.2f" % (1e3 * x_) for x_ in t[nch]), 1e3 * med, 100 * spread(t[nch]), flop / 1e9,
                        flop / med / 1e9, 100 * frac, PEAK_FP64_MATRIX / cus / 1e9, nblocks[0], rel_model))
    prob.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_resolvent_wide.txt"))
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--blocks", default="8,12,16,24,28")
    args = ap.parse_args()
    parts = args.parts.split(",")
    out, lines = {}, []
    if "a" in parts:
        part_a([int(s) for s in args.sizes.split(",")], lines, out)
    if "b" in parts:
        part_b(lines, out)
    if "c" in parts:
        part_c([int(s) for s in args.blocks.split(",")], lines, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/resolvent_wide_rate.py: bspatom_resolvent_coupled_wide_dev (csrc/resolvent_wide.hip), one MI355X; %d repetitions, "
                "alternating; times are wall times of whole calls\n" % REPS)
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
