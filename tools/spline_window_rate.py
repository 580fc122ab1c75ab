#!/usr/bin/env python3
"""spline_window_rate.py -- the rate of bspatom_spline_window_dev (csrc/spline_window.hip) in one process on one GPU, beside the
route there was for a photoelectron spectrum and beside itself without the shared factorisations, IN THE SAME RUN.  Workload: the
final packets of tools/tdse_split_rate.py's sixteen-channel workload -- hydrogen, linear grid, k = 9, channels l = 0 .. 15 at m = 0
coupled by F(t) z, 8 split steps from 1s, here WITHOUT the absorber (the window needs a Hermitian H) --, nscan = 4 packets with
their own peak fields, nfun = 1024 and 4096; the window of order m = 2 and width 0.05 at ne = 256 energies from -0.6 to 2.0.

  (a) Problem.spline_window_dev: one call, 256 x 16 items of 4 right-hand sides: 8192 factorisations, 32768 solves;
  (b) the route there was: one Problem.resolvent_chain_dev call per (scan, channel) -- 64 calls of 256 chains of 2 stages with S as
      the operator between the stages and X returned (16 * ne * nfun bytes per packet) --, then the contraction Re x^H S x in torch.
      The first right-hand side S c is formed once, outside the timed region (in (b)'s favour).  32768 factorisations and solves;
  (c) (a) with window_rhs = 1: a factorisation per packet, 32768 of them in one launch: what sharing a factorisation is worth.

One untimed run of each, then REPS repetitions of (a), (b), (c) alternating.  Wall time between synchronised points; medians, and
(max - min) / median as the spread.  (a) and (c) must return the same bits, in every repetition; (b)'s x are (a)'s (C1 - C6 of
bspatom.h), its norms are summed in torch's order: the largest relative difference is reported.  The gate: (a) takes no longer
than (b) x (1 + the larger of the two spreads); the ratios (b)/(a) and (c)/(a) are reported, not gated.  Not measured: hardware
counters.  Writes a text report (default profiles/r27_spline_window.txt), prints one JSON line, and exits 1 if the gate fails.

    timeout -k 10 900 python tools/spline_window_rate.py [--out FILE] [--sizes 1024,4096]
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
NCH, NSCAN, NSTEPS, NE, M, GAMMA = 16, 4, 8, 256, 2, 0.05
DEV = "cuda:0"
spread = lambda v: (max(v) - min(v)) / statistics.median(v)
ms = lambda v: " ".join("%.3f" % (1e3 * x) for x in v)
put = lambda v: torch.from_numpy(np.array(v, order="C")).to(DEV)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def band_apply_torch(SF, X):
    """S x for the rows of X (m, n) complex on the device; SF (2k-1, n) the full band"""
    b, n = (SF.shape[0] - 1) // 2, SF.shape[1]
    Y = torch.zeros_like(X)
    for d in range(-b, b + 1):
        lo, hi = max(0, -d), min(n, n - d)
        Y[:, lo:hi] += SF[d + b, lo:hi] * X[:, lo + d:hi + d]
    return Y


def workload(n):
    rb = 0.25 * n
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=NCH - 1, n0_ini=1, l_ini=0, zatom=1.0))
    E, info = prob.solve(0, 1)
    assert np.all(info == 0)
    v1s = prob.eigvecs(0, 1, 1)[0]
    SB, HB = prob.assemble(0, NCH)
    chans = [(l, 0) for l in range(NCH)]
    tm = host.spline_midpoints(0.0, DT, NSTEPS)
    F = np.linspace(0.01, 0.1, NSCAN)[None, :] * (np.sin(np.pi * tm / (NSTEPS * DT)) ** 2)[:, None]
    c0 = np.ascontiguousarray(np.broadcast_to(host.spline_packet(prob, chans, 0, v1s), (NSCAN, NCH, n)))
    c, sinfo = host.split_propagate(prob, np.arange(NCH), c0, DT, host.split_angular(chans), F)
    assert np.all(sinfo == 0)
    l = np.arange(NCH, dtype=np.int32)
    Egrid = np.linspace(-0.6, 2.0, NE)
    z = host.window_shifts(Egrid, GAMMA, M)
    SF = host.band_symmetric(SB)
    cd, SFd = put(c), put(SF)
    Na = torch.zeros((NSCAN, NCH, NE), dtype=torch.float64, device=DEV)
    Nc = torch.zeros_like(Na)
    Nb = torch.zeros_like(Na)
    Bd = band_apply_torch(SFd, cd.reshape(NSCAN * NCH, n)).reshape(NSCAN, NCH, n).contiguous()     # S c, outside the timed region
    Xd = torch.zeros((NE, 1, n), dtype=torch.complex128, device=DEV)
    lch = [np.full((NE, M), ch, dtype=np.int32) for ch in range(NCH)]
    ones = np.ones((NE, M - 1, 1))

    def run_a():
        return prob.spline_window_dev(l, NSCAN, cd.data_ptr(), z, Na.data_ptr())

    def run_c():
        capi.set_option("window_rhs", 1)
        try:
            return prob.spline_window_dev(l, NSCAN, cd.data_ptr(), z, Nc.data_ptr())
        finally:
            capi.set_option("window_rhs", 0)

    def run_b():
        bad = 0
        for q in range(NSCAN):
            for ch in range(NCH):
                bad += int(np.any(prob.resolvent_chain_dev(lch[ch], z, 1, Bd[q, ch].data_ptr(), nop=1, G_ptr=SFd.data_ptr(), a=ones,
                                                           X_ptr=Xd.data_ptr()) != 0))
                X = Xd[:, 0]
                Y = band_apply_torch(SFd, X)
                Nb[q, ch] = torch.sum(X.real * Y.real + X.imag * Y.imag, dim=1)
        return bad

    assert np.all(run_a() == 0) and np.all(run_c() == 0) and run_b() == 0    # untimed: first launches
    first = Na.cpu().numpy().copy()
    assert np.array_equal(first.view(np.uint64), Nc.cpu().numpy().view(np.uint64)), "window_rhs = 1 changed the bits"
    t = {"a": [], "b": [], "c": []}
    for _ in range(REPS):
        for key, run in (("a", run_a), ("b", run_b), ("c", run_c)):
            t[key].append(wall(run)[0])
    for v in (Na, Nc):                                                 # the same bits after every repetition
        assert np.array_equal(v.cpu().numpy().view(np.uint64), first.view(np.uint64))
    rel = float(np.max(np.abs(Nb.cpu().numpy() - first) / first))
    med = {k_: statistics.median(v) for k_, v in t.items()}
    ba = [x / y for x, y in zip(t["b"], t["a"])]
    ca = [x / y for x, y in zip(t["c"], t["a"])]
    larger = max(spread(t["a"]), spread(t["b"]))
    ok = med["a"] <= med["b"] * (1.0 + larger)
    P = GAMMA ** (2 * M) * first
    r = {"nfun": n, "window_ms": [round(1e3 * x, 3) for x in t["a"]], "chain_route_ms": [round(1e3 * x, 3) for x in t["b"]],
         "window_rhs1_ms": [round(1e3 * x, 3) for x in t["c"]], "window_median_ms": round(1e3 * med["a"], 3),
         "chain_route_median_ms": round(1e3 * med["b"], 3), "window_rhs1_median_ms": round(1e3 * med["c"], 3),
         "window_relative_spread": round(spread(t["a"]), 4), "chain_route_relative_spread": round(spread(t["b"]), 4),
         "window_rhs1_relative_spread": round(spread(t["c"]), 4),
         "chain_route_over_window": round(med["b"] / med["a"], 3), "chain_route_over_window_range": [round(min(ba), 3), round(max(ba), 3)],
         "rhs1_over_window": round(med["c"] / med["a"], 3), "rhs1_over_window_range": [round(min(ca), 3), round(max(ca), 3)],
         "gate_window_no_slower_than_chain_route": bool(ok), "max_rel_diff_chain_route": rel,
         "P_sum_over_channels_first_last_energy": [float(P[0].sum(0)[0]), float(P[0].sum(0)[-1])]}
    line = ("nfun = %d: (a) spline_window_dev: %s ms (median %.3f, (max - min) / median = %.1f %%); (b) %d resolvent_chain_dev calls with X, then "
            "torch: %s ms (median %.3f, %.1f %%); (c) spline_window_dev with window_rhs = 1: %s ms (median %.3f, %.1f %%); (b)/(a) = %.3f "
            "[%.3f .. %.3f]; (c)/(a) = %.3f [%.3f .. %.3f]; gate (a) <= (b) x (1 + %.3f): %s; (a) and (c): the same bits; largest relative "
            "difference of (b)'s norms: %.2e"
            % (n, ms(t["a"]), 1e3 * med["a"], 100 * spread(t["a"]), NSCAN * NCH, ms(t["b"]), 1e3 * med["b"], 100 * spread(t["b"]), ms(t["c"]),
               1e3 * med["c"], 100 * spread(t["c"]), r["chain_route_over_window"], min(ba), max(ba), r["rhs1_over_window"], min(ca), max(ca),
               larger, "holds" if ok else "FAILS", rel))
    prob.close()
    torch.cuda.empty_cache()
    return r, line, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_spline_window.txt"))
    ap.add_argument("--sizes", default="1024,4096")
    args = ap.parse_args()
    out = {"workload": "final packets of %d split steps, l = 0..%d, k = %d, no absorber, nscan = %d; window m = %d, gamma = %g, ne = %d; %d "
                       "repetitions, alternating" % (NSTEPS, NCH - 1, K, NSCAN, M, GAMMA, NE, REPS)}
    lines, good = [], True
    for n in [int(s) for s in args.sizes.split(",")]:
        r, line, ok = workload(n)
        out["nfun_%d" % n] = r
        lines.append(line)
        good = good and ok
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/spline_window_rate.py: bspatom_spline_window_dev beside the chain route and beside window_rhs = 1 in the same run, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
        f.write("Not measured: hardware counters.\n")
    print(json.dumps(out))
    sys.exit(0 if good else 1)


if __name__ == "__main__":
    main()
