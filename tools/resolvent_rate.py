#!/usr/bin/env python3
"""resolvent_rate.py -- the rate of bspatom_resolvent_dev (csrc/resolvent.hip) in one process on one GPU, against the only route there
was before: torch.linalg.solve on the dense complex128 matrices of the same batch.  Workload: hydrogen, linear grid, k = 9, nfun = 1024
and 4096; 256 energies z = E_1s + omega, omega in [0.55, 3], of channel l = 1 with the absorber cap_profile(r, 0.75 rb, 1e-3); one
right-hand side b = r |1s>, one projection p = b, R only (the photoabsorption workload of host.photoabsorption).

  (a) Problem.resolvent_dev: 256 matrices in one call (host arrays l, z, w uploaded, info downloaded, scratch allocated and freed inside);
  (b) torch.linalg.solve on the dense matrices, built on the GPU from the same bands BEFORE the clock starts, in chunks of at most
      `--dense-chunk` matrices (a chunk of 32 at nfun = 4096 is 8 GiB), then p^T x; the chunks' times are summed;
  (c) Problem.eigvecs_batch_dev, 256 vectors of the same channel: the cost of an invit_batch_kernel item (a real LU and two or three
      real solves), the yardstick the kernel was expected to cost a few times of.

One untimed run of each; then REPS repetitions of (a) and (c) alternating, then -- after bspatom_assemble, which hands out the bands and
ends the state of the solve -- REPS repetitions of (a) and (b) alternating; (a)'s median is over all 2 REPS.  Every time is wall time
between synchronised points.
Writes a text report (default profiles/r18_resolvent.txt) and prints one JSON line.

    timeout -k 10 600 python tools/resolvent_rate.py [--out FILE] [--sizes 1024,4096] [--dense-chunk 32]
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

NMAT, K, REPS = 256, 9, 5


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def dense_batch(SB, HB, WB, z):
    """(len(z), n, n) complex128 on the GPU: H - i W - z S from the bands (torch tensors on the device)"""
    k, n = SB.shape
    M = torch.zeros((z.numel(), n, n), dtype=torch.complex128, device=SB.device)
    for d in range(k):
        up = HB[d, :n - d] - z[:, None] * SB[d, :n - d]
        M.diagonal(offset=d, dim1=1, dim2=2).copy_(up - 1j * WB[k - 1 + d, :n - d])
        if d:
            M.diagonal(offset=-d, dim1=1, dim2=2).copy_(up - 1j * WB[k - 1 - d, d:])
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_resolvent.txt"))
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--dense-chunk", type=int, default=32)
    args = ap.parse_args()
    dev = "cuda:0"
    out, lines = {"workload": "%d energies of channel l = 1, k = %d, absorber on, nrhs = 1, nproj = 1, R only" % (NMAT, K)}, []
    for n in [int(s) for s in args.sizes.split(",")]:
        rb = 0.25 * n
        prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=1, n0_ini=1, l_ini=0, zatom=1.0))
        E, info = prob.solve(0, 2)
        assert np.all(info == 0)
        b = host.band_apply(prob.dipole_bands()[0], prob.eigvecs(0, 1, 1))[0].astype(np.complex128)
        WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
        z = (E[0, 0] + np.linspace(0.55, 3.0, NMAT)).astype(np.complex128)
        l = np.ones(NMAT, dtype=np.int32)
        bd, Wd = torch.from_numpy(b).to(dev), torch.from_numpy(WB).to(dev)
        Rd = torch.zeros((NMAT, 1, 1), dtype=torch.complex128, device=dev)
        Zd = torch.zeros((NMAT, n), dtype=torch.float64, device=dev)
        run_a = lambda: prob.resolvent_dev(l, z, 1, bd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr(), nproj=1, P_ptr=bd.data_ptr(), R_ptr=Rd.data_ptr())
        run_c = lambda: prob.eigvecs_batch_dev(1, 1, 1, NMAT, Zd.data_ptr())

        def dense_route():
            """sum over the chunks of the time of torch.linalg.solve + p^T x; the matrices are built outside the clock"""
            total, Rs = 0.0, []
            zt = torch.from_numpy(z).to(dev)
            for c0 in range(0, NMAT, args.dense_chunk):
                M = dense_batch(SBd, HBd, Wd, zt[c0:c0 + args.dense_chunk])
                dt_, r = wall(lambda: (torch.linalg.solve(M, bd[None, :, None].expand(M.shape[0], n, 1))[:, :, 0] * bd).sum(dim=1))
                total += dt_
                Rs.append(r)
                del M
            return total, torch.cat(Rs)

        info_a = run_a()                                               # untimed: first launches
        assert np.all(info_a == 0)
        run_c()
        R_a = Rd.cpu().numpy()[:, 0, 0]
        t = {"a": [], "c": []}
        for _ in range(REPS):
            for key, run in (("a", run_a), ("c", run_c)):
                t[key].append(wall(run)[0])
        # the dense route's operands are the problem's own bands (this ends the state of the solve, so it comes after (c))
        SBh, HBh = prob.assemble(0, 2)
        SBd, HBd = torch.from_numpy(SBh).to(dev), torch.from_numpy(HBh[1]).to(dev)
        dense_route()                                                  # untimed
        t["b"] = []
        R_b = None
        for _ in range(REPS):
            t["a"].append(wall(run_a)[0])                              # (a) again beside (b): the bands are the same after assemble
            dt_, R_b = dense_route()
            t["b"].append(dt_)
        R_b = R_b.cpu().numpy()
        assert np.array_equal(Rd.cpu().numpy()[:, 0, 0], R_a)          # after the solve and after assemble: the same bits
        med = {k_: statistics.median(v) for k_, v in t.items()}
        # the absorbing term of host.photoabsorption, 4 pi omega Im R(E_1s + omega) / (3 c) (R(E_1s - omega) is real up to the absorber's tail)
        sigma = 4.0 * np.pi * np.linspace(0.55, 3.0, NMAT) * R_a.imag / (3.0 * host.C_RESPONSE)
        r = {"nfun": n, "resolvent_ms": [round(1e3 * x, 3) for x in t["a"]], "dense_solve_ms": [round(1e3 * x, 3) for x in t["b"]],
             "eigvecs_batch_ms": [round(1e3 * x, 3) for x in t["c"]],
             "resolvent_median_ms": round(1e3 * med["a"], 3), "dense_median_ms": round(1e3 * med["b"], 3),
             "eigvecs_batch_median_ms": round(1e3 * med["c"], 3),
             "resolvent_us_per_matrix": round(1e6 * med["a"] / NMAT, 2), "dense_us_per_matrix": round(1e6 * med["b"] / NMAT, 2),
             "invit_us_per_item": round(1e6 * med["c"] / NMAT, 2),
             "dense_over_resolvent": round(med["b"] / med["a"], 2), "resolvent_over_invit": round(med["a"] / med["c"], 3),
             "max_rel_diff_R": float(np.max(np.abs(R_a - R_b) / np.abs(R_b))), "sigma_first_last": [float(sigma[0]), float(sigma[-1])]}
        out["nfun_%d" % n] = r
        lines.append("nfun = %d: (a) resolvent_dev %s ms (median %.3f, %.2f us per matrix); (b) torch.linalg.solve, dense, chunks of %d: %s ms "
                     "(median %.3f, %.2f us per matrix); (c) eigvecs_batch_dev, %d vectors: %s ms (median %.3f, %.2f us per item); "
                     "(b)/(a) = %.2f, (a)/(c) = %.3f; max |R_a - R_b| / |R_b| = %.3g; sigma(0.55) = %.6e, sigma(3.0) = %.6e"
                     % (n, " ".join("%.3f" % x for x in r["resolvent_ms"]), r["resolvent_median_ms"], r["resolvent_us_per_matrix"],
                        args.dense_chunk, " ".join("%.3f" % x for x in r["dense_solve_ms"]), r["dense_median_ms"], r["dense_us_per_matrix"],
                        NMAT, " ".join("%.3f" % x for x in r["eigvecs_batch_ms"]), r["eigvecs_batch_median_ms"], r["invit_us_per_item"],
                        r["dense_over_resolvent"], r["resolvent_over_invit"], r["max_rel_diff_R"], sigma[0], sigma[-1]))
        prob.close()
        del bd, Wd, Rd, Zd, SBd, HBd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/resolvent_rate.py: bspatom_resolvent_dev against torch.linalg.solve on the dense matrices and against "
                "bspatom_eigvecs_batch_dev, alternating, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
