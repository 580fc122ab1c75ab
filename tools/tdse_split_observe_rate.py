#!/usr/bin/env python3
"""tdse_split_observe_rate.py -- what the dipole and acceleration rows of bspatom_tdse_split_observe_dev (csrc/spline_expect.hip) cost along
a run, in one process on one GPU, on tools/tdse_split_rate.py's workloads: hydrogen, linear grid, k = 9, channels l = 0.. at m = 0
coupled by F(t) z, the absorber cap_profile(r, 0.75 rb, 1e-3) on every channel, packets 1s with each scan its own peak field, a sin^2
pulse, dt = 0.05.

  (1) four channels, nfun = 1024 and 4096, 64 packets x 32 steps;
  (2) ONE packet of 64 channels at nfun = 4096, 8 steps.

Three routes IN THE SAME RUN, nexp = 2 (host.split_expect_dipole and host.split_expect_accel), every step observed:
  (a) tdse_split_dev without rows: the run alone;
  (b) tdse_split_observe_dev with obs_every = 1: the run with its rows;
  (c) the route there was: tdse_split_dev with snap_every = 1 into device memory, then a torch contraction of c0 and the snapshots
      with the same matrices and bands (the mix with B as a matmul, the band as 2k - 1 shifted multiply-adds, the conjugate dot).

One untimed run of each route, then REPS repetitions alternating between the three.  Wall time between synchronised points; medians,
and (max - min) / median as the spread.  Every repetition restarts from the same packets; (a), (b) and (c) must return the same
packets bit for bit, and the rows of (b) and (c) are compared.  Reported: (b) / (a), (c) / (b), the bytes of snapshots (c) needs.
Not measured: hardware counters; the host variants; obs_every > 1.  Writes a text report (default
profiles/r25_tdse_split_observe.txt) and prints one JSON line.

    timeout -k 10 600 python tools/tdse_split_observe_rate.py [--out FILE] [--only 1,2]
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


def contract(pk, Bd, GEd):
    """e (npackets, nscan, nexp) complex of packets pk (npackets, nscan, nch, n) in torch: the caller's code of route (c)"""
    b, n = (GEd.shape[1] - 1) // 2, pk.shape[-1]
    out = []
    for o in range(Bd.shape[0]):
        u = torch.nn.functional.pad(torch.view_as_real(torch.matmul(Bd[o].to(pk.dtype), pk)), (0, 0, b, b))   # (.., nch, n + 2b, 2)
        y = torch.zeros(pk.shape + (2,), dtype=torch.float64, device=pk.device)
        for d in range(-b, b + 1):
            y += GEd[o, d + b, :, None] * u[..., b + d:b + d + n, :]
        out.append((pk.conj() * torch.view_as_complex(y)).sum(dim=(-1, -2)))
    return torch.stack(out, dim=-1)


def workload(name, nch, n, nscan, nsteps):
    rb = 0.25 * n
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=rb, k=K, nfun=n, l_fin=nch - 1, n0_ini=1, l_ini=0, zatom=1.0))
    E, info = prob.solve(0, 1)
    assert np.all(info == 0)
    v1s = prob.eigvecs(0, 1, 1)[0]
    prob.assemble(0, nch)
    chans = [(l, 0) for l in range(nch)]
    G = np.ascontiguousarray(prob.dipole_bands()[0])
    WB = prob.operator_bands(host.cap_profile(prob.quadrature()[0], 0.75 * rb, 1e-3), [0])[0]
    c0 = np.ascontiguousarray(np.broadcast_to(host.spline_packet(prob, chans, 0, v1s), (nscan, nch, n)))
    tm = host.spline_midpoints(0.0, DT, nsteps)
    F = np.linspace(0.01, 0.1, nscan)[None, :] * (np.sin(np.pi * tm / (nsteps * DT)) ** 2)[:, None]
    Q, lam = host.split_angular(chans)
    Bdip, Gdip = host.split_expect_dipole(prob, chans)
    Bacc, Gacc = host.split_expect_accel(prob, chans)
    B, GE = np.concatenate([Bdip, Bacc]), np.concatenate([Gdip, Gacc])
    nexp, RW = 2, nch + 4
    l = np.arange(nch, dtype=np.int32)
    c0d, Gd, Wd, fd, Bd, GEd = put(c0), put(G), put(WB), put(F.astype(np.complex128)), put(B), put(GE)
    ca, cb, cc = torch.empty_like(c0d), torch.empty_like(c0d), torch.empty_like(c0d)
    obs = torch.zeros((nsteps + 1, nscan, RW), dtype=torch.float64, device=DEV)
    snaps = torch.zeros((nsteps, nscan, nch, n), dtype=torch.complex128, device=DEV)
    common = dict(G_ptr=Gd.data_ptr(), Q=Q, lam=lam, f_ptr=fd.data_ptr(), nabs=1, W_ptr=Wd.data_ptr())
    rows_c = [None]

    def run_a():
        ca.copy_(c0d)
        return prob.tdse_split_dev(l, nscan, nsteps, DT, ca.data_ptr(), **common)

    def run_b():
        cb.copy_(c0d)
        return prob.tdse_split_observe_dev(l, nscan, nsteps, DT, cb.data_ptr(), obs_every=1, obs_ptr=obs.data_ptr(),
                                           expect=(B, GEd.data_ptr()), **common)

    def run_c():
        cc.copy_(c0d)
        info = prob.tdse_split_dev(l, nscan, nsteps, DT, cc.data_ptr(), snap_every=1, snap_ptr=snaps.data_ptr(), **common)
        rows_c[0] = torch.cat([contract(c0d[None], Bd, GEd), contract(snaps, Bd, GEd)])
        return info

    runs = [("a", run_a), ("b", run_b), ("c", run_c)]
    for key, run in runs:                                              # untimed: first launches
        assert np.all(run() == 0), key
    first = bits(ca)
    t = {key: [] for key, _ in runs}
    for _ in range(REPS):
        for key, run in runs:
            t[key].append(wall(run)[0])
    assert np.array_equal(bits(ca), first) and np.array_equal(bits(cb), first) and np.array_equal(bits(cc), first)
    rows_b = host.split_expect_rows(obs.cpu().numpy(), nch, 0)
    diff = float(np.max(np.abs(rows_b - rows_c[0].cpu().numpy())))
    med = {key: statistics.median(v) for key, v in t.items()}
    rba, rcb = [p / q for p, q in zip(t["b"], t["a"])], [p / q for p, q in zip(t["c"], t["b"])]
    snap_bytes = 16 * nscan * nch * n * nsteps
    r = {"channels": nch, "nfun": n, "packets": nscan, "steps": nsteps, "nexp": nexp}
    for key in "abc":
        r[key + "_ms"] = [round(1e3 * x, 3) for x in t[key]]
        r[key + "_median_ms"] = round(1e3 * med[key], 3)
        r[key + "_relative_spread"] = round(spread(t[key]), 4)
    r.update({"b_over_a": round(med["b"] / med["a"], 4), "b_over_a_range": [round(min(rba), 4), round(max(rba), 4)],
              "c_over_b": round(med["c"] / med["b"], 4), "c_over_b_range": [round(min(rcb), 4), round(max(rcb), 4)],
              "snapshot_bytes_of_c": snap_bytes, "largest_row_difference_b_c": diff,
              "largest_dipole": float(np.max(np.abs(rows_b[..., 0]))), "largest_acceleration": float(np.max(np.abs(rows_b[..., 1])))})
    line = ("%s: l = 0..%d, nfun = %d, %d packets x %d steps, nexp = 2, every step observed: (a) no rows: %s ms (median %.3f, (max - min) / median "
            "= %.1f %%); (b) observing call: %s ms (median %.3f, %.1f %%); (c) snapshots + torch contraction: %s ms (median %.3f, %.1f %%); "
            "(b) / (a) = %.4f [%.4f .. %.4f]; (c) / (b) = %.3f [%.3f .. %.3f]; (c) holds %.1f MB of snapshots (%d bytes), (b) %d bytes of rows; "
            "largest |row (b) - row (c)| = %.3e (largest |<z>| %.3e, largest |<dV/dr cos theta>| %.3e)"
            % (name, nch - 1, n, nscan, nsteps, ms(t["a"]), 1e3 * med["a"], 100 * spread(t["a"]), ms(t["b"]), 1e3 * med["b"], 100 * spread(t["b"]),
               ms(t["c"]), 1e3 * med["c"], 100 * spread(t["c"]), r["b_over_a"], min(rba), max(rba), r["c_over_b"], min(rcb), max(rcb),
               snap_bytes / 1e6, snap_bytes, 8 * (nsteps + 1) * nscan * RW, diff, r["largest_dipole"], r["largest_acceleration"]))
    prob.close()
    del snaps, obs
    torch.cuda.empty_cache()
    return r, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_tdse_split_observe.txt"))
    ap.add_argument("--only", default="1,2")
    args = ap.parse_args()
    only = [int(s) for s in args.only.split(",")]
    jobs = []
    if 1 in only:
        jobs += [("(1) nfun = 1024", 4, 1024, 64, 32), ("(1) nfun = 4096", 4, 4096, 64, 32)]
    if 2 in only:
        jobs += [("(2)", 64, 4096, 1, 8)]
    out = {"workload": "channels l = 0.. at m = 0 coupled by F(t) z, k = %d, dt = %g, absorber on; dipole and acceleration rows on every step; "
                       "%d repetitions, alternating" % (K, DT, REPS)}
    lines = []
    for job in jobs:
        r, line = workload(*job)
        out[job[0]] = r
        lines.append(line)
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_split_observe_rate.py: bspatom_tdse_split_dev without rows (a), bspatom_tdse_split_observe_dev with dipole and acceleration "
                "rows (b), and snapshots of every step contracted in torch (c), on the same workload in the same run, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
        f.write("Not measured: hardware counters; the host variants; obs_every > 1.\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
