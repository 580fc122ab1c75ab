#!/usr/bin/env python3
"""tdse_observe_rate.py -- what the observables of bspatom_tdse_observe_dev cost per step, in one process on one GPU, on the workload
of tools/tdse_rate.py: 32 channels in a chain, 256 states each, 500 steps, at nscan = 1 and nscan = 16.  Writes a text report
(default profiles/r10_tdse_observe.txt) and prints one JSON line.

  (a) bspatom_tdse_propagate_dev: the run without observables (seven launches per step);
  (b) bspatom_tdse_observe_dev with obs_every = 1: the observing stage 0 and the reduction on every step (eight launches);
  (c) the route without it: bspatom_tdse_propagate_dev with snap_every = 1, then a torch contraction of the snapshots with D
      (pop, sum E |a|^2 and z_c of every step, in chunks of 50 steps) -- the snapshot traffic and one more read of D per step.

Every time is wall time between synchronised points, the second of two runs of each.  The report quotes (b) / (a), (b) - (a) and
(c) / (b), and the largest difference between the rows of (b) and of (c).

    timeout -k 10 600 python tools/tdse_observe_rate.py [--out FILE] [--steps N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch                               # first: its HIP runtime is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspatom_amd import capi, host          # noqa: E402

NCH, COUNT, DT, CHUNK = 32, 256, 0.01, 50


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def torch_observables(E, Dc, states):
    """rows (T, nscan, nch, 4) of the chain from states (T, nscan, nch, count) complex128; Dc (nch-1, count, count) complex"""
    out = torch.zeros(states.shape[:3] + (4,), dtype=torch.float64, device=states.device)
    for t0 in range(0, states.shape[0], CHUNK):
        s = states[t0:t0 + CHUNK]
        T, nscan = s.shape[0], s.shape[1]
        p2 = s.real * s.real + s.imag * s.imag
        out[t0:t0 + T, :, :, 0] = p2.sum(dim=-1)
        out[t0:t0 + T, :, :, 1] = (E * p2).sum(dim=-1)
        lo = s[:, :, :-1].permute(2, 0, 1, 3).reshape(NCH - 1, T * nscan, COUNT)               # a_ci
        hi = s[:, :, 1:].permute(2, 0, 1, 3).reshape(NCH - 1, T * nscan, COUNT)                # a_cf
        z = (torch.conj(hi) * torch.matmul(lo, Dc)).sum(dim=-1).reshape(NCH - 1, T, nscan).permute(1, 2, 0)
        out[t0:t0 + T, :, 1:, 2] = z.real
        out[t0:t0 + T, :, 1:, 3] = z.imag
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_tdse_observe.txt"))
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
    Dc = Dd.to(torch.complex128)
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
        od = torch.zeros((nsteps + 1, nscan, NCH, 4), dtype=torch.float64, device=dev)
        sd = torch.zeros((nsteps + 1, nscan, NCH, COUNT), dtype=torch.complex128, device=dev)      # [0] = a0, then the snapshots
        sd[0] = a0d
        run_a = lambda n: prob.tdse_propagate_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr())
        run_b = lambda n: prob.tdse_observe_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr(),
                                                1, od.data_ptr())

        def run_c(n):
            prob.tdse_propagate_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr(), 1,
                                    sd[1:].data_ptr())
            return torch_observables(Ed, Dc, sd[:n + 1])

        t, res = {}, {}
        for key, run in (("a", run_a), ("b", run_b), ("c", run_c)):
            ad.copy_(a0d)
            run(2)                                                   # the first launches outside the timing
            for _ in range(2):
                ad.copy_(a0d)
                t[key], res[key] = wall(lambda: run(nsteps))
            res[key + "_a"] = ad.cpu().numpy()
        same_a = bool(np.array_equal(res["a_a"].view(np.uint64), res["b_a"].view(np.uint64)))
        diff = float((od - res["c"]).abs().max())
        capi.set_option("ktime", 1)
        capi.kernel_times()
        ad.copy_(a0d)
        run_b(10)
        ms, launches = next(v for k, v in capi.kernel_times().items() if "tdse_stage_kernel" in k)
        capi.set_option("ktime", 0)
        r = {"nscan": nscan, "propagate_ms_per_step": round(1e3 * t["a"] / nsteps, 4), "observe_ms_per_step": round(1e3 * t["b"] / nsteps, 4),
             "snapshot_torch_ms_per_step": round(1e3 * t["c"] / nsteps, 4), "b_over_a": round(t["b"] / t["a"], 3),
             "b_minus_a_us_per_step": round(1e6 * (t["b"] - t["a"]) / nsteps, 2), "c_over_b": round(t["c"] / t["b"], 2),
             "stage_slot_launches_per_step": launches / 10.0, "stage_slot_us_per_launch": round(1e3 * ms / launches, 2),
             "a_bit_identical_to_propagate": same_a, "max_abs_diff_rows_b_c": diff}
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: (a) propagate %.4f ms/step, (b) observe every step %.4f ms/step, (c) snapshot every step + torch "
                     "contraction %.4f ms/step; (b)/(a) = %.3f, (b)-(a) = %.2f us/step, (c)/(b) = %.2f; stage slot of (b): %.1f launches/step "
                     "(+ the step kernel and the reduction), %.2f us each under events; amplitudes of (b) bit-identical to (a): %s; "
                     "max|rows of (b) - rows of (c)| %.3g"
                     % (nscan, r["propagate_ms_per_step"], r["observe_ms_per_step"], r["snapshot_torch_ms_per_step"], r["b_over_a"],
                        r["b_minus_a_us_per_step"], r["c_over_b"], r["stage_slot_launches_per_step"], r["stage_slot_us_per_launch"], same_a, diff))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_observe_rate.py: bspatom_tdse_observe_dev against bspatom_tdse_propagate_dev and against snapshots + torch, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
