#!/usr/bin/env python3
"""tdse_rate.py -- bspatom_tdse_propagate_dev (csrc/tdse.hip) against a torch complex128 restatement of the same Runge-Kutta step
on the same device -- what a user can do today with dipole_matrix_dev's output -- in one process on one GPU: 32 channels in a
chain, 256 states each, 500 steps, at nscan = 1 and nscan = 16.  Writes a text report (default profiles/r09_tdse_propagate.txt) and
prints one JSON line.

  ms per step of both; launches per step of the library from bspatom_kernel_times (option "ktime", a separate short run: the stage
  kernel's slot, plus the one step kernel); effective D bytes/s (every block read once per stage) and flop/s (both orientations of
  every block times 2 nscan real columns) of the library call.

Every time is wall time between synchronised points.  For scale: a dependent launch costs about 9.4 us here, so 7 launches per step
put the floor of this design at about 65 us per step.

    timeout -k 10 600 python tools/tdse_rate.py [--out FILE] [--steps N]
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

NCH, COUNT, DT = 32, 256, 0.01
A = [[float(x) for x in row] for row in host.RK_A]
D5 = [float(x) for x in host.RK_D]
DE = [float(x - y) for x, y in zip(host.RK_D, host.RK_B)]


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def torch_propagate(E, Dc, a, field, dt):
    """the chain's step in torch complex128: a (nscan, nch, count), Dc (nch-1, count, count) complex, field (nsteps, 6, nscan)"""
    err = torch.zeros(a.shape[0], dtype=torch.float64, device=a.device)
    DcT = Dc.transpose(1, 2)

    def rhs(y, f):
        h = E * y
        yt = y.transpose(0, 1)                                        # (nch, nscan, count)
        h[:, 1:] += f[:, None, None] * torch.matmul(yt[:-1], Dc).transpose(0, 1)             # D_p^T a_ci
        h[:, :-1] += torch.conj(f)[:, None, None] * torch.matmul(yt[1:], DcT).transpose(0, 1)   # D_p a_cf
        return -1j * h

    for n in range(field.shape[0]):
        k = []
        for s in range(6):
            y = a
            if s:
                acc = A[s][0] * k[0]
                for j in range(1, s):
                    acc = acc + A[s][j] * k[j]
                y = a + dt * acc
            k.append(rhs(y, field[n, s]))
        a = a + dt * (D5[0] * k[0] + D5[2] * k[2] + D5[3] * k[3] + D5[4] * k[4] + D5[5] * k[5])
        e = DE[0] * k[0] + DE[2] * k[2] + DE[3] * k[3] + DE[4] * k[4] + DE[5] * k[5]
        err = torch.maximum(err, dt * e.abs().reshape(a.shape[0], -1).amax(dim=1))
    return a, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_tdse_propagate.txt"))
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
        run = lambda n: prob.tdse_propagate_dev(NCH, COUNT, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, n, DT, fd.data_ptr(), ad.data_ptr())
        run(2)                                                       # the first launches outside the timing
        ad.copy_(torch.from_numpy(a0))
        t_lib, err = wall(lambda: run(nsteps))
        a_lib = ad.cpu().numpy()
        capi.set_option("ktime", 1)
        capi.kernel_times()
        run(10)
        ms, launches = next(v for k, v in capi.kernel_times().items() if "tdse_stage_kernel" in k)
        capi.set_option("ktime", 0)
        at = torch.from_numpy(a0).to(dev)
        torch_propagate(Ed, Dc, at, fd[:2], DT)
        t_t, (a_t, err_t) = wall(lambda: torch_propagate(Ed, Dc, at, fd, DT))
        diff = float(np.max(np.abs(a_t.cpu().numpy() - a_lib)))
        dbytes = 6.0 * D.size * 8 * nsteps
        flop = 6.0 * 2 * len(pairs) * 2.0 * COUNT * COUNT * 2 * nscan * nsteps
        r = {"nscan": nscan, "lib_ms_per_step": round(1e3 * t_lib / nsteps, 4), "torch_ms_per_step": round(1e3 * t_t / nsteps, 4),
             "speedup": round(t_t / t_lib, 2), "launches_per_step": launches / 10.0 + 1, "stage_kernel_us": round(1e3 * ms / launches, 2),
             "D_GB_per_s": round(dbytes / t_lib / 1e9, 1), "Gflop_per_s": round(flop / t_lib / 1e9, 1),
             "max_abs_diff_lib_torch": diff, "max_err": float(np.max(err)), "max_err_torch": float(err_t.max())}
        out["nscan_%d" % nscan] = r
        lines.append("nscan = %2d: library %.4f ms/step, torch complex128 %.4f ms/step (x %.2f); %.0f launches/step (stage kernel %.2f us "
                     "each under events); D %.1f GB/s, %.1f Gflop/s; max|a_lib - a_torch| %.3g; err %.3g (torch %.3g)"
                     % (nscan, r["lib_ms_per_step"], r["torch_ms_per_step"], r["speedup"], r["launches_per_step"], r["stage_kernel_us"],
                        r["D_GB_per_s"], r["Gflop_per_s"], diff, r["max_err"], r["max_err_torch"]))
    prob.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/tdse_rate.py: bspatom_tdse_propagate_dev against a torch complex128 restatement, one MI355X\n")
        f.write(out["workload"] + "\n")
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
