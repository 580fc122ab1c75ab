#!/usr/bin/env python3
"""operator_matrix_rate.py -- bspatom_operator_matrix (csrc/opmat.hip) against the quadrature route host.radial_matrix it
relieves, in one process on one GPU, on the C4 grid (n = 4096, k = 9) after a 2-channel solve; prints one JSON line.

Channels 0 .. 1, the pairs (0, 1) and (1, 0), states 1 .. 256 on both sides, nop = 1 and nop = 64 operators (smooth profiles
g_o(r) = exp(-r / (5 + o)), every fourth one with d/dr):
  - one Problem.operator_matrix call: wall time after a warm-up call
  - the equivalent host.radial_matrix call(s) (one per operator, summed with the coefficients): wall time after a warm-up
  - operator_band_kernel alone at nop = 64: HIP events around its launch (option "ktime", bspatom_kernel_times)
  - the largest |D - R| relative to max|D|

    timeout -k 10 600 python tools/operator_matrix_rate.py
"""
import json
import os
import sys
import time

import numpy as np
import torch                               # first: its HIP runtime is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspatom_amd import capi, host          # noqa: E402
from bspatom_amd.namelist import read_namelists  # noqa: E402


def c4_input(lmax):
    nl = read_namelists(open(os.path.join(ROOT, "tests", "golden", "inputs", "c4_4096.inp")).read())
    kw = {}
    kw.update(nl["vars_bsp"]); kw.update(nl["vars_tise"]); kw["l_fin"] = lmax
    return capi.make_input(**kw)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    cnt, pairs = 256, [(0, 1), (1, 0)]
    prob = capi.Problem(c4_input(1))
    E, info = prob.solve(0, 2)
    assert np.all(info == 0)
    r = prob.quadrature()[0]
    out = {"workload": "C4 grid n=%d k=%d ka=%d, %d quadrature points, channels 0..1 solved; pairs %s, states 1..%d on both sides"
                       % (prob.nfun, prob.k, prob.ka, r.size, pairs, cnt)}
    for nop in (1, 64):
        g = np.stack([np.exp(-r / (5.0 + o)) for o in range(nop)])
        deriv = np.array([1 if o % 4 == 3 else 0 for o in range(nop)], dtype=np.int32)
        a = 1.0 / (1.0 + np.arange(nop))
        op = lambda: prob.operator_matrix(pairs, g, deriv, 1, cnt, 1, cnt, a)
        rad = lambda: sum(a[o] * host.radial_matrix(prob, pairs, g[o], 1, cnt, 1, cnt, deriv=bool(deriv[o])) for o in range(nop))
        op()
        t_op, D = wall(op)
        if nop == 1:
            rad()
        t_rad, R = wall(rad)
        res = {"operator_matrix_s": round(t_op, 4), "radial_matrix_s": round(t_rad, 4), "radial_matrix_calls": nop,
               "max_abs_diff_over_max_abs_D": float(np.max(np.abs(D - R)) / np.max(np.abs(D))), "max_abs_D": float(np.max(np.abs(D)))}
        if nop == 64:
            gd = torch.from_numpy(g).to("cuda:0")
            GB = torch.empty((nop, 2 * prob.k - 1, prob.nfun), dtype=torch.float64, device="cuda:0")
            prob.operator_bands_dev(nop, gd.data_ptr(), deriv, GB.data_ptr())
            capi.kernel_times()
            capi.set_option("ktime", 1)
            for _ in range(5):
                prob.operator_bands_dev(nop, gd.data_ptr(), deriv, GB.data_ptr())
            capi.set_option("ktime", 0)
            ms, launches = next(v for k, v in capi.kernel_times().items() if "operator_band_kernel" in k)
            res["operator_band_kernel_ms_per_launch_hip_events"] = round(ms / launches, 4)
            res["operator_band_kernel_launches_timed"] = launches
        out["nop_%d" % nop] = res
    prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
