#!/usr/bin/env python3
"""dipole_rate.py -- bspatom_dipole_matrix (csrc/dipole.hip) against the loop of per-state bspatom_dipole_elements calls it
replaces, in one process on one GPU, on the C4 grid (n = 4096, k = 9) after a 32-channel solve; prints one JSON line.

States 1 .. 256 on both sides, the pairs (l, l + 1) for l = 0 .. 30 (31 pairs, 31 x 256 x 256 elements):
  - one dipole_matrix call (host output) and one dipole_matrix_dev call (device output): wall time
  - the per-state loop: 8 sampled initial states of the pair (0, 1) timed, then SCALED to 31 pairs x 256 states (the output
    says so); the sampled rows are compared with the one call's

Every time is wall time between synchronised points (each call returns when its stream has drained).  The kernel-time split
(inverse iterations, band apply, product) comes from a run of its own under the profiler:

    timeout -k 10 600 python tools/dipole_rate.py
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -- python tools/dipole_rate.py
"""
import json
import os
import sys
import time

import numpy as np
import torch                               # first: its HIP runtime is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bspatom_amd import capi                # noqa: E402
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
    nch, cnt, sample = 32, 256, 8
    prob = capi.Problem(c4_input(nch - 1))
    n = prob.nfun
    E, info = prob.solve(0, nch)
    assert np.all(info == 0)
    pairs = [(l, l + 1) for l in range(nch - 1)]
    a = [1.0, 0.0, 0.0]
    prob.dipole_matrix(pairs[:1], 1, 1, 1, 1, a)              # the first launches outside the timing
    prob.dipole_elements(0, 1, 1, 1, 1, a)
    t_h, D = wall(lambda: prob.dipole_matrix(pairs, 1, cnt, 1, cnt, a))
    Dd = torch.empty((len(pairs), cnt, cnt), dtype=torch.float64, device="cuda:0")
    t_d, _ = wall(lambda: prob.dipole_matrix_dev(pairs, 1, cnt, 1, cnt, a, Dd.data_ptr()))
    rows = [int(r) for r in np.linspace(0, cnt - 1, sample)]
    t_s, R = wall(lambda: [prob.dipole_elements(0, 1 + r, 1, 1, cnt, a) for r in rows])
    t_loop = t_s / sample * cnt * len(pairs)
    dev = max(float(np.max(np.abs(D[0, r] - R[i]))) for i, r in enumerate(rows))
    out = {"workload": "C4 grid n=%d k=%d, %d channels solved; %d pairs (l, l+1), states 1..%d on both sides" % (n, prob.k, nch, len(pairs), cnt),
           "elements": len(pairs) * cnt * cnt,
           "dipole_matrix_host_s": round(t_h, 4), "dipole_matrix_dev_s": round(t_d, 4),
           "dev_equals_host": bool(np.array_equal(Dd.cpu().numpy(), D)),
           "loop_sample": {"pair": [0, 1], "initial_states": [r + 1 for r in rows], "sample_s": round(t_s, 4)},
           "loop_s_SCALED_from_sample": round(t_loop, 2),
           "note": "loop time = sample time / %d x %d states x %d pairs (scaled, not run in full)" % (sample, cnt, len(pairs)),
           "speedup_host": round(t_loop / t_h, 1), "speedup_dev": round(t_loop / t_d, 1),
           "max_abs_diff_on_sampled_rows": dev, "max_abs_D_pair0": float(np.max(np.abs(D[0])))}
    prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
