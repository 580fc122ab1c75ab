#!/usr/bin/env python3
"""wavefunctions_rate.py -- bspatom_wavefunctions_dev / bspatom_tabulate_dev (csrc/wavefn.hip) on the C4 grid (n = 4096, k = 9,
49 080 quadrature points) after a 32-channel solve, in one process on one GPU; prints one JSON line.

States 1 .. 256 of the 32 channels on the quadrature grid, u and u' (2 x 32 x 256 x 49 080 doubles = 6.4 GB), _dev variants:
  - one wavefunctions_dev call (inverse iterations + tables): wall time
  - one tabulate_dev call on the same eigenvectors already in device memory (eigvecs_batch_dev): wall time, and the bytes of
    U and dU per second of that wall time (the basis gather and the synchronisation are inside it)
  - the only route before these entry points, write_wf per state (one vector, values only, a uniform grid of as many points):
    8 sampled states timed, then SCALED to 32 x 256 states (the output says so)

Every time is wall time between synchronised points.  The kernel split (inverse iterations, gather, tabulation) comes from a
run of its own under the profiler:

    timeout -k 10 600 python tools/wavefunctions_rate.py
    timeout -k 10 600 rocprofv3 --kernel-trace --stats -- python tools/wavefunctions_rate.py
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
    npts = prob.quadrature()[0].size
    U = torch.empty((nch, cnt, npts), dtype=torch.float64, device="cuda:0")
    dU = torch.empty((nch, cnt, npts), dtype=torch.float64, device="cuda:0")
    Z = torch.empty((nch, cnt, n), dtype=torch.float64, device="cuda:0")
    prob.wavefunctions_dev(0, 1, 1, 1, U.data_ptr(), dU.data_ptr())          # the first launches outside the timing
    prob.write_wf(np.ones(n), npts)
    t_w, _ = wall(lambda: prob.wavefunctions_dev(0, nch, 1, cnt, U.data_ptr(), dU.data_ptr()))
    t_e, _ = wall(lambda: prob.eigvecs_batch_dev(0, nch, 1, cnt, Z.data_ptr()))
    U2 = torch.empty_like(U); dU2 = torch.empty_like(dU)
    t_t, _ = wall(lambda: prob.tabulate_dev(nch * cnt, Z.data_ptr(), U2.data_ptr(), dU2.data_ptr()))
    t_t2, _ = wall(lambda: prob.tabulate_dev(nch * cnt, Z.data_ptr(), U2.data_ptr(), dU2.data_ptr()))
    t_v, _ = wall(lambda: prob.tabulate_dev(nch * cnt, Z.data_ptr(), U2.data_ptr(), None))
    same = bool(torch.equal(U, U2)) and bool(torch.equal(dU, dU2))
    rows = [int(r) for r in np.linspace(0, cnt - 1, sample)]
    Zs = Z[0][rows].cpu().numpy()
    t_s, R = wall(lambda: [prob.write_wf(Zs[i], npts) for i in range(sample)])
    t_loop = t_s / sample * cnt * nch
    nbytes = 2 * nch * cnt * npts * 8
    out = {"workload": "C4 grid n=%d k=%d, %d channels solved; states 1..%d of every channel on the %d quadrature points, u and u'"
                       % (n, prob.k, nch, cnt, npts),
           "table_bytes": nbytes,
           "wavefunctions_dev_s": round(t_w, 4), "eigvecs_batch_dev_s": round(t_e, 4),
           "tabulate_dev_s": round(t_t, 5), "tabulate_dev_again_s": round(t_t2, 5),
           "tabulate_dev_written_TB_per_s_of_wall": round(nbytes / min(t_t, t_t2) / 1e12, 3),
           "tabulate_dev_values_only_s": round(t_v, 5),
           "wavefunctions_dev_equals_tabulate_dev_of_eigvecs_batch_dev": same,
           "write_wf_sample": {"channel": 0, "states": [r + 1 for r in rows], "points": npts + 1, "sample_s": round(t_s, 4)},
           "write_wf_loop_s_SCALED_from_sample": round(t_loop, 2),
           "note": "write_wf loop = sample time / %d x %d states x %d channels (scaled, not run in full); it gives u only, on a uniform grid"
                   % (sample, cnt, nch),
           "speedup_wavefunctions_dev": round(t_loop / t_w, 1), "speedup_tabulate_dev": round(t_loop / min(t_t, t_t2), 1)}
    prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
