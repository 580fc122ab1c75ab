#!/usr/bin/env python3
"""eigvecs_rate.py -- bspatom_eigvecs_batch (csrc/eigvec.hip::invit_batch_kernel) against bspatom_eigvecs per channel, in one
process on one GPU, on the C4 input (n = 4096, k = 9, 128 channels); prints one JSON line.

  (a) all 4096 vectors of 32 channels through eigvecs_batch_dev, against eigvecs per channel on 4 channels: channels/s
  (b) the KIND_PI >= 3 shape, 256 vectors of each of the 128 channels: eigvecs_batch (host memory, as write_eigenvec_all
      asks) and eigvecs_batch_dev, against the per-channel loop over the same channels: wall time

Every time is wall time between synchronised points (each call returns when its stream has drained).

    timeout -k 10 600 python tools/eigvecs_rate.py
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


def c4_input():
    nl = read_namelists(open(os.path.join(ROOT, "tests", "golden", "inputs", "c4_4096.inp")).read())
    kw = {}
    kw.update(nl["vars_bsp"]); kw.update(nl["vars_tise"]); kw["l_fin"] = 127
    return capi.make_input(**kw)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def main():
    prob = capi.Problem(c4_input())
    n, nch = prob.nfun, prob.lmax + 1
    E, info = prob.solve(0, nch)
    assert np.all(info == 0)
    out = {"workload": "C4 n=%d k=%d, %d channels solved" % (n, prob.k, nch)}
    # (a) all vectors
    nl_a, loop_a = 32, 4
    Zd = torch.empty((nl_a, n, n), dtype=torch.float64, device="cuda:0")
    prob.eigvecs_batch_dev(0, 1, 1, 1, Zd.data_ptr())         # the first launch outside the timing
    t_b, _ = wall(lambda: prob.eigvecs_batch_dev(0, nl_a, 1, n, Zd.data_ptr()))
    t_l, R = wall(lambda: [prob.eigvecs(l, 1, n) for l in range(loop_a)])
    same = all(np.array_equal(Zd[l].cpu().numpy(), R[l]) for l in range(loop_a))
    del Zd, R
    out["a_all_vectors"] = {"channels": nl_a, "vectors_per_channel": n, "batch_dev_s": round(t_b, 4),
                            "batch_channels_per_s": round(nl_a / t_b, 2), "loop_channels": loop_a, "loop_s": round(t_l, 4),
                            "loop_channels_per_s": round(loop_a / t_l, 2), "speedup": round((t_l / loop_a) / (t_b / nl_a), 2),
                            "bit_identical_on_loop_channels": same}
    # (b) KIND_PI >= 3 shape
    cnt = 256
    t_bh, Zh = wall(lambda: prob.eigvecs_batch(0, nch, 1, cnt))
    Zd = torch.empty((nch, cnt, n), dtype=torch.float64, device="cuda:0")
    t_bd, _ = wall(lambda: prob.eigvecs_batch_dev(0, nch, 1, cnt, Zd.data_ptr()))
    t_lp, R = wall(lambda: [prob.eigvecs(l, 1, cnt) for l in range(nch)])
    same = np.array_equal(Zh, np.stack(R)) and np.array_equal(Zd.cpu().numpy(), Zh)
    out["b_kind_pi3_shape"] = {"channels": nch, "vectors_per_channel": cnt, "batch_host_s": round(t_bh, 4),
                               "batch_dev_s": round(t_bd, 4), "loop_s": round(t_lp, 4), "speedup_host": round(t_lp / t_bh, 2),
                               "speedup_dev": round(t_lp / t_bd, 2), "bit_identical": bool(same)}
    prob.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
