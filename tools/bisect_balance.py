#!/usr/bin/env python3
"""bisect_balance.py -- where the workgroups of csrc/tridiag.hip::bisect3_kernel run and how long: one solve of BASELINE configs[3]'s
pencil (n = 4096, k = 9) with the instrumented kernel (option bisect_diag: a record per logical workgroup on stderr -- x, channel,
XCD, CU, wall-clock stamps, rounds), then
  1. duration and rounds by x (the quarter of the spectrum the workgroup owns);
  2. which x share a CU and an XCD;
  3. per CU: the time it has a workgroup, against the kernel's time, and the rounds it runs;
  4. for the queue launch (bisect_queue, the records then carry the hardware workgroup and its arrival number on its CU): items per
     hardware workgroup, which x started together on a CU, and when the CUs of every such starting set were done.
usage: tools/bisect_balance.py [--channels N] [--save FILE | --records FILE] [name=value ...]      (e.g. bisect_pair=0, bisect_queue=0)
--save keeps the records as the library wrote them; --records reports on such a file instead of running a solve."""
import os
import sys
import tempfile
from collections import Counter, defaultdict
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bspatom_amd import capi


def captured_stderr(fn):
    """what fn() and the library under it write to file descriptor 2"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode()


def parse(text):
    head, recs = None, []
    for line in text.splitlines():
        f = line.split()
        if line.startswith("bisect3 diag:"):
            head = {f[i]: f[i + 1] for i in range(2, len(f) - 1, 2) if f[i] not in ("grid",)}
            head["grid"] = line.split("grid ")[1].split(" lds")[0]
        elif line.startswith("bisect3 wg:"):
            recs.append({f[i]: int(f[i + 1], 0) for i in range(2, len(f) - 1, 2)})
    return head, recs


def union_length(iv):
    tot, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end: tot += b - a; end = b
        elif b > end: tot += b - end; end = b
    return tot


def report(head, recs):
    tick_ms = 1.0 / float(head["wall_khz"])
    t_first = min(r["t0"] for r in recs); t_last = max(r["t1"] for r in recs)
    kernel = (t_last - t_first) * tick_ms
    print("launch: n %s, %s channels, %s logical workgroups per channel, pair_stride %s, queue %s, grid %s, %s bytes of LDS, %s CUs; first start to last end %.2f ms"
          % (head["n"], head["batch"], head["nw"], head["pair_stride"], head.get("queue", "0"), head["grid"], head["lds"], head["cus"], kernel))
    print("1. by x: workgroups, duration in ms (mean / min / max), start after the first start (mean), lock-step + tail rounds (mean; max of the sum)")
    xs = sorted({r["x"] for r in recs})
    dur_x = {}
    for x in xs:
        rr = [r for r in recs if r["x"] == x]
        d = np.array([(r["t1"] - r["t0"]) * tick_ms for r in rr])
        s = np.array([(r["t0"] - t_first) * tick_ms for r in rr])
        dur_x[x] = d.mean()
        print("   x %d: %4d   %.2f / %.2f / %.2f   start %.2f   rounds %.1f + %.1f; %d" % (
            x, len(rr), d.mean(), d.min(), d.max(), s.mean(), np.mean([r["rounds"] for r in rr]), np.mean([r["tail"] for r in rr]),
            max(r["rounds"] + r["tail"] for r in rr)))
    dm = np.array(list(dur_x.values()))
    print("   the per-x mean durations differ by %.0f %% of their mean" % (100 * (dm.max() - dm.min()) / dm.mean()))
    cu_of = lambda r: (r["xcc"], (r["hwid"] >> 8) & 0xff)           # XCD; SE, SH and CU bits of HW_REG_HW_ID
    by_xcd, by_cu = defaultdict(Counter), defaultdict(list)
    for r in recs:
        by_xcd[r["xcc"]][r["x"]] += 1
        by_cu[cu_of(r)].append(r)
    print("2. placement: workgroups of every x per XCD")
    for xcc in sorted(by_xcd):
        print("   XCD %d: %s" % (xcc, "  ".join("x %d: %d" % (x, by_xcd[xcc][x]) for x in xs)))
    mix = Counter(tuple(sorted(r["x"] for r in rr)) for rr in by_cu.values())
    print("   the x that share a CU -> CUs with that set: %s" % "  ".join("%s: %d" % (k, v) for k, v in sorted(mix.items())))
    busy = np.array([union_length([(r["t0"], r["t1"]) for r in rr]) * tick_ms for rr in by_cu.values()])
    rsum = np.array([sum(r["rounds"] + r["tail"] for r in rr) for rr in by_cu.values()], float)
    print("3. per CU (%d of %s hold a workgroup): time with a workgroup / the kernel's %.2f ms: mean %.0f %%, min %.0f %%, max %.0f %%" % (
        len(by_cu), head["cus"], kernel, 100 * busy.mean() / kernel, 100 * busy.min() / kernel, 100 * busy.max() / kernel))
    print("   rounds per CU: mean %.1f, min %d, max %d (max %.0f %% above the mean)" % (rsum.mean(), rsum.min(), rsum.max(),
                                                                                      100 * (rsum.max() / rsum.mean() - 1)))
    if head.get("queue", "0") != "1":
        return
    by_hwg = defaultdict(list)
    for r in recs:
        by_hwg[r["hwg"]].append(r)
    per = np.array([len(v) for v in by_hwg.values()])
    sides = Counter(v[0]["side"] for v in by_hwg.values())
    print("4. queue: %d hardware workgroups ran items, %.2f items each (max %d); arrival number on the CU -> workgroups: %s" % (
        len(by_hwg), per.mean(), per.max(), "  ".join("%d: %d" % kv for kv in sorted(sides.items()))))
    ends = defaultdict(list)                                       # the x that started together on a CU -> end of that CU's last item
    for rr in by_cu.values():
        firsts = [min(v, key=lambda r: r["t0"]) for v in by_hwg.values() if cu_of(v[0]) == cu_of(rr[0])]
        start = tuple(r["x"] for r in sorted(firsts, key=lambda r: r["side"]))
        ends[start].append((max(r["t1"] for r in rr) - t_first) * tick_ms)
    print("   x that started together on a CU (by arrival) -> CUs, end of the CU's last item in ms (mean / max)")
    for k, v in sorted(ends.items()):
        print("   %-10s %4d   %.2f / %.2f" % (k, len(v), np.mean(v), np.max(v)))


if __name__ == "__main__":
    args = sys.argv[1:]
    chans, opts, save, records = 128, {}, None, None
    while args:
        a = args.pop(0)
        if a == "--channels": chans = int(args.pop(0))
        elif a == "--save": save = args.pop(0)
        elif a == "--records": records = args.pop(0)
        else:
            k, v = a.split("="); opts[k] = int(v)
    if records:
        head, recs = parse(open(records).read())
        print("== records of %s" % records)
        report(head, recs)
        sys.exit(0)
    for k, v in opts.items():
        capi.set_option(k, v)
    prob = capi.Problem(capi.make_input(kind_grid=0, ra=0.0, rb=800.0, k=9, nfun=4096, n0_ini=1, l_ini=0, l_fin=127, zatom=1.0))
    prob.solve(0, chans)                                            # warm-up: the instrumented launch is not the process's first
    capi.set_option("bisect_diag", 1)
    try:
        text = captured_stderr(lambda: prob.solve(0, chans))
    finally:
        capi.set_option("bisect_diag", 0)
    prob.close()
    if save:
        with open(save, "w") as f:
            f.write("".join(l + "\n" for l in text.splitlines() if l.startswith("bisect3 ")))
    head, recs = parse(text)
    if not head or not recs:
        sys.exit("no diagnostic records on stderr:\n" + text[-2000:])
    print("== %d channels %s" % (chans, " ".join("%s=%d" % kv for kv in opts.items())))
    report(head, recs)
