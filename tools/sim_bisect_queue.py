#!/usr/bin/env python3
"""sim_bisect_queue.py -- list-scheduling model of the three launches of csrc/tridiag.hip::bisect3_kernel (CPU, no GPU needed):
  unpaired  one hardware workgroup per item (x, channel), placed as the dispatcher was observed to place them (profiles/r12_bisect_pairs.txt
            section 1: an XCD takes every 8th workgroup, its CUs take them in turn, two per CU; further ones as slots fall free);
  paired    one hardware workgroup per CU runs x and then x + ceil(nw / 2) of its channel (bisect_pair);
  queue     G hardware workgroups, two per CU, claim items from a list in the order of the kernel: the first on a CU from the head (the
            costly end), the second from the tail (bisect_queue).
An item is a logical workgroup with a duration ALONE on a CU.  Two workgroups on a CU slow each other down; the model has the two rates
at which they then advance (alone = 1): `older` for the workgroup that came to the CU first, `younger` for the other.  One co-residency
factor f means both advance at 1 / f.  The rates of r12 (section 1 against section 2, the same items sharing and alone):
  the fastest sharing workgroup of an x takes 1.09 - 1.16 x its time alone (mean 1.12), the slowest 1.72 - 1.83 x (mean 1.77), the mean
  is 1.45 x: NOT one factor for both -- the older workgroup is slowed by r_min = 1.12, the younger advances at `younger` until the older
  one is done and alone afterwards, so it ends at r_max a = r_min a + (1 - r_min younger) a for equal items:
  younger = (1 + r_min - r_max) / r_min = 0.31.
usage: tools/sim_bisect_queue.py [--cus 256] [--grid G] [--factor F | --rates OLDER,YOUNGER] [--records FILE | --r12]
  --records FILE   the durations alone from the records of a launch in which every workgroup had its CU to itself (tools/bisect_balance.py --save
                   of a paired launch); default --r12: the per-x mean / min / max of profiles/r12_bisect_pairs.txt section 2, rising with the channel."""
import sys

# profiles/r12_bisect_pairs.txt: section 2, ms alone on a CU by x (mean, min, max); section 1, the same sharing a CU with the same x
R12_ALONE = {0: (4.77, 4.12, 5.16), 1: (3.50, 3.09, 3.91), 2: (3.66, 3.09, 4.03), 3: (5.65, 4.89, 6.11)}
R12_SHARING = {0: (6.90, 4.58, 9.00), 1: (5.06, 3.37, 6.71), 2: (5.48, 3.58, 7.37), 3: (8.22, 5.49, 10.88)}
R12_UNPAIRED_MS, R12_PAIRED_MS = 10.88, 9.82
XCDS = 8


def r12_rates():
    """(older, younger) from the min and max ratios sharing / alone of r12, averaged over x"""
    rmin = sum(R12_SHARING[x][1] / R12_ALONE[x][1] for x in R12_ALONE) / len(R12_ALONE)
    rmax = sum(R12_SHARING[x][2] / R12_ALONE[x][2] for x in R12_ALONE) / len(R12_ALONE)
    return 1.0 / rmin, (1.0 + rmin - rmax) / rmin


def r12_durations(batch=128):
    """dur[x][ch]: from min (channel 0) to max (the last channel, the rounds rise with l: r12 section 0), the exponent set by the mean"""
    dur = {}
    for x, (mean, lo, hi) in R12_ALONE.items():
        g = (hi - lo) / (mean - lo) - 1.0
        dur[x] = [lo + (hi - lo) * (c / (batch - 1.0)) ** g for c in range(batch)]
    return dur


def queue_item(i, nw, batch):
    """item i of the queue's list -> (x, channel): rank-major, the ranks take x from the ends inwards (the kernel's rule)"""
    rank = i // batch
    return ((rank >> 1) if rank & 1 else nw - 1 - (rank >> 1)), i - rank * batch


class Queue:
    """the kernel's three counters"""
    def __init__(self, nw, batch):
        self.nw, self.batch, self.items = nw, batch, nw * batch
        self.claimed = self.head = self.tail = 0

    def claim(self, side):
        t = self.claimed; self.claimed += 1
        if t >= self.items: return None
        if side & 1:
            i = self.items - 1 - self.tail; self.tail += 1
        else:
            i = self.head; self.head += 1
        return queue_item(i, self.nw, self.batch)


def simulate(wgs, ncu, older, younger, log=None):
    """wgs: hardware workgroups in dispatch order, each (cu or None, next_item) with next_item() -> duration alone or None; a CU holds
    two; a workgroup without a CU takes the first slot that falls free.  Returns the time the last one ends."""
    slots = [[] for _ in range(ncu)]                 # per CU: [remaining, next_item, id] in the order of arrival
    pending = []
    now = 0.0

    def start(cu, k, nxt):
        d = nxt()
        if d is not None:
            slots[cu].append([d, nxt, k])
            if log is not None: log.append((k, cu, len(slots[cu]) - 1, now))

    for k, (cu, nxt) in enumerate(wgs):
        if cu is not None and len(slots[cu]) < 2: start(cu, k, nxt)
        else: pending.append((k, nxt))
    while True:
        best = None
        for cu, s in enumerate(slots):
            for j, w in enumerate(s):
                rate = 1.0 if len(s) == 1 else (older if j == 0 else younger)
                dt = w[0] / rate
                if best is None or dt < best[0]: best = (dt, cu, j)
        if best is None: return now
        dt, bcu, bj = best
        now += dt
        for cu, s in enumerate(slots):
            for j, w in enumerate(s):
                w[0] -= dt * (1.0 if len(s) == 1 else (older if j == 0 else younger))
        w = slots[bcu][bj]
        d = w[1]()                                   # the same hardware workgroup goes on with its next item and keeps its place
        if d is not None: w[0] = d
        else:
            slots[bcu].pop(bj)
            if pending:
                k, nxt = pending.pop(0); start(bcu, k, nxt)


def once(d):
    left = [d]
    return lambda: left.pop() if left else None


def unpaired(dur, nw, batch, ncu, older, younger):
    per_xcd = ncu // XCDS
    wgs, seen = [], [0] * XCDS
    for ch in range(batch):
        for x in range(nw):
            k = len(wgs); xcd = k % XCDS
            j = seen[xcd]; seen[xcd] += 1
            wgs.append((xcd * per_xcd + j % per_xcd if j < 2 * per_xcd else None, once(dur[x][ch])))
    return simulate(wgs, ncu, older, younger)


def paired(dur, nw, batch, ncu, older, younger):
    stride = (nw + 1) // 2
    wgs = []
    for ch in range(batch):
        for x in range(stride):
            todo = [dur[x2][ch] for x2 in (x + stride, x) if x2 < nw]
            k = len(wgs)
            wgs.append((k if k < ncu else None, (lambda t: (lambda: t.pop() if t else None))(todo)))
    return simulate(wgs, ncu, older, younger)


def queue(dur, nw, batch, ncu, older, younger, grid=0, handed=None):
    q = Queue(nw, batch)
    g = min(nw * batch, 2 * ncu)
    if grid: g = min(g, grid)

    def source(side):
        def nxt():
            it = q.claim(side)
            if it is None: return None
            if handed is not None: handed.append(it)
            return dur[it[0]][it[1]]
        return nxt
    # the first ncu workgroups are the first on their CUs, the next ncu the second
    return simulate([(k % ncu, source(k // ncu)) for k in range(g)], ncu, older, younger)


def durations_from_records(path):
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    import bisect_balance
    head, recs = bisect_balance.parse(open(path).read())
    tick_ms = 1.0 / float(head["wall_khz"])
    nw, batch = int(head["nw"]), int(head["batch"])
    dur = {x: [0.0] * batch for x in range(nw)}
    for r in recs:
        dur[r["x"]][r["ch"]] = (r["t1"] - r["t0"]) * tick_ms
    return dur, nw, batch


if __name__ == "__main__":
    args = sys.argv[1:]
    cus, grid, rates, records = 256, 0, r12_rates(), None
    while args:
        a = args.pop(0)
        if a == "--cus": cus = int(args.pop(0))
        elif a == "--grid": grid = int(args.pop(0))
        elif a == "--factor": f = float(args.pop(0)); rates = (1.0 / f, 1.0 / f)
        elif a == "--rates": rates = tuple(float(v) for v in args.pop(0).split(","))
        elif a == "--records": records = args.pop(0)
        elif a == "--r12": records = None
        else: sys.exit(__doc__)
    if records: dur, nw, batch = durations_from_records(records)
    else: dur, nw, batch = r12_durations(), 4, 128
    work = sum(sum(v) for v in dur.values())
    print("%d items (nw %d x %d channels), %.0f CU ms alone, %d CUs; two on a CU advance at %.3f (older) and %.3f (younger) of their rate alone"
          % (nw * batch, nw, batch, work, cus, rates[0], rates[1]))
    print("  unpaired launch: %.2f ms" % unpaired(dur, nw, batch, cus, *rates))
    print("  paired launch:   %.2f ms" % paired(dur, nw, batch, cus, *rates))
    print("  queue launch:    %.2f ms   (both slots of every CU full to the end: %.2f ms)"
          % (queue(dur, nw, batch, cus, *rates, grid=grid), work / (rates[0] + rates[1]) / cus))
