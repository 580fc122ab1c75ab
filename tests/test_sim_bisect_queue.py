"""tools/sim_bisect_queue.py (CPU): the list-scheduling model of bisect3_kernel's launches reproduces the two kernel times that
profiles/r12_bisect_pairs.txt measured -- before its prediction for the queue launch is quoted anywhere -- and the queue's claim order
(the Python restatement of the kernel's rule) hands every item out exactly once."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("sim_bisect_queue", os.path.join(ROOT, "tools", "sim_bisect_queue.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def test_reproduces_the_measured_unpaired_and_paired_launches(sim):
    """fed the r12 figures (per-x time alone, the two co-residency rates from the sharing / alone ratios) the model must give the
    measured 10.88 ms (unpaired) and 9.82 ms (paired) to within 10 %"""
    dur = sim.r12_durations()
    older, younger = sim.r12_rates()
    assert 0 < younger < older < 1
    for x, (mean, lo, hi) in sim.R12_ALONE.items():
        assert abs(sum(dur[x]) / len(dur[x]) - mean) < 0.01 and min(dur[x]) == lo and abs(max(dur[x]) - hi) < 1e-12
    t_unpaired = sim.unpaired(dur, 4, 128, 256, older, younger)
    t_paired = sim.paired(dur, 4, 128, 256, older, younger)
    print("unpaired %.2f (measured %.2f)  paired %.2f (measured %.2f)" % (t_unpaired, sim.R12_UNPAIRED_MS, t_paired, sim.R12_PAIRED_MS))
    assert abs(t_unpaired / sim.R12_UNPAIRED_MS - 1) < 0.10
    assert abs(t_paired / sim.R12_PAIRED_MS - 1) < 0.10
    # the queue can do no better than both slots of every CU full to the end, and should not do worse than the pairs
    t_queue = sim.queue(dur, 4, 128, 256, older, younger)
    floor = sum(sum(v) for v in dur.values()) / (older + younger) / 256
    assert floor <= t_queue < t_paired


def test_item_order(sim):
    """ends of the spectrum first, rank-major: at nw = 4 the x order is 3, 0, 2, 1, within a rank the channels in turn"""
    assert [sim.queue_item(i, 4, 1)[0] for i in range(4)] == [3, 0, 2, 1]
    assert [sim.queue_item(i, 5, 1)[0] for i in range(5)] == [4, 0, 3, 1, 2]
    assert [sim.queue_item(i, 3, 2) for i in range(6)] == [(2, 0), (2, 1), (0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("nw,batch,grid", [(4, 128, 0), (4, 128, 7), (3, 3, 1), (3, 3, 2), (3, 3, 5), (9, 2, 3), (2, 3, 0), (1, 5, 4), (5, 67, 40)])
def test_every_item_is_handed_out_exactly_once(sim, nw, batch, grid):
    # durations that differ from item to item, so that head and tail claims interleave
    dur = {x: [1.0 + ((7 * x + 3 * c) % 11) / 5.0 for c in range(batch)] for x in range(nw)}
    for ncu in (1, 4, 256):
        handed = []
        sim.queue(dur, nw, batch, ncu, 0.9, 0.3, grid=grid, handed=handed)
        assert sorted(handed) == [(x, c) for x in range(nw) for c in range(batch)]
    q = sim.Queue(nw, batch)
    for _ in range(nw * batch):
        q.claim(_ % 3)
    assert q.claim(0) is None and q.claim(1) is None and q.head + q.tail == nw * batch
