#!/usr/bin/env python
"""What the capped graph (dpilqr_dispatch_graph_nearest, csrc/frontend_nearest.hpp) costs beside the uncapped one
(dpilqr_dispatch_graph_wide), and what a cap buys a dense team's solve.  Nothing is asserted and no target is set: the front end is
at most a per-cent of a round beside solves of tens to hundreds of milliseconds.

Graph entries: DoubleIntDynamics4D teams of k = 65, 128 and 256 agents, S = 1, 32 and 256 scenarios, trajectories of 11 rows (all
sampled).  Two kinds of scenario:
  sparse   the lattice of tests/swarm_cases.py (spacing 3.0, graph radius 0.5, neighbourhoods of at most a handful) with m = 64: the
           cap never bites, the ranking branch is never taken -- the price of holding the keys
  dense    the lattice of tests/nearest_cases.py (spacing 0.9, graph radius 4.0, near-cliques) with m = 8: the cap bites for every
           agent, every wavefront ranks its candidates
Both entries run in ONE process on the same buffers, alternately, one HIP-event pair around each call (graph + de-duplication +
bucket sort: the whole entry); per figure the median (min .. max) of --reps calls after a warm-up.  On a dense scenario the uncapped
entry's masks are not plannable (clusters beyond 64); its time is the yardstick all the same.
Whole solves: solve_scenarios_distributed(max_cluster=m) on the k = 130 dense lattice (tests/nearest_cases.py), S = 2, T = 8, for
m = 2, 4, 8, 16: wall-clock seconds, median (min .. max) of 3 calls after a warm-up, with the front end's share.

    python scripts/bench_nearest.py [--reps 15] [--out profiles/nearest_graph.txt]"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TEAMS, BATCHES, ROWS, NS = (65, 128, 256), (1, 32, 256), 11, 4


def scenarios(kind, k, S):
    """X (S, ROWS, k * 4) and the graph's radius"""
    import numpy as np
    from tests import nearest_cases as nc
    from tests import swarm_cases as sw
    rng = np.random.default_rng(17 * k + S)
    if kind == "sparse":
        p, radius, jitter = sw.positions(k, sw.OFFSET_SOLVE), sw.RADIUS, 0.15
    else:
        p, radius, jitter = nc.scenario(k)[0][0].reshape(k, NS)[:, :2], nc.GRAPH_RADIUS, 0.05
    x0 = np.zeros((S, k, NS)); x0[:, :, :2] = p[None] + rng.uniform(-jitter, jitter, size=(S, k, 2))
    move = np.zeros((S, k, NS)); move[:, :, :2] = rng.uniform(-0.15, 0.15, size=(S, k, 2))
    X = x0[:, None] + np.linspace(0.0, 1.0, ROWS)[None, :, None, None] * move[:, None]
    return X.reshape(S, ROWS, k * NS), radius


def graph_times(reps):
    import numpy as np
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import device, ptr, stream_handle, to_dev
    L = _lib.load()
    lines = []
    for kind, m in (("sparse", 64), ("dense", 8)):
        for k in TEAMS:
            for S in BATCHES:
                X, radius = scenarios(kind, k, S)
                nw = (k + 63) // 64
                Xd, rad = to_dev(X), to_dev(np.full(S, radius))
                bits = torch.zeros((S * k, nw), dtype=torch.int64, device=device())
                rep, size, order, slot, dropped = (torch.zeros((S * k,), dtype=torch.int32, device=device()) for _ in range(5))
                bstart, bcount = (torch.zeros((k + 1,), dtype=torch.int32, device=device()) for _ in range(2))
                head = (S, ROWS, k, NS, ptr(Xd), ptr(rad), 1, None)
                tail = (ptr(bits), ptr(rep), ptr(size), ptr(order), ptr(slot), ptr(bstart), ptr(bcount))
                wide = lambda: _lib.check(L.dpilqr_dispatch_graph_wide(*head, *tail, nw, stream_handle()))
                near = lambda: _lib.check(L.dpilqr_dispatch_graph_nearest(*head, m, *tail, ptr(dropped), nw, stream_handle()))
                wide(); near(); torch.cuda.synchronize()
                bitten = int((dropped > 0).sum().item())
                largest = int(size.max().item())
                tw, tn = [], []
                for _ in range(reps):      # alternately, in the same window
                    for fn, ts in ((wide, tw), (near, tn)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                        ts.append(1e3 * e0.elapsed_time(e1))
                f = lambda ts: "%8.1f (%7.1f ..%8.1f)" % (statistics.median(ts), min(ts), max(ts))
                lines.append("%-6s %4d %4d %3d  %s  %s  %5.2f  %7d of %-6d %4d" % (kind, k, S, m, f(tw), f(tn), statistics.median(tn) / statistics.median(tw),
                                                                                bitten, S * k, largest))
    return lines


def solve_times():
    import time
    import numpy as np
    import torch
    import dpilqr_amd as dp
    from tests import nearest_cases as nc
    from tests.test_gpu_swarm import dp_problem
    k, S, T = 130, 2, 8
    x0, xf, _ = nc.scenario(k)
    prob = dp_problem(dp, nc.Case(k, 5), xf[0])
    X, U0 = x0[:S, None, :], np.zeros((S, T, k * nc.NC))
    lines = []
    for m in (2, 4, 8, 16):
        ts, front = [], []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, J, info = dp.solve_scenarios_distributed(prob, X, U0, nc.GRAPH_RADIUS, xf=xf[:S], max_cluster=m, n_lqr_iter=nc.N_LQR_ITER)
            if i:      # the first call warms up
                ts.append(time.perf_counter() - t0); front.append(info["seconds"]["front_end"])
        lines.append("%3d  %8.4f (%7.4f ..%8.4f)  %8.5f  %5d  %-28s %8d  %s" % (m, statistics.median(ts), min(ts), max(ts), statistics.median(front), info["n_unique"],
                                                                              info["sizes"], int(info["n_dropped"].sum()), np.array2string(J, precision=2)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nearest_graph.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build(verbose=False)
    lines = ["capped graph (dpilqr_dispatch_graph_nearest) beside the uncapped one (dpilqr_dispatch_graph_wide): DoubleIntDynamics4D, trajectories of "
             "%d rows, all sampled; microseconds per call of the whole entry (graph, de-duplication, bucket sort), median (min .. max) of %d calls "
             "after a warm-up, the two entries alternating in one process (HIP events)" % (ROWS, a.reps),
             "%-6s %4s %4s %3s  %-27s  %-27s  %5s  %-17s %4s" % ("kind", "k", "S", "m", "graph_wide us", "graph_nearest us", "ratio", "agents the cap bit",
                                                                 "largest capped cluster")]
    lines += graph_times(a.reps)
    lines += ["", "whole solves: solve_scenarios_distributed(max_cluster=m), k = 130 dense lattice (uncapped: refused, neighbourhoods of 70 .. 130), S = 2, T = 8; "
              "wall-clock seconds, median (min .. max) of 3 calls after a warm-up",
              "%3s  %-28s  %8s  %5s  %-28s %8s  %s" % ("m", "seconds", "front end", "sub-problems", "sizes", "dropped", "J_full")]
    lines += solve_times()
    lines += ["", "measured: the figures above.  The sort's single workgroup (k_bucket_sort_wide) is part of both entries' times and grows with S k.",
              "not measured: hardware counters (LDS bank conflicts, occupancy) for k_graph_bits_nearest; other model families (the graph reads two "
              "coordinates per agent whatever the family); N = 1 calls (one row instead of 11); teams of k <= 64 against dispatch_graph; the solve "
              "times of sparse teams, which a cap that never bites leaves as they are."]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
