#!/usr/bin/env python
"""Time of the dispatch front end and of J_full for large teams.  Nothing is asserted.

Cases: S = 1024 scenarios of k DoubleIntDynamics4D agents, T = 10 -- k = 64 on the one-word entries (dpilqr_dispatch_graph,
dpilqr_rollout), k = 128 and k = 256 on the wide entries (dpilqr_dispatch_graph_wide, dpilqr_rollout_wide).  The agents stand on
the lattice of tests/swarm_cases.py (spacing 3.0, its partners and its triple) with N(0, 0.5) planar jitter per scenario, so that
neighbourhoods of several sizes occur; the graph radius is 0.5.
  front end   ScenarioFrontEnd from device tensors: graph, de-duplication, bucket sort, and the one host read of the k + 1 bucket
              counts (wall clock around a synchronised call); from the scenarios' states (1 row) and from trajectories (11 rows)
  J_full      dispatch.full_rollout_cost of given controls on the full team (HIP events)
Per row: median (min .. max) of --reps runs after a warm-up.

    python scripts/bench_swarm.py [--reps 7] [--scenarios 1024] [--out profiles/swarm_dispatch.txt]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

T, RADIUS = 10, 0.5


def case(k, S, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    from dpilqr_amd.dispatch import ScenarioFrontEnd, full_rollout_cost
    from dpilqr_amd.lowering import describe
    from tests import swarm_cases as sw
    rng = np.random.default_rng(k)
    x0 = np.zeros((S, k, 4)); x0[:, :, :2] = sw.positions(k, 0.6)[None] + rng.normal(scale=0.5, size=(S, k, 2))
    xf = x0[0].copy(); xf[:, :2] += rng.uniform(-0.4, 0.4, size=(k, 2))
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(0.1, i) for i in ids])
    refs = [dp.ReferenceCost(xf[a], np.diag([1.0, 1, 0, 0]), np.eye(2), 1000.0 * np.eye(4), i) for a, i in enumerate(ids)]
    d = describe(dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([4] * k, RADIUS, [2] * k))))
    dev = torch.device("cuda")
    X1 = torch.as_tensor(x0.reshape(S, 1, -1), device=dev)
    drift = torch.as_tensor(rng.uniform(-1.0, 1.0, size=(S, 1, k * 4)), device=dev) * torch.linspace(0, 1, T + 1, device=dev, dtype=torch.float64)[None, :, None]
    XT = (X1 + drift).contiguous()
    U = 0.5 * torch.randn((S, T, k * 2), dtype=torch.float64, device=dev)

    def wall(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts), min(ts), max(ts)

    def events(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    fe = ScenarioFrontEnd(d, X1, U, RADIUS, None)
    sizes = {c: int(fe.counts[c]) for c in fe.sizes()}
    f1 = wall(lambda: ScenarioFrontEnd(d, X1, U, RADIUS, None))
    fT = wall(lambda: ScenarioFrontEnd(d, XT, U, RADIUS, None))
    jf = events(lambda: full_rollout_cost(d, fe, U))
    return dict(k=k, path="wide" if fe.wide else "narrow", n_words=fe.n_words, sizes=sizes, front_1=f1, front_T=fT, j_full=jf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "swarm_dispatch.txt"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least five runs")
    fmt = lambda t: "%9.3f (%8.3f .. %8.3f)" % t
    lines = ["dispatch front end and J_full for large teams: %d scenarios of k DoubleIntDynamics4D agents, T = %d; ms, median (min .. max) "
             "of %d runs after a warm-up" % (a.scenarios, T, a.reps),
             "front end: wall clock of ScenarioFrontEnd from device tensors, the host read of the bucket counts included; J_full: HIP events",
             "%4s %-7s %5s  %-32s %-32s %-32s" % ("k", "path", "words", "front end, 1 row", "front end, %d rows" % (T + 1), "J_full")]
    for k in (64, 128, 256):
        r = case(k, a.scenarios, a.reps)
        lines.append("%4d %-7s %5d  %-32s %-32s %-32s" % (k, r["path"], r["n_words"], fmt(r["front_1"]), fmt(r["front_T"]), fmt(r["j_full"])))
        lines.append("     unique sub-problems by cluster size: %s" % r["sizes"])
        Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
