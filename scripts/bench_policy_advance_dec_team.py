#!/usr/bin/env python
"""Launch time of the team receding-horizon advance (dpilqr_policy_advance_dec_team, csrc/policy_advance_dec_team.hpp) beside the
solve of the same round.  Nothing is asserted: nobody has measured this kernel before, and no time is a pass criterion.

Workloads: DoubleIntDynamics4D teams, T = 50, under a disturbance and control limits, with 1, 32 and 256 scenarios and h = 1 and
h = 5 executed steps:
  24 agents, kc_max = 8   three cliques of eight (agent a sees the eight agents of its clique)        n_x = 96
  64 agents, full         every agent sees all 64 (the mask is -1 as int64)                           n_x = 256
The policy the advance is timed with is synthetic (a resting nominal, small random gains): the kernel's work does not depend on
the values.  Beside each figure: ONE solve_scenarios_distributed(policy=True) of the same number of scenarios from a placement
with exactly those neighbourhoods (cliques on circles of radius 0.4, ten apart; graph radius 0.5), cold warm start -- the other
part of a round of solve_rhc_closed_loop(centralized=False, team=True) -- and the advance's share of the two.  Where the solve of
a workload is refused or would run past its budget the column says so and the advance stands alone.

A timed window is `inner` launches between two HIP events (a single launch at one scenario is too short to time alone); the
median, minimum and maximum of --reps windows after a warm-up, per launch.  The solve: a host clock around one call that ends in
a device synchronise, the median of three after a warm-up.  Every workload runs in a child process under its own time limit and
nothing more is started after a failure.

    python scripts/bench_policy_advance_dec_team.py [--reps 9] [--label COMMIT] [--out profiles/policy_advance_dec_team.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {"24xDoubleInt4D kc_max=8": (24, 8), "64xDoubleInt4D full": (64, 64)}
NS, NC, T, DT, RADIUS = 4, 2, 50, 0.1, 0.5
SCENARIOS = (1, 32, 256)
HS = (1, 5)
INNER = 20            # launches per timed window
SOLVE_BUDGET = 60.0   # seconds: a solve projected past it (from the smaller scenario count) is not started


def placement(k, clique, S, rng):
    """Cliques of `clique` agents on circles of radius 0.4 (longest chord 0.8 < 2 RADIUS), ten apart; goals a step away."""
    pos = np.zeros((S, k, 2))
    for a in range(k):
        ang = 2 * np.pi * (a % clique) / clique
        pos[:, a] = [10.0 * (a // clique) + 0.4 * np.cos(ang), 0.4 * np.sin(ang)]
    pos += 0.01 * rng.normal(size=pos.shape)
    goal = pos + rng.uniform(0.6, 1.4, size=pos.shape) * rng.choice([-1.0, 1.0], size=pos.shape)
    st = lambda p: np.concatenate([p, np.zeros_like(p)], axis=2).reshape(S, k * NS)
    return st(pos), st(goal)


def one(name, reps):
    import torch
    import dpilqr_amd as dp
    k, clique = WORKLOADS[name]
    n, m = k * NS, k * NC
    rng = np.random.default_rng(k)
    Q, R, Qf = np.diag([1.0, 1.0, 0.5, 0.5]), np.eye(NC), 100.0 * np.eye(NS)

    def timed(fn, before=None):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / INNER)
        return statistics.median(ts), min(ts), max(ts)

    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(DT) for _ in range(k)])
    last_solve = None
    for S in SCENARIOS:
        x0, xf = placement(k, clique, S, rng)
        pb = dp.ProblemBatch([0] * k, [2] * k, xf, Q, R, Qf, RADIUS, DT, T)
        dev = pb._xf.device
        X = torch.as_tensor(np.repeat(x0[:, None, :], T + 1, axis=1), device=dev)
        U = torch.zeros((S, T, m), dtype=torch.float64, device=dev)
        masks = np.zeros((S, k), dtype=np.uint64)
        for a in range(k):
            masks[:, a] = np.uint64(sum(1 << (clique * (a // clique) + j) for j in range(clique)))
        bits = torch.as_tensor(masks.view(np.int64), device=dev)
        Kc = torch.as_tensor(1e-3 * rng.normal(size=(S, T, k, NC, clique * NS)), device=dev)
        L = INNER * max(HS)
        W = dp.device.to_dev(1e-3 * rng.normal(size=(S, L, n)))
        u_lim = np.stack([np.full(m, -2.0), np.full(m, 2.0)])
        state = pb.advance_state(x0, L)
        pb.policy_advance_dec_team(X, U, Kc, bits, 1, state, W=W, u_lim=u_lim)      # the first call reads the masks back and checks them
        out = dict(name=name, S=S, k=k, n_x=n, kc_max=clique, workgroups=-(-S // (256 // k)), h={}, solve=None)
        for h in HS:
            adv = timed(lambda: pb.policy_advance_dec_team(X, U, Kc, bits, h, state, W=W, u_lim=u_lim, masks_checked=bits),
                        before=lambda: state["n_done"].zero_())
            assert int(state["n_done"].min().item()) == INNER * h      # every launch of the last window executed h steps
            out["h"][h] = adv
        # the round's solve: the same scenarios, a placement with exactly these neighbourhoods
        if last_solve is not None and last_solve[1] * S / last_solve[0] > SOLVE_BUDGET:
            out["solve"] = "not measured: projected past %d s from %d scenarios" % (SOLVE_BUDGET, last_solve[0])
        else:
            costs = [dp.ReferenceCost(xf[0][NS * i:NS * (i + 1)], Q, R, Qf, i) for i in range(k)]
            problem = dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([NS] * k, RADIUS, [2] * k)))
            U0 = np.zeros((S, T, m))
            try:
                def solve():
                    t0 = time.perf_counter()
                    _, _, _, info = dp.solve_scenarios_distributed(problem, x0[:, None, :], U0, RADIUS, xf=xf, device_out=True, policy=True)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, info
                _, info = solve()      # warm-up
                cb = info.get("cluster_bits")
                cb = cb.cpu().numpy() if isinstance(cb, torch.Tensor) else np.asarray([] if cb is None else cb)
                sizes = sorted({bin(int(v)).count("1") for v in cb.astype(np.uint64).reshape(-1)})
                ts = [solve()[0] for _ in range(3)]
                out["solve"] = dict(ms=[1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)], sizes=sizes)
                last_solve = (S, statistics.median(ts))
            except (ValueError, NotImplementedError) as e:      # a refusal on the host, in the library's own words
                out["solve"] = "not served: " + str(e).splitlines()[0][:160]
            except dp._lib.DpilqrError as e:                    # ... or of the C entry before any launch; anything else ends the child
                if e.code != dp._lib.EUNSUPPORTED:
                    raise
                out["solve"] = "not served: " + str(e).splitlines()[0][:160]
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--label", default="unlabelled", help="the commit the figures are taken at")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance_dec_team.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds per workload")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.reps)
    fmt = lambda t: "%8.4f (%7.4f..%7.4f)" % tuple(t)
    lines = ["team receding-horizon advance (dpilqr_policy_advance_dec_team): DoubleIntDynamics4D teams, T = %d, under W and u_lim; commit: %s" % (T, a.label),
             "advance: ONE launch (h steps, floor(256 / k) scenarios per workgroup, the bookkeeping included); per launch: median (min .. max) ms",
             "         of %d windows of %d launches after a warm-up, HIP events" % (a.reps, INNER),
             "solve:   ONE solve_scenarios_distributed(policy=True) of the same scenarios, cold warm start, host clock to a device synchronise,",
             "         median (min .. max) ms of three after a warm-up; sizes: the neighbourhood sizes its graph found",
             "share:   advance / (solve + advance) of one receding-horizon round",
             "%-24s %5s %4s %2s %28s %8s   %s" % ("team", "S", "wgs", "h", "advance ms", "share", "solve ms")]
    rc = 0
    for name in WORKLOADS:
        try:
            p = subprocess.run([sys.executable, __file__, "--one", name, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
            rc, err, got = p.returncode, p.stderr.strip().splitlines()[-1:], p.stdout
        except subprocess.TimeoutExpired as e:
            rc, err, got = 124, ["time limit of %d s" % a.limit], (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        for row in got.strip().splitlines():
            if not row.startswith("{"):
                continue
            d = json.loads(row)
            for h, adv in d["h"].items():
                sv = d["solve"]
                if isinstance(sv, dict):
                    share, txt = "%7.3f%%" % (100.0 * adv[0] / (sv["ms"][0] + adv[0])), "%10.2f (%9.2f..%9.2f)  sizes %s" % (*sv["ms"], sv["sizes"])
                else:
                    share, txt = "%8s" % "-", sv
                lines.append("%-24s %5d %4d %2s %28s %8s   %s" % (d["name"], d["S"], d["workgroups"], h, fmt(adv), share, txt))
        if rc != 0:      # nothing more is started on the device after a failure
            lines.append(f"{name}: exit status {rc}: {err}")
            break
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main())
