#!/usr/bin/env python
"""Launch time of the wide receding-horizon advance (dpilqr_policy_advance_dec_wide, csrc/policy_advance_dec_team.hpp at four
mask words) beside what the same result cost before it existed and beside the solve of the same round.  Nothing is asserted: nobody has measured this
kernel before, and no time is a pass criterion.

Workloads: DoubleIntDynamics4D teams of k = 65, 128 and 256 agents, T = 50, under a disturbance and control limits, neighbourhoods
of kc_max = 8 and 20 (groups of consecutive agents; the last group of a team is smaller), with 1, 32 and 256 scenarios and h = 1
and h = 5 executed steps.  The policy is synthetic (a resting nominal, small random gains): the kernel's work does not depend on
the values.  Per row:
  advance   ONE launch of policy_advance_dec_wide (h steps, floor(256 / k) scenarios per workgroup, the bookkeeping included)
  before    what produced the same state before: ONE one-sample policy_rollout_dec_wide over all T steps (W padded to the horizon,
            trajectories stored) plus the torch shift (U_next, X_next) and append (X_exec, U_exec, x_cur, n_done) -- without J_exec,
            min_sep of the prefix and dist_left, which the rollout does not give for a prefix
  solve     ONE solve_scenarios_distributed(policy="wide") of the same number of scenarios from a placement with exactly those
            neighbourhoods (groups on circles of radius 0.4, ten apart; graph radius 0.5), cold warm start -- the other part of a
            round of solve_rhc_closed_loop(centralized=False, wide=True); not started where it is projected past its budget
Then, at k = 64 (one word, both kernels serve it): policy_advance_dec_wide against policy_advance_dec_team, launched ALTERNATELY
inside one timed window each; and ProblemBatch.cost_wide at k = 256 (one point per scenario: the loop's terminal cost; one thread
per point, 32,640 serial pair terms).

A timed window is `inner` launches between two HIP events; the median, minimum and maximum of --reps windows after a warm-up, per
launch.  The solve: a host clock around one call that ends in a device synchronise, the median of three after a warm-up.  Every
workload runs in a child process under its own time limit and nothing more is started after a failure.
Not collected: hardware counters of any kind (occupancy, LDS bank conflicts, memory traffic), and no kernel trace.

    python scripts/bench_policy_advance_dec_wide.py [--reps 7] [--label COMMIT] [--out profiles/policy_advance_dec_wide.txt]"""
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

TEAMS = (65, 128, 256)
GROUPS = (8, 20)
WORKLOADS = {"%dxDoubleInt4D kc_max=%d" % (k, g): (k, g) for k in TEAMS for g in GROUPS}
EXTRA = ("k64 wide against team", "cost_wide k256")
NS, NC, T, DT, RADIUS = 4, 2, 50, 0.1, 0.5
SCENARIOS = (1, 32, 256)
HS = (1, 5)
INNER = 10            # launches per timed window
SOLVE_BUDGET = 20.0   # seconds: a solve projected past it (from the smaller scenario count) is not started
Q, R, QF = np.diag([1.0, 1.0, 0.5, 0.5]), np.eye(NC), 100.0 * np.eye(NS)


def placement(k, group, S, rng):
    """Groups of `group` consecutive agents on circles of radius 0.4 (longest chord 0.8 < 2 RADIUS), ten apart; goals a step away."""
    pos = np.zeros((S, k, 2))
    for a in range(k):
        ang = 2 * np.pi * (a % group) / group
        pos[:, a] = [10.0 * (a // group) + 0.4 * np.cos(ang), 0.4 * np.sin(ang)]
    pos += 0.01 * rng.normal(size=pos.shape)
    goal = pos + rng.uniform(0.6, 1.4, size=pos.shape) * rng.choice([-1.0, 1.0], size=pos.shape)
    st = lambda p: np.concatenate([p, np.zeros_like(p)], axis=2).reshape(S, k * NS)
    return st(pos), st(goal)


def group_words(k, group, S):
    """(S, k, n_words) uint64: agent a sees the agents of its group."""
    nw = (k + 63) // 64
    words = np.zeros((S, k, nw), dtype=np.uint64)
    for a in range(k):
        for j in range(group * (a // group), min(group * (a // group + 1), k)):
            words[:, a, j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return words


def _timed(torch, fn, reps, before=None, inner=INNER):
    fn(); torch.cuda.synchronize()      # warm-up
    ts = []
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def _synthetic(dp, torch, k, group, S, rng, x0, xf):
    n, m = k * NS, k * NC
    pb = dp.ProblemBatch([0] * k, [2] * k, xf, Q, R, QF, RADIUS, DT, T)
    dev = pb._xf.device
    X = torch.as_tensor(np.repeat(x0[:, None, :], T + 1, axis=1), device=dev)
    U = torch.zeros((S, T, m), dtype=torch.float64, device=dev)
    Kc = 1e-3 * torch.randn((S, T, k, NC, group * NS), dtype=torch.float64, device=dev)
    L = INNER * max(HS)
    W = dp.device.to_dev(1e-3 * rng.normal(size=(S, L, n)))
    u_lim = np.stack([np.full(m, -2.0), np.full(m, 2.0)])
    return pb, dev, X, U, Kc, L, W, u_lim


def one(name, reps):
    import torch
    import dpilqr_amd as dp
    if name == EXTRA[0]:
        return one_word(reps)
    if name == EXTRA[1]:
        return cost_wide(reps)
    k, group = WORKLOADS[name]
    n, m = k * NS, k * NC
    rng = np.random.default_rng(k + group)
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(DT, i) for i in ids])
    last_solve = None
    for S in SCENARIOS:
        x0, xf = placement(k, group, S, rng)
        pb, dev, X, U, Kc, L, W, u_lim = _synthetic(dp, torch, k, group, S, rng, x0, xf)
        bits = torch.as_tensor(group_words(k, group, S).view(np.int64), device=dev)
        state = pb.advance_state(x0, L)
        pb.policy_advance_dec_wide(X, U, Kc, bits, 1, state, W=W, u_lim=u_lim)      # the first call reads the masks back and checks them
        out = dict(name=name, S=S, k=k, kc_max=group, workgroups=-(-S // (256 // k)), h={}, before={}, solve=None)
        for h in HS:
            adv = _timed(torch, lambda: pb.policy_advance_dec_wide(X, U, Kc, bits, h, state, W=W, u_lim=u_lim, masks_checked=bits), reps,
                         before=lambda: state["n_done"].zero_())
            assert int(state["n_done"].min().item()) == INNER * h      # every launch of the last window executed h steps
            out["h"][h] = adv
            # before: the one-sample rollout over the whole horizon, then the shift and the append in torch
            Wp = torch.zeros((S, 1, T, n), dtype=torch.float64, device=dev)
            Wp[:, 0, :h] = W[:, :h]
            x_cur, Xe, Ue = state["x_cur"].clone(), state["X_exec"].clone(), state["U_exec"].clone()
            Un, Xn, done = state["U_next"].clone(), state["X_next"].clone(), torch.zeros((S,), dtype=torch.int32, device=dev)

            def old():
                r = pb.policy_rollout_dec_wide(X, U, Kc, bits, x_cur[:, None, :], W=Wp, u_lim=u_lim, trajectories=True, masks_checked=bits)
                Xe[:, :h + 1] = r["X"][:, 0, :h + 1]; Ue[:, :h] = r["U"][:, 0, :h]      # (at offset 0: the copy's size is what counts)
                x_cur.copy_(r["X"][:, 0, h]); done.add_(h)
                Un[:, :T - h] = U[:, h:]; Un[:, T - h:] = 0.0
                Xn[:, 0] = x_cur; Xn[:, 1:T - h + 1] = X[:, h + 1:]; Xn[:, T - h + 1:] = X[:, T:]
            out["before"][h] = _timed(torch, old, reps)
        if last_solve is not None and last_solve[1] * S / last_solve[0] > SOLVE_BUDGET:
            out["solve"] = "not measured: projected past %d s from %d scenarios" % (SOLVE_BUDGET, last_solve[0])
        else:
            costs = [dp.ReferenceCost(xf[0][NS * i:NS * (i + 1)], Q, R, QF, id_) for i, id_ in enumerate(ids)]
            problem = dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([NS] * k, RADIUS, [2] * k)))
            U0 = np.zeros((S, T, m))
            try:
                def solve():
                    t0 = time.perf_counter()
                    _, _, _, info = dp.solve_scenarios_distributed(problem, x0[:, None, :], U0, RADIUS, xf=xf, device_out=True, policy="wide")
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, info
                _, info = solve()      # warm-up
                ts = [solve()[0] for _ in range(3)]
                out["solve"] = dict(ms=[1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)], kc_max=int(info["policy"].kc_max))
                last_solve = (S, statistics.median(ts))
            except (ValueError, NotImplementedError) as e:      # a refusal on the host, in the library's own words
                out["solve"] = "not served: " + str(e).splitlines()[0][:160]
            except dp._lib.DpilqrError as e:                    # ... or of the C entry before any launch; anything else ends the child
                if e.code != dp._lib.EUNSUPPORTED:
                    raise
                out["solve"] = "not served: " + str(e).splitlines()[0][:160]
        print(json.dumps(out), flush=True)


def one_word(reps):
    """k = 64, every agent sees its group of 8: the wide and the team advance alternately inside each window."""
    import torch
    import dpilqr_amd as dp
    k, group = 64, 8
    rng = np.random.default_rng(64)
    for S in SCENARIOS:
        x0, xf = placement(k, group, S, rng)
        pb, dev, X, U, Kc, L, W, u_lim = _synthetic(dp, torch, k, group, S, rng, x0, xf)
        words = torch.as_tensor(group_words(k, group, S).view(np.int64), device=dev)
        masks = words[:, :, 0].contiguous()
        sw_, st_ = pb.advance_state(x0, L), pb.advance_state(x0, L)
        pb.policy_advance_dec_wide(X, U, Kc, words, 1, sw_, W=W, u_lim=u_lim); pb.policy_advance_dec_team(X, U, Kc, masks, 1, st_, W=W, u_lim=u_lim)
        for h in HS:
            wide = lambda: pb.policy_advance_dec_wide(X, U, Kc, words, h, sw_, W=W, u_lim=u_lim, masks_checked=words)
            team = lambda: pb.policy_advance_dec_team(X, U, Kc, masks, h, st_, W=W, u_lim=u_lim, masks_checked=masks)
            wide(); team(); torch.cuda.synchronize()
            tw, tt = [], []
            for _ in range(reps):
                sw_["n_done"].zero_(); st_["n_done"].zero_()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * INNER + 1)]
                ev[0].record()
                for i in range(INNER):      # alternately: wide, team, wide, team ...
                    wide(); ev[2 * i + 1].record(); team(); ev[2 * i + 2].record()
                torch.cuda.synchronize()
                tw.append(sum(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(INNER)) / INNER)
                tt.append(sum(ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(INNER)) / INNER)
            same = all(bool(torch.equal(sw_[f], st_[f])) for f in ("X_exec", "U_exec", "J_exec", "x_cur"))
            stat = lambda t: (statistics.median(t), min(t), max(t))
            print(json.dumps(dict(name=EXTRA[0], S=S, h=h, wide=stat(tw), team=stat(tt), same_bits=same)), flush=True)


def cost_wide(reps):
    import torch
    import dpilqr_amd as dp
    k = 256
    rng = np.random.default_rng(256)
    for S in SCENARIOS:
        x0, xf = placement(k, 8, S, rng)
        pb = dp.ProblemBatch([0] * k, [2] * k, xf, Q, R, QF, RADIUS, DT, T)
        x = dp.device.to_dev(x0[:, None, :]); u = torch.zeros((S, 1, k * NC), dtype=torch.float64, device=x.device)
        t = _timed(torch, lambda: pb.cost_wide(x, u, terminal=True), reps)
        print(json.dumps(dict(name=EXTRA[1], S=S, ms=t)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="unlabelled", help="the commit the figures are taken at")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance_dec_wide.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per workload")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.reps)
    fmt = lambda t: "%8.4f (%7.4f..%7.4f)" % tuple(t)
    lines = ["wide receding-horizon advance (dpilqr_policy_advance_dec_wide): DoubleIntDynamics4D teams, T = %d, under W and u_lim; commit: %s" % (T, a.label),
             "advance: ONE launch (h steps, floor(256 / k) scenarios per workgroup, the bookkeeping included); per launch: median (min .. max) ms",
             "         of %d windows of %d launches after a warm-up, HIP events" % (a.reps, INNER),
             "before:  ONE one-sample policy_rollout_dec_wide over all T steps, trajectories stored, plus the torch shift and append; the same windows",
             "solve:   ONE solve_scenarios_distributed(policy=\"wide\") of the same scenarios, cold warm start, host clock to a device synchronise,",
             "         median (min .. max) ms of three after a warm-up; kc_max: the largest neighbourhood its graph found",
             "share:   advance / (solve + advance) of one receding-horizon round",
             "not collected: hardware counters (occupancy, LDS conflicts, memory traffic), kernel traces",
             "%-26s %4s %4s %2s %28s %28s %8s   %s" % ("team", "S", "wgs", "h", "advance ms", "before ms", "share", "solve ms")]
    rc = 0
    for name in list(WORKLOADS) + list(EXTRA):
        try:
            p = subprocess.run([sys.executable, __file__, "--one", name, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
            rc, err, got = p.returncode, p.stderr.strip().splitlines()[-1:], p.stdout
        except subprocess.TimeoutExpired as e:
            rc, err, got = 124, ["time limit of %d s" % a.limit], (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        for row in got.strip().splitlines():
            if not row.startswith("{"):
                continue
            d = json.loads(row)
            if d["name"] == EXTRA[0]:
                lines.append("k = 64, kc_max = 8, alternately in one window: S %4d h %s  wide %s  team %s  wide / team %.3f  same bits: %s"
                             % (d["S"], d["h"], fmt(d["wide"]), fmt(d["team"]), d["wide"][0] / d["team"][0], d["same_bits"]))
            elif d["name"] == EXTRA[1]:
                lines.append("cost_wide, k = 256, one point per scenario (terminal): S %4d  %s ms per call" % (d["S"], fmt(d["ms"])))
            else:
                for h, adv in d["h"].items():
                    sv = d["solve"]
                    if isinstance(sv, dict):
                        share, txt = "%7.3f%%" % (100.0 * adv[0] / (sv["ms"][0] + adv[0])), "%10.2f (%9.2f..%9.2f)  kc_max %d" % (*sv["ms"], sv["kc_max"])
                    else:
                        share, txt = "%8s" % "-", sv
                    lines.append("%-26s %4d %4d %2s %28s %28s %8s   %s" % (d["name"], d["S"], d["workgroups"], h, fmt(adv), fmt(d["before"][h]), share, txt))
        if rc != 0:      # nothing more is started on the device after a failure
            lines.append(f"{name}: exit status {rc}: {err}")
            break
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main())
