#!/usr/bin/env python
"""Launch time of the receding-horizon advance for large clusters (dpilqr_policy_advance_large, csrc/policy_advance_large.hpp) at
BASELINE config 5's shape (14 x Quadcopter12D + 6 x padded HumanDynamics6D, n_x = 240, n_u = 80, T = 150) with 1, 32 and 256
scenarios, h = 1 and h = 5, under a disturbance and control limits.  Beside each figure, both existing code: dpilqr_policy_rollout_large
of the same items with ONE sample over the whole horizon (trajectories stored) -- what the executed prefix cost before the advance
existed, without the bookkeeping -- and one round's solve (ProblemBatch.solve from a cold warm start) and gains (backward_pass).
Reported: the launch as a share of the round, advance / (solve + gains + advance), and the rate at which K is streamed: every
workgroup reads its item's K[i], n_u n_x 8 = 153.6 KB, once per step, so a launch reads S h 153.6 KB; at S = 1 that rate is what
ONE compute unit streams.  No target: the file is the record.

Every scenario count runs in a child process under its own time limit and nothing more is started after a failure.  A timed
window is `inner` launches between two HIP events (a single launch at S = 1 is too short to time alone); the median, minimum and
maximum of --reps windows after a warm-up, per launch.

    python scripts/bench_policy_advance_large.py [--reps 9] [--out profiles/policy_advance_large.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODELS, N_DIMS, T, DT = [7] * 14 + [8] * 6, [3] * 14 + [2] * 6, 150, 0.05
SCENARIOS = (1, 32, 256)
HS = (1, 5)
INNER = 20      # launches per timed window


def one(S, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    k = len(MODELS)
    ns, nc = dp.batch.MODEL_DIMS[MODELS[0]]
    n, m = k * ns, k * nc
    rng = np.random.default_rng(5)
    xf = rng.normal(size=(S, n)) * 1.5; x0 = rng.normal(size=(S, n)) * 1.5
    x0.reshape(S, k, ns)[:, :, 3:] *= 0.1 * 0.02; xf.reshape(S, k, ns)[:, :, 3:] = 0.0      # near hover (scripts/bench_policy_large.py)
    U0 = rng.normal(size=(S, T, m)) * 0.05 * 1e-4; U0[:, :, 3::4] += 9.80665 * 63.0 / 2000.0
    pb = dp.ProblemBatch(MODELS, N_DIMS, xf, np.eye(ns), np.eye(nc), 100.0 * np.eye(ns), 0.5, DT, T)
    L = INNER * max(HS)
    W = dp.device.to_dev(1e-3 * rng.normal(size=(S, L, n)))
    u_lim = np.stack([np.full(m, -2.0), np.full(m, 2.0)]); u_lim[:, 3::4] += 9.80665 * 63.0 / 2000.0

    def timed(fn, before=None, reps_=reps, inner=1):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps_):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / inner)
        return statistics.median(ts), min(ts), max(ts)

    x0d, U0d = dp.device.to_dev(x0), dp.device.to_dev(U0)
    sol = pb.solve(x0d, U0d)
    X, U = sol["X"], sol["U"]
    n_bwd = float(sol["n_bwd"].double().mean().item())
    K = pb.backward_pass(X, U, 0.0)[0]
    solve_ms = timed(lambda: pb.solve(x0d, U0d), reps_=3)
    gains_ms = timed(lambda: pb.backward_pass(X, U, 0.0), reps_=5)
    state = pb.advance_state(x0, L)
    x0s = x0d[:, None, :].contiguous()
    out = dict(S=S, k=k, T=T, n_x=n, n_u=m, solve_ms=solve_ms, gains_ms=gains_ms, n_bwd=n_bwd, h={})
    for h in HS:
        adv = timed(lambda: pb.policy_advance_large(X, U, K, h, state, W=W, u_lim=u_lim), before=lambda: state["n_done"].zero_(), inner=INNER)
        assert int(state["n_done"].min().item()) == INNER * h      # every launch of the last window executed h steps
        Wp = torch.zeros((S, 1, T, n), dtype=torch.float64, device=X.device); Wp[:, 0, :h] = W[:, :h]
        roll = timed(lambda: pb.policy_rollout_large(X, U, K, x0s, W=Wp, u_lim=u_lim, trajectories=True), inner=5)
        out["h"][h] = dict(advance_ms=adv, rollout_ms=roll)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance_large.txt"))
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per scenario count")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.reps)
    fmt = lambda t: "%8.4f (%7.4f..%7.4f)" % tuple(t)
    lines = ["receding-horizon advance for large clusters at BASELINE config 5's shape (n_x = 240, n_u = 80, T = 150) under W and u_lim",
             "per launch: median (min .. max) ms of %d windows of %d launches after a warm-up, HIP events" % (a.reps, INNER),
             "advance: ONE dpilqr_policy_advance_large launch (h steps, one workgroup per scenario, the bookkeeping included)",
             "rollout: dpilqr_policy_rollout_large, one sample per item, all T steps, trajectories stored (windows of 5 launches)",
             "solve, gains: ProblemBatch.solve from a cold warm start (3 repetitions; mean backward passes per item beside it), backward_pass",
             "share:   advance / (solve + gains + advance) of one receding-horizon round",
             "K GB/s:  S h n_u n_x 8 bytes over the launch time (K[i] once per workgroup and step); /wg: per workgroup -- at S = 1, what one CU streams",
             "%5s %2s %28s %28s %7s %26s %8s %10s %7s %9s %8s" % ("S", "h", "advance ms", "rollout ms", "ratio", "solve ms", "n_bwd", "gains ms",
                                                                   "share", "K GB/s", "/wg")]
    for S in SCENARIOS:
        try:
            p = subprocess.run([sys.executable, __file__, "--one", str(S), "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=a.limit)
            rc, err = p.returncode, p.stderr.strip().splitlines()[-1:]
        except subprocess.TimeoutExpired:
            rc, err = 124, ["time limit of %d s" % a.limit]
        if rc != 0:      # nothing more is started on the device after a failure
            lines.append(f"S={S}: exit status {rc}: {err}")
            Path(a.out).write_text("\n".join(lines) + "\n")
            print("\n".join(lines))
            return rc
        d = json.loads(p.stdout.strip().splitlines()[-1])
        for h, r in d["h"].items():
            adv, roll = r["advance_ms"][0], r["rollout_ms"][0]
            gbs = d["S"] * int(h) * d["n_u"] * d["n_x"] * 8 / (adv * 1e-3) / 1e9
            lines.append("%5d %2s %28s %28s %7.2f %26s %8.1f %10.3f %6.3f%% %9.1f %8.2f"
                         % (d["S"], h, fmt(r["advance_ms"]), fmt(r["rollout_ms"]), roll / adv, fmt(d["solve_ms"]), d["n_bwd"], d["gains_ms"][0],
                            100.0 * adv / (d["solve_ms"][0] + d["gains_ms"][0] + adv), gbs, gbs / d["S"]))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
