#!/usr/bin/env python
"""Launch time of the receding-horizon advance (dpilqr_policy_advance, csrc/policy_advance.hpp) against what the same result
cost before it existed: dpilqr_policy_rollout with ONE sample per item over the whole horizon (trajectories stored), plus the
torch shift and append of solve_rhc_scenarios.  Also the share of one receding-horizon round (solve + gains + advance) the
advance takes.  Shapes: cfg2's (5 x DoubleInt4D, T = 50) at 1024 scenarios and 10 x Quadcopter6D at T = 75 (256 scenarios),
each at h = 1 and h = 5, under a disturbance and control limits.  Every shape runs in a child process under its own time
limit; medians (min .. max) of --reps timed repetitions (HIP events) after a warm-up.

    python scripts/bench_policy_advance.py [--reps 9] [--out profiles/policy_advance.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"cfg2_5xDoubleInt4D": (0, 5, 1024, 50), "10xQuadcopter6D": (4, 10, 256, 75)}
HS = (1, 5)


def one(shape, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    model, k, S, T = SHAPES[shape]
    ns, nc = dp.batch.MODEL_DIMS[model]
    n, m = k * ns, k * nc
    rng = np.random.default_rng(5)
    xf = rng.normal(size=(S, n)) * 1.5; x0 = rng.normal(size=(S, n)) * 1.5
    x0.reshape(S, k, ns)[:, :, 2:] *= 0.1; xf.reshape(S, k, ns)[:, :, 2:] = 0.0
    U0 = rng.normal(size=(S, T, m)) * 0.01
    if model == 4:
        U0[:, :, 0::nc] += 9.80665
    nd = [3 if ns >= 6 else 2] * k
    pb = dp.ProblemBatch([model] * k, nd, xf, np.eye(ns), np.eye(nc), 100.0 * np.eye(ns), 0.5, 0.1, T)
    L = 8
    W = dp.device.to_dev(1e-2 * rng.normal(size=(S, L, n)))
    u_lim = np.stack([np.full(m, -2.0), np.full(m, 2.0)]) + (9.80665 * (np.arange(m) % nc == 0) if model == 4 else 0.0)

    def timed(fn, before=None, reps_=reps):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps_):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    x0d, U0d = dp.device.to_dev(x0), dp.device.to_dev(U0)
    sol = pb.solve(x0d, U0d)
    X, U = sol["X"], sol["U"]
    K = pb.backward_pass(X, U, 0.0)[0]
    solve_ms = timed(lambda: pb.solve(x0d, U0d), reps_=3)
    gains_ms = timed(lambda: pb.backward_pass(X, U, 0.0))
    state = pb.advance_state(x0, L)
    x0s = x0d[:, None, :].contiguous()
    out = dict(shape=shape, S=S, k=k, T=T, n_x=n, solve_ms=solve_ms, gains_ms=gains_ms, h={})
    for h in HS:
        adv = timed(lambda: pb.policy_advance(X, U, K, h, state, W=W, u_lim=u_lim), before=lambda: state["n_done"].zero_())
        Wp = torch.zeros((S, 1, T, n), dtype=torch.float64, device=X.device); Wp[:, 0, :h] = W[:, :h]
        xi, Xw, Uw = x0d.clone(), torch.zeros_like(X), torch.zeros_like(U)
        ia = torch.arange(S, device=X.device)

        def parent():      # the rollout over the whole horizon, then solve_rhc_scenarios' bookkeeping in torch
            r = pb.policy_rollout(X, U, K, x0s, W=Wp, u_lim=u_lim, trajectories=True)
            Xa, Ua = r["X"][:, 0], r["U"][:, 0]
            Xa[:, :h].clone(); Ua[:, :h].clone()
            xi[ia] = Xa[:, h]
            Xw[ia] = torch.cat([X[:, h:], X[:, -1:].expand(-1, h, -1)], dim=1)
            Uw[ia] = torch.cat([U[:, h:], torch.zeros((S, h, m), dtype=torch.float64, device=X.device)], dim=1)

        par = timed(parent)
        roll = timed(lambda: pb.policy_rollout(X, U, K, x0s, W=Wp, u_lim=u_lim, trajectories=True))
        out["h"][h] = dict(advance_ms=adv, parent_ms=par, rollout_ms=roll)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--limit", type=int, default=200, help="seconds per shape")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.reps)
    fmt = lambda t: "%8.3f (%6.3f..%6.3f)" % tuple(t)
    lines = ["receding-horizon advance under W and u_lim; median (min .. max) ms of %d repetitions after a warm-up, HIP events" % a.reps,
             "advance: ONE dpilqr_policy_advance launch (h steps, floor(256 / k) scenarios per workgroup, the bookkeeping included)",
             "before:  dpilqr_policy_rollout, one sample per item, all T steps, trajectories stored (its launch alone: 'rollout')",
             "         + the torch shift / append of solve_rhc_scenarios (eight small launches)",
             "share:   advance / (solve + gains + advance) of one receding-horizon round from a cold warm start",
             "K[i] is read from global memory by the lane that uses it; what a staged copy would cost instead was NOT measured.",
             "%-20s %5s %3s %2s %24s %24s %24s %7s %10s %10s %7s" % ("shape", "S", "T", "h", "advance ms", "before ms", "rollout ms", "ratio",
                                                                     "solve ms", "gains ms", "share")]
    for shape in SHAPES:
        p = subprocess.run([sys.executable, __file__, "--one", shape, "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:      # nothing more is started on the device after a failure
            lines.append(f"{shape}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1:]}")
            Path(a.out).write_text("\n".join(lines) + "\n")
            print("\n".join(lines))
            return p.returncode
        d = json.loads(p.stdout.strip().splitlines()[-1])
        for h, r in d["h"].items():
            adv, par = r["advance_ms"][0], r["parent_ms"][0]
            lines.append("%-20s %5d %3d %2s %24s %24s %24s %7.2f %10.3f %10.3f %6.1f%%"
                         % (shape, d["S"], d["T"], h, fmt(r["advance_ms"]), fmt(r["parent_ms"]), fmt(r["rollout_ms"]), par / adv,
                            d["solve_ms"][0], d["gains_ms"][0], 100.0 * adv / (d["solve_ms"][0] + d["gains_ms"][0] + adv)))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
