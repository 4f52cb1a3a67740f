#!/usr/bin/env python
"""Launch time of the closed-loop ensemble rollout (dpilqr_policy_rollout, csrc/policy.hpp) against its yardstick, the
open-loop dpilqr_rollout on B * S independent items fed the same controls: the same dynamics and cost work without K dx and
without sharing.  Shapes: cfg2's (5 x DoubleInt4D, T = 50, B = 1024) and two at n_x = 60 (10 x Quadcopter6D, 15 x Unicycle4D,
T = 50, B = 256), each at S = 1, 16, 64, trajectories not stored.  Every (shape, S) runs in a child process under its own time
limit; the median of --reps timed launches (HIP events) after a warm-up is reported, with ns per sample-step, the ratio to the
yardstick and the algorithmic bytes per step (K[t], X[t], U[t] counted once per workgroup).

    python scripts/bench_policy.py [--reps 7] [--out profiles/policy_rollout.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {"cfg2_5xDoubleInt4D": (0, 5, 1024), "10xQuadcopter6D": (4, 10, 256), "15xUnicycle4D": (3, 15, 256)}
T = 50


def one(shape, S, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    model, k, B = SHAPES[shape]
    ns, nc = dp.batch.MODEL_DIMS[model]
    n, m = k * ns, k * nc
    rng = np.random.default_rng(5)
    xf = rng.normal(size=(B, n)) * 1.5; x0 = rng.normal(size=(B, n)) * 1.5
    x0.reshape(B, k, ns)[:, :, 2:] *= 0.1; xf.reshape(B, k, ns)[:, :, 2:] = 0.0
    U0 = rng.normal(size=(B, T, m)) * 0.05
    if model == 4:
        U0[:, :, 0::nc] += 9.80665
    Q, R, Qf = np.eye(ns), np.eye(nc), 100.0 * np.eye(ns)
    nd = [3 if ns >= 6 else 2] * k
    pb = dp.ProblemBatch([model] * k, nd, xf, Q, R, Qf, 0.5, 0.1, T)
    X, _ = pb.rollout(x0, U0)
    K, _ = pb.backward_pass(X, U0, 1.0)
    x0s = X[:, :1, :] + 0.05 * torch.randn((B, S, n), dtype=torch.float64, device=X.device, generator=torch.Generator(X.device).manual_seed(1))
    U0d = dp.device.to_dev(U0)
    r = pb.policy_rollout(X, U0d, K, x0s, trajectories=True)
    Us = r["U"].reshape(B * S, T, m).contiguous()
    pb2 = dp.ProblemBatch([model] * k, nd, np.repeat(xf, S, axis=0), Q, R, Qf, 0.5, 0.1, T)
    x0f = x0s.reshape(B * S, n).contiguous()

    def timed(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    pol = timed(lambda: pb.policy_rollout(X, U0d, K, x0s))
    opn = timed(lambda: pb2.rollout(x0f, Us))
    spw = 256 // k
    chunks = -(-S // spw)
    shared = 8 * (m * n + n + m) * B * chunks           # per step, K[t], X[t], U[t] once per workgroup
    per_sample = 8 * (n + (2 + k)) * B * S / T          # x0s in, J / min_sep / goal_dist out, spread over the steps
    print(json.dumps(dict(shape=shape, S=S, B=B, k=k, n_x=n, n_u=m, policy_ms=pol, open_loop_ms=opn, chunks=chunks,
                          bytes_per_step=shared + per_sample, bytes_per_step_unshared=8 * (m * n + n + m) * B * S + per_sample)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_rollout.txt"))
    ap.add_argument("--one", nargs=2, default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per (shape, S)")
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], int(a.one[1]), a.reps)
    lines = ["closed-loop ensemble rollout, T = %d, trajectories not stored; median (min .. max) of %d launches after a warm-up" % (T, a.reps),
             "yardstick: dpilqr_rollout on B * S items fed the controls the policy produced",
             "%-20s %5s %3s %22s %12s %24s %7s %14s %10s" % ("shape", "B", "S", "policy ms", "ns/smp-step", "open-loop ms", "ratio", "alg. B/step", "GB/s")]
    base = {}
    for shape in SHAPES:
        for S in (1, 16, 64):
            p = subprocess.run([sys.executable, __file__, "--one", shape, str(S), "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=a.limit)
            if p.returncode != 0:      # nothing more is started on the device after a failure
                lines.append(f"{shape} S={S}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1:]}")
                Path(a.out).write_text("\n".join(lines) + "\n")
                print("\n".join(lines))
                return p.returncode
            d = json.loads(p.stdout.strip().splitlines()[-1])
            med, lo, hi = d["policy_ms"]; omed, olo, ohi = d["open_loop_ms"]
            if S == 1:
                base[shape] = med
            lines.append("%-20s %5d %3d %8.3f (%6.3f..%6.3f) %12.2f %9.3f (%6.3f..%6.3f) %7.2f %14.0f %10.1f   x%.1f of S = 1"
                         % (shape, d["B"], S, med, lo, hi, med * 1e6 / (d["B"] * S * T), omed, olo, ohi, med / omed, d["bytes_per_step"],
                            d["bytes_per_step"] * T / (med * 1e-3) / 1e9, med / base[shape]))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
