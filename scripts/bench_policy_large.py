#!/usr/bin/env python
"""Launch time of the large-cluster closed-loop rollout (dpilqr_policy_rollout_large, csrc/policy_large.hpp) against the yardstick
of scripts/bench_policy.py: the open-loop dpilqr_rollout on B * S independent items fed the controls the policy produced -- the
same dynamics and cost work without K dx and without sharing.  Shapes: BASELINE config 5's composition (14 x Quadcopter12D + 6 x
padded HumanDynamics6D, n_x = 240, n_u = 80, T = 150) at B = 1 and 32, and 16 x Unicycle4D (n_x = 64, T = 50) at B = 256, each at
S = 1, 12, 64, trajectories not stored.  Every (shape, S) runs in a child process under its own time limit and nothing more is
started after a failure; the median, minimum and maximum of --reps timed launches (HIP events) after a warm-up are reported, with
ns per sample-step, the ratio to the yardstick, the K bytes read per second (B * chunks * T * n_u * n_x * 8 over the launch time:
K[t] once per workgroup and step) and the fp64 rate of the product (2 n_u n_x per sample-step).  No threshold: the file is the record.

    python scripts/bench_policy_large.py [--reps 7] [--out profiles/policy_large_rollout.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# name: (models, n_dims, T, B, dt)
SHAPES = {"cfg5_14xQuad12D+6xHuman": ([7] * 14 + [8] * 6, [3] * 14 + [2] * 6, 150, 1, 0.05),
          "cfg5_14xQuad12D+6xHuman_B32": ([7] * 14 + [8] * 6, [3] * 14 + [2] * 6, 150, 32, 0.05),
          "16xUnicycle4D": ([3] * 16, [2] * 16, 50, 256, 0.1)}
SAMPLES = (1, 12, 64)


def one(shape, S, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    models, nd, T, B, dt = SHAPES[shape]
    k = len(models)
    ns, nc = dp.batch.MODEL_DIMS[models[0]]
    n, m = k * ns, k * nc
    rng = np.random.default_rng(5)
    xf = rng.normal(size=(B, n)) * 1.5; x0 = rng.normal(size=(B, n)) * 1.5
    x0.reshape(B, k, ns)[:, :, 3 if ns >= 6 else 2:] *= 0.1; xf.reshape(B, k, ns)[:, :, 3 if ns >= 6 else 2:] = 0.0
    U0 = rng.normal(size=(B, T, m)) * 0.05
    spread = 0.05
    if ns == 12:      # near hover, short steps (tests/policy_cases.py)
        U0 = U0 * 1e-4; U0[:, :, 3::4] += 9.80665 * 63.0 / 2000.0
        x0.reshape(B, k, ns)[:, :, 3:] *= 0.02
        spread = 0.005
    Q, R, Qf = np.eye(ns), np.eye(nc), 100.0 * np.eye(ns)
    pb = dp.ProblemBatch(models, nd, xf, Q, R, Qf, 0.5, dt, T)
    X, _ = pb.rollout(x0, U0)
    K, _ = pb.backward_pass(X, U0, 1.0)
    x0s = X[:, :1, :] + spread * torch.randn((B, S, n), dtype=torch.float64, device=X.device, generator=torch.Generator(X.device).manual_seed(1))
    U0d = dp.device.to_dev(U0)
    r = pb.policy_rollout_large(X, U0d, K, x0s, trajectories=True)
    finite = float(torch.isfinite(r["J"]).double().mean().item())
    Us = r["U"].reshape(B * S, T, m).contiguous()
    del r
    pb2 = dp.ProblemBatch(models, nd, np.repeat(xf, S, axis=0), Q, R, Qf, 0.5, dt, T)
    x0f = x0s.reshape(B * S, n).contiguous()

    def timed(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    pol = timed(lambda: pb.policy_rollout_large(X, U0d, K, x0s))
    opn = timed(lambda: pb2.rollout(x0f, Us))
    chunks = -(-S // (256 // k))
    print(json.dumps(dict(shape=shape, S=S, B=B, T=T, k=k, n_x=n, n_u=m, policy_ms=pol, open_loop_ms=opn, chunks=chunks, finite=finite,
                          k_bytes=8 * m * n * T * B * chunks, flops=2 * m * n * T * B * S)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_large_rollout.txt"))
    ap.add_argument("--one", nargs=2, default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds per (shape, S)")
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], int(a.one[1]), a.reps)
    lines = ["large-cluster closed-loop ensemble rollout (K[t] dx on the fp64 matrix pipe), trajectories not stored; median (min .. max) of %d "
             "launches after a warm-up" % a.reps,
             "yardstick: dpilqr_rollout on B * S items fed the controls the policy produced",
             "K GB/s: B * chunks * T * n_u * n_x * 8 bytes over the launch time; GF/s: 2 n_u n_x flops per sample-step over the launch time",
             "%-28s %4s %4s %3s %22s %12s %24s %7s %9s %9s %7s" % ("shape", "B", "T", "S", "policy ms", "ns/smp-step", "open-loop ms", "ratio",
                                                                   "K GB/s", "GF/s", "finite")]
    base = {}
    for shape in SHAPES:
        for S in SAMPLES:
            try:
                p = subprocess.run([sys.executable, __file__, "--one", shape, str(S), "--reps", str(a.reps)], capture_output=True, text=True,
                                   timeout=a.limit)
                rc, err = p.returncode, p.stderr.strip().splitlines()[-1:]
            except subprocess.TimeoutExpired:
                rc, err = 124, ["time limit of %d s" % a.limit]
            if rc != 0:      # nothing more is started on the device after a failure
                lines.append(f"{shape} S={S}: exit status {rc}: {err}")
                Path(a.out).write_text("\n".join(lines) + "\n")
                print("\n".join(lines))
                return rc
            d = json.loads(p.stdout.strip().splitlines()[-1])
            med, lo, hi = d["policy_ms"]; omed, olo, ohi = d["open_loop_ms"]
            if S == SAMPLES[0]:
                base[shape] = med
            lines.append("%-28s %4d %4d %3d %8.3f (%6.3f..%6.3f) %12.2f %9.3f (%6.3f..%6.3f) %7.2f %9.1f %9.1f %7.2f   x%.1f of S = %d"
                         % (shape, d["B"], d["T"], S, med, lo, hi, med * 1e6 / (d["B"] * S * d["T"]), omed, olo, ohi, med / omed,
                            d["k_bytes"] / (med * 1e-3) / 1e9, d["flops"] / (med * 1e-3) / 1e9, d["finite"], med / base[shape], SAMPLES[0]))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
