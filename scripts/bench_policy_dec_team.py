#!/usr/bin/env python
"""Launch time of the team closed-loop rollout (dpilqr_policy_rollout_dec_team, csrc/policy_dec_team.hpp).  Nothing is asserted:
nobody has measured these before, and the open-loop figure beside each row is only the yardstick the numbers are read against.

Workloads: DoubleIntDynamics4D teams of k = 24 and k = 64 agents (n_x = 96 / 256), T = 50, 64 samples per item, 1 and 32 items,
once with every neighbourhood full (kc_max = k) and once with kc_max = 8 (agent a sees a .. a + 7 mod k).  The policy is
synthetic (a resting nominal, small random gains): the kernel's work does not depend on the values.  Beside each row:
ProblemBatch.rollout_wide's open-loop time for the same number of trajectories (items x samples, zero controls).
At fifteen UnicycleDynamics4D (n_x = 60), where both kernels run, the same rows with policy_rollout_dec's time beside them.
Per figure: median (min .. max) of --reps launches after a warm-up (HIP events), trajectories not stored.  "gain B/step": the
compact image a workgroup's threads read per step, k n_c kc_max n_s 8 bytes; "lines/load": the distinct 128-byte lines one
wavefront-wide load of the gains touches (neighbouring agents' rows are n_c kw doubles apart).
Every team size runs in a child process under its own time limit; after a failure nothing more is started.

    python scripts/bench_policy_dec_team.py [--reps 7] [--samples 64] [--out profiles/policy_dec_team.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {"24xDoubleInt4D": (0, 24, 4, 2), "64xDoubleInt4D": (0, 64, 4, 2), "15xUnicycle4D": (3, 15, 4, 2)}
T, DT, RADIUS = 50, 0.1, 0.5


def one(name, n_samples, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    model, k, ns, nc = WORKLOADS[name]
    n, m = k * ns, k * nc
    both = n <= 60 and k <= 20
    rng = np.random.default_rng(k)
    Q, R, Qf = np.eye(ns), np.eye(nc), 100.0 * np.eye(ns)

    def timed(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    rows = []
    for B in (1, 32):
        x0 = np.zeros((B, k, ns)); x0[:, :, :2] = rng.uniform(-5.0, 5.0, size=(B, k, 2))
        xf = np.zeros((B, k, ns)); xf[:, :, :2] = rng.uniform(-5.0, 5.0, size=(B, k, 2))
        pb = dp.ProblemBatch([model] * k, [2] * k, xf.reshape(B, n), Q, R, Qf, RADIUS, DT, T)
        dev = pb._xf.device
        X = torch.as_tensor(np.repeat(x0.reshape(B, 1, n), T + 1, axis=1), device=dev)
        U = torch.zeros((B, T, m), dtype=torch.float64, device=dev)
        x0s = torch.as_tensor(x0.reshape(B, 1, n) + 0.05 * rng.normal(size=(B, n_samples, n)), device=dev)
        # the yardstick: the same number of trajectories rolled out open loop
        pw = dp.ProblemBatch([model] * k, [2] * k, np.repeat(xf.reshape(B, n), n_samples, axis=0), Q, R, Qf, RADIUS, DT, T)
        xw = x0s.reshape(B * n_samples, n).contiguous()
        Uw = torch.zeros((B * n_samples, T, m), dtype=torch.float64, device=dev)
        wide = timed(lambda: pw.rollout_wide(xw, Uw, trajectories=False))
        for mode, kc_max in (("full", k), ("kc_max=8", 8)):
            masks = np.zeros((B, k), dtype=np.uint64)
            for a in range(k):
                masks[:, a] = np.uint64(sum(1 << ((a + j) % k) for j in range(kc_max)))
            bits = torch.as_tensor(masks.view(np.int64), device=dev)
            Kc = torch.as_tensor(1e-3 * rng.normal(size=(B, T, k, nc, kc_max * ns)), device=dev)
            pb.policy_rollout_dec_team(X, U, Kc, bits, x0s)      # the first call reads the masks back and checks them
            team = timed(lambda: pb.policy_rollout_dec_team(X, U, Kc, bits, x0s, masks_checked=bits))
            dec = None
            if both:
                pb.policy_rollout_dec(X, U, Kc, bits, x0s)
                dec = timed(lambda: pb.policy_rollout_dec(X, U, Kc, bits, x0s, masks_checked=bits))
            row_bytes = nc * kc_max * ns * 8      # between neighbouring agents' rows
            lines = min(64, k) if row_bytes >= 128 else -(-min(64, k) * row_bytes // 128)
            rows.append(dict(B=B, mode=mode, kc_max=kc_max, team_ms=team, wide_ms=wide, dec_ms=dec, gain_bytes=8 * k * nc * kc_max * ns,
                             lines=int(lines), workgroups=B * -(-n_samples // (256 // k))))
    print(json.dumps(dict(name=name, k=k, n_x=n, samples=n_samples, rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_team.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per team size")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.samples, a.reps)
    fmt = lambda t: "%8.3f (%6.3f..%6.3f)" % t if t else "%24s" % "-"
    lines = ["team closed-loop rollout (dpilqr_policy_rollout_dec_team): T = %d, %d samples per item, trajectories not stored; ms per launch, "
             "median (min .. max) of %d launches after a warm-up" % (T, a.samples, a.reps),
             "open loop: rollout_wide of items x samples trajectories (the yardstick); dec: policy_rollout_dec where it serves the shape",
             "%-16s %5s %-9s %6s %-24s %-24s %7s %-24s %11s %10s" % ("team", "items", "masks", "wgs", "team ms", "open loop ms", "ratio", "dec ms",
                                                                     "gain B/step", "lines/load")]
    faster = []
    for name in WORKLOADS:
        p = subprocess.run([sys.executable, __file__, "--one", name, "--reps", str(a.reps), "--samples", str(a.samples)],
                           capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:      # nothing more is started on the device after a failure
            lines.append(f"{name}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1:]}")
            Path(a.out).write_text("\n".join(lines) + "\n")
            print("\n".join(lines))
            return p.returncode
        d = json.loads(p.stdout.strip().splitlines()[-1])
        for r in d["rows"]:
            team, wide, dec = tuple(r["team_ms"]), tuple(r["wide_ms"]), tuple(r["dec_ms"]) if r["dec_ms"] else None
            lines.append("%-16s %5d %-9s %6d %s %s %7.2f %s %11d %10d" % (name, r["B"], r["mode"], r["workgroups"], fmt(team), fmt(wide),
                                                                         team[0] / wide[0], fmt(dec), r["gain_bytes"], r["lines"]))
            if dec:
                faster.append((name, r["B"], r["mode"], team[0], dec[0]))
    if faster:
        lines.append("where both kernels run (n_x = 60): " + "; ".join(
            "%s %d items %s: team %.3f ms against dec %.3f ms (%s)" % (nm, B, mode, t, d_, "team faster" if t < d_ else "dec faster")
            for nm, B, mode, t, d_ in faster))
        lines.append("DistributedPolicy.rollout keeps policy_rollout_dec for n_x <= 60 and k <= 20 whichever is faster here: rerouting would "
                     "change existing behaviour (J and min_sep are summed in another order).")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
