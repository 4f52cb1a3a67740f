#!/usr/bin/env python
"""Launch time of the closed-loop rollout for teams of up to 256 agents (dpilqr_policy_rollout_dec_wide,
csrc/policy_dec_team.hpp at four mask words).  Nothing is asserted and no target is set: nobody has measured this kernel before, and the open-loop
figure beside each row is only the yardstick the numbers are read against.

Workloads: DoubleIntDynamics4D teams of k = 65, 128 and 256 agents (n_x = 260 .. 1024), T = 50, 64 samples per item, 1 and 32
items, kc_max = 8 and 20 (agent a sees a .. a + kc_max - 1 mod k: neighbourhoods that wrap across the words).  The policy is
synthetic (a resting nominal, small random gains): the kernel's work does not depend on the values.  Beside each row:
ProblemBatch.rollout_wide's open-loop time for the same number of trajectories (items x samples, zero controls).
At k = 64 (n_words = 1) the same rows with policy_rollout_dec_team's time beside them: the two kernels run the same statements
there and should tie; the two are timed alternately in one window and the ratio wide / team is recorded.
Per figure: median (min .. max) of --reps launches after a warm-up (HIP events), trajectories not stored.  "gain B/step": the
compact image a workgroup's threads read per step, k n_c kc_max n_s 8 bytes; "pairs/thread": k / 2 partner offsets per step.
Every team size runs in a child process under its own time limit; after a failure nothing more is started.

    python scripts/bench_policy_dec_wide.py [--reps 7] [--samples 64] [--out profiles/policy_dec_wide.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TEAMS = (64, 65, 128, 256)
KC_MAX = (8, 20)
T, DT, RADIUS, NS, NC = 50, 0.1, 0.5, 4, 2


def one(k, n_samples, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    n, m, nw = k * NS, k * NC, (k + 63) // 64
    rng = np.random.default_rng(k)
    Q, R, Qf = np.eye(NS), np.eye(NC), 100.0 * np.eye(NS)

    def timed(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    def timed_pair(fa, fb):
        """Two versions in the same window, alternating: what a tie is read from."""
        fa(); fb(); torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            for fn, ts in ((fa, ta), (fb, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
        return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))

    rows = []
    for B in (1, 32):
        x0 = np.zeros((B, k, NS)); x0[:, :, :2] = rng.uniform(-5.0, 5.0, size=(B, k, 2))
        xf = np.zeros((B, k, NS)); xf[:, :, :2] = rng.uniform(-5.0, 5.0, size=(B, k, 2))
        pb = dp.ProblemBatch([0] * k, [2] * k, xf.reshape(B, n), Q, R, Qf, RADIUS, DT, T)
        dev = pb._xf.device
        X = torch.as_tensor(np.repeat(x0.reshape(B, 1, n), T + 1, axis=1), device=dev)
        U = torch.zeros((B, T, m), dtype=torch.float64, device=dev)
        x0s = torch.as_tensor(x0.reshape(B, 1, n) + 0.05 * rng.normal(size=(B, n_samples, n)), device=dev)
        # the yardstick: the same number of trajectories rolled out open loop
        pw = dp.ProblemBatch([0] * k, [2] * k, np.repeat(xf.reshape(B, n), n_samples, axis=0), Q, R, Qf, RADIUS, DT, T)
        xw = x0s.reshape(B * n_samples, n).contiguous()
        Uw = torch.zeros((B * n_samples, T, m), dtype=torch.float64, device=dev)
        open_loop = timed(lambda: pw.rollout_wide(xw, Uw, trajectories=False))
        del Uw
        for kc_max in KC_MAX:
            words = np.zeros((B, k, nw), dtype=np.uint64)
            for a in range(k):
                for j in range(kc_max):
                    o = (a + j) % k
                    words[:, a, o // 64] |= np.uint64(1) << np.uint64(o % 64)
            bits = torch.as_tensor(words.view(np.int64), device=dev)
            gen = torch.Generator(device=dev); gen.manual_seed(1000 * k + kc_max)
            Kc = 1e-3 * torch.randn((B, T, k, NC, kc_max * NS), dtype=torch.float64, device=dev, generator=gen)
            pb.policy_rollout_dec_wide(X, U, Kc, bits, x0s)      # the first call reads the masks back and checks them
            run_wide = lambda: pb.policy_rollout_dec_wide(X, U, Kc, bits, x0s, masks_checked=bits)
            team = None
            if k <= 64:
                bits1 = bits.reshape(B, k).contiguous()
                pb.policy_rollout_dec_team(X, U, Kc, bits1, x0s)
                wide, team = timed_pair(run_wide, lambda: pb.policy_rollout_dec_team(X, U, Kc, bits1, x0s, masks_checked=bits1))
            else:
                wide = timed(run_wide)
            rows.append(dict(B=B, kc_max=kc_max, wide_ms=wide, open_ms=open_loop, team_ms=team, gain_bytes=8 * k * NC * kc_max * NS,
                             pairs=k // 2, workgroups=B * -(-n_samples // (256 // k))))
            del Kc
    print(json.dumps(dict(k=k, n_x=n, samples=n_samples, rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_wide.txt"))
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--limit", type=int, default=180, help="seconds per team size")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.samples, a.reps)
    fmt = lambda t: "%8.3f (%6.3f..%6.3f)" % t if t else "%24s" % "-"
    lines = ["wide closed-loop rollout (dpilqr_policy_rollout_dec_wide): DoubleIntDynamics4D, T = %d, %d samples per item, trajectories not "
             "stored; ms per launch, median (min .. max) of %d launches after a warm-up (HIP events)" % (T, a.samples, a.reps),
             "open loop: rollout_wide of items x samples trajectories (the yardstick); team: policy_rollout_dec_team where it serves the team (k <= 64)",
             "%5s %5s %6s %6s %-24s %-24s %7s %-24s %11s %12s" % ("k", "items", "kc_max", "wgs", "wide ms", "open loop ms", "ratio", "team ms",
                                                                  "gain B/step", "pairs/thread")]
    ties = []
    for k in TEAMS:
        try:
            p = subprocess.run([sys.executable, __file__, "--one", str(k), "--reps", str(a.reps), "--samples", str(a.samples)],
                               capture_output=True, text=True, timeout=a.limit)
            rc, err = p.returncode, p.stderr
        except subprocess.TimeoutExpired:
            rc, err = 124, "time limit"
        if rc != 0:      # nothing more is started on the device after a failure
            lines.append(f"k = {k}: exit status {rc}: {err.strip().splitlines()[-1:]}")
            Path(a.out).write_text("\n".join(lines) + "\n")
            print("\n".join(lines))
            return rc
        d = json.loads(p.stdout.strip().splitlines()[-1])
        for r in d["rows"]:
            wide, op, team = tuple(r["wide_ms"]), tuple(r["open_ms"]), tuple(r["team_ms"]) if r["team_ms"] else None
            lines.append("%5d %5d %6d %6d %s %s %7.2f %s %11d %12d" % (k, r["B"], r["kc_max"], r["workgroups"], fmt(wide), fmt(op), wide[0] / op[0],
                                                                      fmt(team), r["gain_bytes"], r["pairs"]))
            if team:
                ties.append((r["B"], r["kc_max"], wide[0], team[0]))
    if ties:
        lines.append("k = 64, n_words = 1, wide / team: " + "; ".join("%d items kc_max %d: %.3f / %.3f ms = %.3f" % (B, kc, w, t, w / t)
                                                                       for B, kc, w, t in ties))
    lines += ["measured: the launch times above, with HIP events around one enqueue each (the masks checked beforehand, not inside the timed call).",
              "supposed, not measured: where a step's time goes.  No counter was collected for this kernel; profiles/policy_dec_team.txt attributes "
              "the team kernel's step to the number of cache lines its gain reads touch, without counters, and the wide kernel reads the same "
              "lines per member -- at k = 256 it adds up to 128 pair terms per thread and step, whose share of the time is not separated here."]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
