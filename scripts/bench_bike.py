#!/usr/bin/env python
"""Whole solves of BikeDynamics5D batches: 4096 problems of k = 1, 2, 3, 4, 6 bikes, T = 50, dt = 0.1, n_lqr_iter = 50.

  default route   the solve loop's own choice (solve_prefers_records: which of the two below it takes)
  in-sweep        DPILQR_DEBUG_ROUTES=1 DPILQR_NO_WAVE_PREF=1: k <= 4, the wavefront sweep with in-sweep production (tu_bike.hip)
  record-fed      DPILQR_DEBUG_ROUTES=1 DPILQR_NO_INPROD=1: the family-5 tile producer + the record-fed padded sweep
  host plugin     the pre-feature way: the bike as a NumPy DynamicalModel subclass, ilqrSolver._solve_host_loop, per problem

Route flags are read once per process, so every (route, k) is a child process of its own; the three device routes alternate
(default, in-sweep, records, twice) and each child reports the median of its synchronised repetitions.

    python scripts/bench_bike.py [--reps 5] [--out profiles/bike_solves.txt]
"""
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
B, T, DT, KS = 4096, 50, 0.1, (1, 2, 3, 4, 6)


def scenarios(k, n, seed0=0):
    """(x0, xf) of n bike problems: random_setup's positions (heading, speed and steering zero), one bike from a seeded draw."""
    sys.path.insert(0, str(ROOT))
    from dpilqr_amd.util import random_setup
    x0 = np.zeros((n, 5 * k)); xf = np.zeros((n, 5 * k))
    for i in range(n):
        if k == 1:
            rng = np.random.default_rng(seed0 + i)
            x0[i, :2], xf[i, :2] = rng.uniform(-2, 2, size=2), rng.uniform(-2, 2, size=2)
            continue
        np.random.seed(seed0 + i)
        a, b = random_setup(k, 5, is_rotation=False, rel_dist=k, var=k / 2, n_d=2, random=True, energy=10.0)
        x0[i], xf[i] = a.ravel(), b.ravel()
    return x0, xf


def weights():
    return np.eye(5), np.eye(2), 1000.0 * np.eye(5)


def child_device(k, reps):
    import torch
    sys.path.insert(0, str(ROOT))
    import dpilqr_amd as dp
    from dpilqr_amd import _lib
    _lib.require_gpu()
    x0, xf = scenarios(k, B)
    Q, R, Qf = weights()
    pb = dp.ProblemBatch([10] * k, [2] * k, xf, Q, R, Qf, 0.5, DT, T)
    U0 = np.zeros((B, T, 2 * k))
    r = pb.solve(x0, U0)               # warm-up: code objects, workspace pool
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = pb.solve(x0, U0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    nb = r["n_bwd"].cpu().numpy()
    print(json.dumps({"k": k, "ms": [1e3 * t for t in times], "median_ms": 1e3 * statistics.median(times),
                      "mean_n_bwd": float(nb.mean()), "J_sum": float(r["J"].sum())}), flush=True)


def child_host(k, n):
    sys.path.insert(0, str(ROOT))
    import dpilqr_amd as dp

    class HostBike(dp.DynamicalModel):      # BikeDynamics5D as a NumPy plugin (one RK4 step: DynamicalModel.__call__)
        def __init__(self, dt, id=None):
            super().__init__(5, 2, dt, id)

        def f(self, x, u):
            return np.array([x[2] * np.cos(x[3]), x[2] * np.sin(x[3]), u[0], x[2] * np.tan(x[4]), u[1]])

        def linearize(self, x, u):
            tp = np.tan(x[4])
            A = np.zeros((5, 5)); Bm = np.zeros((5, 2))
            A[0, 2], A[0, 3] = np.cos(x[3]), -x[2] * np.sin(x[3])
            A[1, 2], A[1, 3] = np.sin(x[3]), x[2] * np.cos(x[3])
            A[3, 2], A[3, 4] = tp, x[2] * (tp * tp + 1)
            Bm[2, 0] = Bm[4, 1] = 1.0
            return np.eye(5) + self.dt * A, self.dt * Bm

    x0, xf = scenarios(k, n)
    Q, R, Qf = weights()
    times = []
    for i in range(n):
        ids = [100 + a for a in range(k)]
        dyn = dp.MultiDynamicalModel([HostBike(DT, id_) for id_ in ids])
        refs = [dp.ReferenceCost(xf[i, 5 * a:5 * a + 5], Q, R, Qf, ids[a]) for a in range(k)]
        prob = dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([5] * k, 0.5, [2] * k)))
        s = dp.ilqrSolver(prob, T)
        assert not s.on_device
        t0 = time.perf_counter()
        s.solve(x0[i], np.zeros((T, 2 * k)), verbose=False)
        times.append(time.perf_counter() - t0)
    print(json.dumps({"k": k, "ms_per_problem": [1e3 * t for t in times], "median_ms": 1e3 * statistics.median(times)}), flush=True)


def run_child(args, env_extra, timeout):
    env = {**os.environ, "DPILQR_DEBUG_ROUTES": "1", **env_extra}
    p = subprocess.run([sys.executable, __file__, *args], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} {env_extra} exited with {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    host_n = int(sys.argv[sys.argv.index("--host-problems") + 1]) if "--host-problems" in sys.argv else 2
    lines = [f"# python scripts/bench_bike.py {' '.join(sys.argv[1:])}",
             f"# {B} problems of k BikeDynamics5D, T = {T}, dt = {DT}, n_lqr_iter = 50, tol = 1e-3; Q = I, R = I, Q_f = 1000 I,"
             f" radius 0.5, n_dims 2; median of {reps} synchronised solves per child process after one warm-up",
             f"# {'k':>2} {'default ms':>11} {'in-sweep ms':>11} {'records ms':>11} {'records/in-sweep':>16} {'mean n_bwd':>10}   "
             f"host plugin ms/problem ({host_n} problems)   per-problem speed-up"]
    for line in lines:
        print(line, flush=True)
    for k in KS:
        runs = {"default": [], "inprod": [], "records": []}
        for rnd in range(2):
            for route, env in (("default", {}), ("inprod", {"DPILQR_NO_WAVE_PREF": "1"}), ("records", {"DPILQR_NO_INPROD": "1"})):
                runs[route].append(run_child(["--child-device", str(k), str(reps)], env, 900))
        d = statistics.median([r["median_ms"] for r in runs["default"]])
        ip = statistics.median([r["median_ms"] for r in runs["inprod"]])
        rc = statistics.median([r["median_ms"] for r in runs["records"]])
        same = all(r["J_sum"] == runs["default"][0]["J_sum"] for rs in runs.values() for r in rs)
        h = run_child(["--child-host", str(k), str(host_n)], {}, 1200)
        per = d / B
        line = (f"  {k:2d} {d:11.1f} {ip:11.1f} {rc:11.1f} {rc / ip:16.3f} {runs['default'][0]['mean_n_bwd']:10.2f}   "
                f"{h['median_ms']:10.1f}   {h['median_ms'] / per:10.0f}x"
                f"{'' if same else '   (!) routes disagree on sum J'}")
        lines.append(line)
        print(line, flush=True)
        lines.append("#    runs " + "  ".join(f"{route} {[round(r['median_ms'], 1) for r in rs]}" for route, rs in runs.items()))
        print(lines[-1], flush=True)
    if out:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--child-device" in sys.argv:
        i = sys.argv.index("--child-device")
        child_device(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    elif "--child-host" in sys.argv:
        i = sys.argv.index("--child-host")
        child_host(int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    else:
        main()
