#!/usr/bin/env python
"""Measure the swarm study (profiles/swarm_study.txt).  Record only: nothing is gated on these figures.

(a) Drawing a cell's inputs: analysis.trial_inputs_batch (dpilqr_trial_inputs, one launch) against the only way there was -- the
    host loop over analysis.trial_inputs plus the upload of x0, xf and the two warm starts.  k = 65 / 128 / 256 double
    integrators, S = 64 / 1024 trials, N = 50; median of 7 after a warm-up, each timed to torch.cuda.synchronize().
(b) One study cell: k = 130, max_cluster = 8, solve_rhc_scenarios(wide=True, rows=...) on device inputs; wall time per round,
    split into the batched solve (solve_scenarios_distributed), the row formatting (rhc_subgraphs + rhc_log_row) and the loop's
    glue (everything else: the shift, the stopping flags, the executed-prefix copies), by timing wrappers around those calls.

    python scripts/bench_swarm_study.py [--out profiles/swarm_study.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def median_of(fn, reps=7):
    import torch
    fn(); torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    return statistics.median(t)


def draw_inputs(lines):
    from dpilqr_amd import analysis
    from dpilqr_amd.device import to_dev
    N, M = 50, analysis.DoubleIntDynamics4D
    lines.append("(a) a cell's inputs, N = 50, DoubleIntDynamics4D, energy = 5 k: median of 7 after a warm-up [ms]")
    lines.append(f"{'k':>5} {'S':>6} {'device':>10} {'host loop':>10} {'upload':>10} {'host total':>11} {'ratio':>8}")
    for k in (65, 128, 256):
        for S in (64, 1024):
            seeds = [analysis.seed_of(M, k, i) for i in range(S)]
            dev = median_of(lambda: analysis.trial_inputs_batch(k, 4, 2 * k, N, 5.0 * k, 2, seeds))
            held = {}

            def host():
                d = [analysis.trial_inputs(k, 4, 2 * k, N, 5.0 * k, 2, s) for s in seeds]
                held["a"] = [np.stack([x[j].reshape(x[j].shape[0], -1) if j > 1 else x[j].ravel() for x in d]) for j in range(4)]

            t_host = median_of(host, reps=3 if S > 64 else 7)
            t_up = median_of(lambda: [to_dev(a) for a in held["a"]])
            lines.append(f"{k:>5} {S:>6} {dev * 1e3:>10.3f} {t_host * 1e3:>10.1f} {t_up * 1e3:>10.3f} {(t_host + t_up) * 1e3:>11.1f} "
                         f"{(t_host + t_up) / dev:>8.0f}")
    lines.append("    (the host loop of S = 1024: median of 3)")


def study_cell(lines):
    import torch
    from dpilqr_amd import analysis, dispatch, distributed
    k, N, S, cap, energy = 130, 20, 8, 8, 600.0
    M = analysis.DoubleIntDynamics4D
    spent = {"solve": 0.0, "rows": 0.0, "rounds": 0}

    def timed(fn, key, count=False):
        def run(*a, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize(); spent[key] += time.perf_counter() - t0
            if count:
                spent["rounds"] += 1
            return r
        return run

    x0, xf, _, U_d = analysis.trial_inputs_batch(k, 4, 2 * k, N, energy, 2, [analysis.seed_of(M, k, i) for i in range(S)])
    prob = analysis.build_problem(M, k, 0.1, 0.5, xf[0].cpu().numpy(), 2)
    kw = dict(xf=xf, U0=U_d, centralized=False, n_d=2, step_size=analysis.STEP_SIZE, dist_converge=0.1, t_diverge=0.85, wide=True,
              max_cluster=cap, i_trial=list(range(S)))
    distributed.solve_rhc_scenarios(prob, x0, N, 0.5, rows=[], **kw)      # warm-up
    keep = dispatch.solve_scenarios_distributed, distributed.rhc_subgraphs, distributed.rhc_log_row
    dispatch.solve_scenarios_distributed = timed(keep[0], "solve", count=True)
    distributed.rhc_subgraphs, distributed.rhc_log_row = timed(keep[1], "rows"), timed(keep[2], "rows")
    try:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        distributed.solve_rhc_scenarios(prob, x0, N, 0.5, rows=[], **kw)
        torch.cuda.synchronize(); total = time.perf_counter() - t0
    finally:
        dispatch.solve_scenarios_distributed, distributed.rhc_subgraphs, distributed.rhc_log_row = keep
    n = max(spent["rounds"], 1)
    glue = total - spent["solve"] - spent["rows"]
    lines.append("")
    lines.append(f"(b) one study cell: k = {k}, max_cluster = {cap}, S = {S} trials, N = {N}, energy = {energy:g}, {spent['rounds']} rounds, "
                 "one run after a warm-up run [ms per round]")
    lines.append(f"    total {total / n * 1e3:.1f} = solve {spent['solve'] / n * 1e3:.1f} + row formatting {spent['rows'] / n * 1e3:.1f} + loop glue "
                 f"{glue / n * 1e3:.1f}   (glue includes the closing rollout and rows, once per run)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "swarm_study.txt"))
    args = ap.parse_args()
    from dpilqr_amd import _lib
    _lib.require_gpu()
    lines = ["swarm study: scripts/bench_swarm_study.py on one MI355X (wall clock, host timers around synchronised calls)", ""]
    draw_inputs(lines)
    study_cell(lines)
    lines += ["", "Not measured: counters (none collected), the kernel's own time apart from the launch and the allocations of its four",
              "outputs (the device column is the whole call), other models, energies or caps, and the study above one cell."]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
