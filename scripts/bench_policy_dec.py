#!/usr/bin/env python
"""Launch time of the neighbourhood-sparse closed-loop rollout (dpilqr_policy_rollout_dec, csrc/policy_dec.hpp) against its
yardstick, the dense dpilqr_policy_rollout fed the SAME policy expanded to K[S][T][n_u][n_x] with zeros outside the
neighbourhoods.  Nothing is asserted.

Workloads: 1024 scenarios x 64 samples of the Monte-Carlo study's setups (analysis.trial_inputs / build_problem, radius 0.5) for
cfg2's shape (five DoubleIntDynamics4D, T = 50) and for ten QuadcopterDynamics6D at T = 75.  Per workload one distributed solve
with policy=True supplies the policy with the cluster sizes a real solve produces ("real"); two extremes are cut from the same
gains: every agent alone (kc_max = 1: its own diagonal block) and every agent seeing everyone (kc_max = k: the dense rows
regrouped).  Per row: median (min .. max) of --reps launches after a warm-up (HIP events), trajectories not stored, the ratio
sparse / dense, and the algorithmic K bytes per step and workgroup, k n_c kc_max n_s 8 against n_u n_x 8.  The "real" rows also
give the stitch of gains (dpilqr_dispatch_stitch_policy) as a share of the distributed solve's wall time.
Every workload runs in a child process under its own time limit; after a failure nothing more is started.

    python scripts/bench_policy_dec.py [--reps 7] [--scenarios 1024] [--samples 64] [--out profiles/policy_dec_rollout.txt]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {"cfg2_5xDoubleInt4D_T50": ("DoubleIntDynamics4D", 5, 50, 2), "10xQuadcopter6D_T75": ("QuadcopterDynamics6D", 10, 75, 3)}
RADIUS, DT, MU = 0.5, 0.1, 1.0


def one(name, n_scen, n_samples, reps):
    import numpy as np
    import torch
    import dpilqr_amd as dp
    from dpilqr_amd import analysis
    model_name, k, T, n_d = WORKLOADS[name]
    model = getattr(dp, model_name)
    ns = model(-1).n_x
    nc = model(-1).n_u
    n, m = k * ns, k * nc
    x0 = np.zeros((n_scen, n)); xf = np.zeros((n_scen, n))
    for s in range(n_scen):
        a, b, _, _ = analysis.trial_inputs(k, ns, m, T, 10.0, n_d, analysis.seed_of(model, k, s))
        x0[s], xf[s] = a.ravel(), b.ravel()
    dp._reset_ids()
    problem = analysis.build_problem(model, k, DT, RADIUS, xf[0], n_d)
    U0 = np.zeros((n_scen, T, m))
    kw = dict(xf=xf, device_out=True, policy=True, policy_mu=MU)
    dp.solve_scenarios_distributed(problem, x0[:, None, :], U0, RADIUS, **kw)      # warm-up: allocator, workspaces, code objects
    X_dec, U_dec, J, info = dp.solve_scenarios_distributed(problem, x0[:, None, :], U0, RADIUS, **kw)
    pol = info["policy"]
    sec = info["seconds"]
    pb = pol.batch()
    dev = X_dec.device
    bits = pol.bits.cpu().numpy().astype(np.uint64)
    sizes = np.zeros((n_scen, k), dtype=np.int64)
    for j in range(k):
        sizes += ((bits >> np.uint64(j)) & np.uint64(1)).astype(np.int64)
    gen = torch.Generator(dev).manual_seed(1)
    x0s = X_dec[:, :1, :] + 0.05 * torch.randn((n_scen, n_samples, n), dtype=torch.float64, device=dev, generator=gen)

    # the policy expanded to dense: block (a, j) of K is block rank_a(j) of agent a's compact row where bit j is set
    Kc = pol.Kc
    K_dense = torch.zeros((n_scen, T, m, n), dtype=torch.float64, device=dev)
    for a in range(k):
        for j in range(k):
            has = ((bits[:, a] >> np.uint64(j)) & np.uint64(1)).astype(bool)
            rank = np.zeros(n_scen, dtype=np.int64)
            for q in range(j):
                rank += ((bits[:, a] >> np.uint64(q)) & np.uint64(1)).astype(np.int64)
            for p in np.unique(rank[has]):
                sel = torch.as_tensor(np.nonzero(has & (rank == p))[0], device=dev)
                K_dense[sel, :, a * nc:(a + 1) * nc, j * ns:(j + 1) * ns] = Kc[sel, :, a, :, p * ns:(p + 1) * ns]

    def timed(fn):
        fn(); torch.cuda.synchronize()      # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    own = torch.as_tensor(np.tile(np.uint64(1) << np.arange(k, dtype=np.uint64), (n_scen, 1)).view(np.int64), device=dev)
    full = torch.full((n_scen, k), (1 << k) - 1, dtype=torch.int64, device=dev)
    Kc_alone = torch.stack([K_dense[:, :, a * nc:(a + 1) * nc, a * ns:(a + 1) * ns] for a in range(k)], dim=2).contiguous()
    K_alone = torch.zeros_like(K_dense)
    for a in range(k):
        K_alone[:, :, a * nc:(a + 1) * nc, a * ns:(a + 1) * ns] = Kc_alone[:, :, a]
    Kc_full = K_dense.reshape(n_scen, T, k, nc, n).contiguous()
    rows = []
    for mode, kc_max, Kc_m, bits_m, Kd in (("real", pol.kc_max, Kc, pol.bits, K_dense), ("all alone", 1, Kc_alone, own, K_alone),
                                           ("all full", k, Kc_full, full, K_dense)):
        pb.policy_rollout_dec(X_dec, pol.U_ff, Kc_m, bits_m, x0s)      # the first call reads the masks back and checks them
        sparse = timed(lambda: pb.policy_rollout_dec(X_dec, pol.U_ff, Kc_m, bits_m, x0s, masks_checked=bits_m))
        dense = timed(lambda: pb.policy_rollout(X_dec, pol.U_ff, Kd, x0s))
        rows.append(dict(mode=mode, kc_max=int(kc_max), sparse_ms=sparse, dense_ms=dense, k_bytes_sparse=8 * k * nc * int(kc_max) * ns,
                         k_bytes_dense=8 * m * n))
    hist = {int(c): int((sizes == c).sum()) for c in range(1, k + 1) if (sizes == c).any()}
    print(json.dumps(dict(name=name, k=k, T=T, n_x=n, n_u=m, scenarios=n_scen, samples=n_samples, rows=rows, seconds=sec,
                          sizes=info["sizes"], agents_by_neighbourhood_size=hist)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenarios", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_rollout.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds per workload")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.scenarios, a.samples, a.reps)
    lines = ["neighbourhood-sparse closed-loop rollout against the dense kernel fed the same policy expanded with zeros; %d scenarios x %d samples, "
             "trajectories not stored; median (min .. max) of %d launches after a warm-up" % (a.scenarios, a.samples, a.reps),
             "%-24s %-10s %6s %24s %24s %7s %18s" % ("workload", "masks", "kc_max", "sparse ms", "dense ms", "ratio", "K B/step sparse/dense")]
    for name in WORKLOADS:
        p = subprocess.run([sys.executable, __file__, "--one", name, "--reps", str(a.reps), "--scenarios", str(a.scenarios),
                            "--samples", str(a.samples)], capture_output=True, text=True, timeout=a.limit)
        if p.returncode != 0:      # nothing more is started on the device after a failure
            lines.append(f"{name}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1:]}")
            Path(a.out).write_text("\n".join(lines) + "\n")
            print("\n".join(lines))
            return p.returncode
        d = json.loads(p.stdout.strip().splitlines()[-1])
        for r in d["rows"]:
            (sm, sl, sh), (dm, dl, dh) = r["sparse_ms"], r["dense_ms"]
            lines.append("%-24s %-10s %6d %9.3f (%6.3f..%6.3f) %9.3f (%6.3f..%6.3f) %7.2f %9d / %6d"
                         % (name, r["mode"], r["kc_max"], sm, sl, sh, dm, dl, dh, sm / dm, r["k_bytes_sparse"], r["k_bytes_dense"]))
        sec = d["seconds"]
        total = sum(sec.values())
        lines.append("  %s: unique sub-problems by size %s; agents by neighbourhood size %s" % (name, d["sizes"], d["agents_by_neighbourhood_size"]))
        lines.append("  distributed solve with policy=True, wall seconds: " + ", ".join(f"{k_} {v:.4f}" for k_, v in sec.items())
                     + "; stitch of gains %.2f %% of %.4f s (the buckets' backward passes are inside `solves`)" % (100 * sec["stitch_policy"] / total, total))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
