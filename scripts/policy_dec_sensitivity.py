#!/usr/bin/env python
"""profiles/policy_dec_sensitivity.txt: per case of tests/test_gpu_policy_dec.py the masks of item 2 and the reference-alone
figures (share of samples without a bound, largest sensitivity among the bounded ones, clamped share of the u_lim run, share of
samples inside the radius, share of samples whose cost the perturbed start moves by 1 % and more) and, on a GPU, the worst
measured error / bound ratio of every variant; then, on a GPU, per case of tests/policy_cases.py whether the sparse kernel fed
full masks returns the dense kernel's results bit for bit (recorded here; tests/test_gpu_policy_dec.py asserts it).

    python scripts/policy_dec_sensitivity.py [--no-gpu] [--out profiles/policy_dec_sensitivity.txt]"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import policy_cases as pc       # noqa: E402
from tests import policy_dec_cases as dc   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_sensitivity.txt"))
    a = ap.parse_args()
    lines = ["neighbourhood-sparse closed-loop rollout (dpilqr_policy_rollout_dec) against the CPU reference fed the masked dense gains: "
             "tests/policy_dec_cases.py, T = %d, B = %d" % (pc.T, pc.B),
             "masks: item 0 full, item 1 every agent alone, item 2 as listed; unused columns of Kc hold NaN",
             "bound per sample: max(%g, %g x the reference's own change under %g relative perturbations of x0s, K, X, U); unchecked beyond %g"
             % (pc.lc.TOL_PASS, pc.lc.SPREAD_FACTOR, pc.lc.PERTURB, pc.lc.SPREAD_CAP), ""]
    if not a.no_gpu:
        from tests import test_gpu_policy_dec as tg
    for case in dc.CASES:
        ref = dc.case_ref(case)
        f = ref.figures()
        lines.append(f"{case.id}: k {case.k}, S {case.S}, sigma {case.sigma}, radius {case.radius}, weights {case.weights}, "
                     f"item 2 masks {[hex(int(m)) for m in ref.masks[2]]}")
        lines.append("  reference alone: clamped %.3f  inside radius %.3f  J moved >= 1 %% %.3f" % (f["clamped"], f["near"], f["moved"]))
        for v in ("plain", "W", "u_lim"):
            row = "  %-6s unchecked %.3f  largest bounded sensitivity %.2e" % (v, f["unchecked"][v], f["max_spread"][v])
            if not a.no_gpu:
                got = tg.gpu_runs(case)[v]
                worst = 0.0
                for i in range(pc.B):
                    for s in range(case.S):
                        bound = pc.bound_of(ref.spread[v][i, s])
                        if bound is None:
                            continue
                        g = dict(X=got["X"][i, s], U=got["U"][i, s], J=float(got["J"][i, s]), min_sep=float(got["min_sep"][i, s]),
                                 goal_dist=got["goal_dist"][i, s])
                        worst = max(worst, pc.difference(g, ref.ref[v][i][s]) / bound)
                row += "  GPU worst error / bound %.3g" % worst
            lines.append(row)
    lines += ["", "all masks full against the dense kernel (dpilqr_policy_rollout) on the same K, cases of tests/policy_cases.py:"]
    if a.no_gpu:
        lines.append("  not run (no GPU)")
    else:
        for case in pc.CASES:
            ref = pc.case_ref(case)
            b, k = ref.batch, case.k
            pb = tg._pb(case, b)
            masks = np.full((pc.B, k), (1 << k) - 1, dtype=np.uint64)
            Kc = dc.compact_gains(ref.K, masks, case.ns, case.nc, k)
            same = []
            for v in tg.VARIANTS:
                W, lim = ref.args(v)
                dense = tg._host(pb.policy_rollout(ref.X, ref.U, ref.K, b["x0s"], W=W, u_lim=lim, trajectories=True))
                dec = tg._host(pb.policy_rollout_dec(ref.X, ref.U, Kc, masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
                same.append(all(np.array_equal(dense[key], dec[key]) for key in dense))
            lines.append("  %-22s bit-identical (plain, W, u_lim): %s" % (case.id, same))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
