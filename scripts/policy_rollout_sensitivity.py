#!/usr/bin/env python
"""profiles/policy_rollout_sensitivity.txt: per case of tests/test_gpu_policy.py the reference-alone figures (share of samples
without a bound, largest sensitivity among the bounded ones, clamped share of the u_lim run, share of samples inside the
radius, share of samples whose cost the perturbed start moves by 1 % and more) and, on a GPU, the worst measured
error / bound ratio of every variant.

    python scripts/policy_rollout_sensitivity.py [--no-gpu] [--out profiles/policy_rollout_sensitivity.txt]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import policy_cases as pc   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_rollout_sensitivity.txt"))
    a = ap.parse_args()
    lines = ["closed-loop ensemble rollout (dpilqr_policy_rollout) against the CPU reference: tests/policy_cases.py, T = %d, B = %d" % (pc.T, pc.B),
             "bound per sample: max(%g, %g x the reference's own change under %g relative perturbations of x0s, K, X, U); unchecked beyond %g"
             % (pc.lc.TOL_PASS, pc.lc.SPREAD_FACTOR, pc.lc.PERTURB, pc.lc.SPREAD_CAP), ""]
    if not a.no_gpu:
        from tests import test_gpu_policy as tg
    for case in pc.CASES:
        ref = pc.case_ref(case)
        f = ref.figures()
        lines.append(f"{case.id}: k {case.k}, S {case.S}, sigma {case.sigma}, radius {case.radius}, weights {case.weights}")
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
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
