#!/usr/bin/env python
"""The team closed-loop rollout's cases (tests/policy_dec_team_cases.py): the reference-alone figures that keep them honest and,
with a GPU, the largest measured error of every case and variant beside its bound, the cross-check against policy_rollout_dec and
the kernels' resources in the built library.  Writes profiles/policy_dec_team_checks.txt.  Nothing is asserted here: the tests
(tests/test_policy_dec_team_host.py, tests/test_gpu_policy_dec_team.py) hold what this records.

    python scripts/policy_dec_team_checks.py [--cpu-only] [--out profiles/policy_dec_team_checks.txt]"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_team_checks.txt"))
    a = ap.parse_args()
    import numpy as np
    from tests import policy_cases as pc
    from tests import policy_dec_cases as dc
    from tests import policy_dec_team_cases as tc
    lines = ["team closed-loop rollout (dpilqr_policy_rollout_dec_team): the cases of tests/policy_dec_team_cases.py, T = %d, B = %d" % (tc.T, tc.B), "",
             "1. from the CPU reference alone: share of clamped control entries (u_lim variant), of samples inside the radius, of samples whose "
             "cost the start moves by a hundredth, of samples without a bound per variant (cap %.2f); seconds of the case's CPU side" % pc.MAX_UNCHECKED]
    for case in tc.CASES:
        t0 = time.perf_counter()
        f = tc.case_ref(case).figures()
        lines.append("%-26s clamped %.4f near %.4f moved %.4f unchecked plain %.4f W %.4f u_lim %.4f  (%.1f s)"
                     % (case.id, f["clamped"], f["near"], f["moved"], f["unchecked"]["plain"], f["unchecked"]["W"], f["unchecked"]["u_lim"],
                        time.perf_counter() - t0))
    if not a.cpu_only:
        import __graft_entry__ as g
        g.build(verbose=False)
        from tests import test_gpu_policy_dec_team as tg
        lines += ["", "2. on the GPU: per case and variant the largest error / bound ratio of X, U, J, min_sep, goal_dist over the samples "
                  "(policy_cases.difference), that sample's error and its bound max(1e-9, 100 x the reference's own spread), samples without a bound"]
        for case in tc.CASES:
            runs = tg.gpu_runs(case)
            for v in tg.VARIANTS:
                worst, d, bound, unchecked, failures = tg.worst_against_reference(case, v, runs[v])
                same = all(np.array_equal(runs[v][key], runs[v + "-nostore"][key]) for key in ("J", "min_sep", "goal_dist"))
                lines.append("%-26s %-5s error %.3g bound %.3g ratio %.3g  unchecked %d of %d  beyond their bound %d  trajectories=False same bits: %s"
                             % (case.id, v, d, bound, worst, unchecked, tc.B * case.S, len(failures), same))
        lines += ["", "3. against policy_rollout_dec on cases both serve (same inputs): X, U, goal_dist bit for bit?  J and min_sep: largest "
                  "relative difference (tolerance %.0e)" % pc.TOL_ROLLOUT]
        for case in tc.CROSS:
            ref = dc.case_ref(case)
            b = ref.batch
            pb = tg._pb(case, b)
            Kc = dc.compact_gains(ref.K, ref.masks, case.ns, case.nc, case.k)
            for v in tg.VARIANTS:
                W, lim = ref.args(v)
                old = tg._host(pb.policy_rollout_dec(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
                new = tg._host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
                bits = {key: bool(np.array_equal(old[key], new[key])) for key in ("X", "U", "goal_dist", "J", "min_sep")}
                eJ = float(np.max(np.abs(new["J"] - old["J"]) / np.abs(old["J"])))
                eS = float(np.max(np.abs(new["min_sep"] - old["min_sep"]) / np.abs(old["min_sep"])))
                lines.append("%-26s %-5s same bits: X %s U %s goal_dist %s J %s min_sep %s; J %.2e min_sep %.2e"
                             % (case.id, v, bits["X"], bits["U"], bits["goal_dist"], bits["J"], bits["min_sep"], eJ, eS))
    import kernel_resources
    from tests.policy_dec_wide_cases import kernel_names
    if (kernel_resources.LLVM / "llvm-readelf").exists() and (ROOT / "dpilqr_amd" / "libdpilqr_hip.so").exists():
        lines += ["", "%d. kernel resources of the built library (scripts/kernel_resources.py), no unit flag" % (2 if a.cpu_only else 4)]
        for r in kernel_resources.resources():
            if r["demangled"] in kernel_names("k_policy_rollout_dec_team"):      # the one-word instantiations
                lines.append("%-36s vgpr %3d agpr %3d sgpr %3d spill v %d scratch %d B  static lds %5d B  wg %d"
                             % (r["demangled"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
                                r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"]))
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
