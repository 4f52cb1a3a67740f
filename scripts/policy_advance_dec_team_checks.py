#!/usr/bin/env python
"""The team receding-horizon advance on the cases of tests/policy_dec_team_cases.py (tests/policy_advance_dec_team_cases.py): the
reference-alone figures that keep the cases honest on the executed prefixes and, with a GPU, the largest measured error of every
case, variant and h beside the bound it was held to and the share of scenarios without a bound, the cross-check against
policy_advance_dec and the kernels' resources in the built library.  Writes profiles/policy_advance_dec_team_checks.txt.  Nothing
is asserted here: the tests (tests/test_policy_advance_dec_team_host.py, tests/test_gpu_policy_advance_dec_team.py) hold what this
records.  --mutants FILE appends a record of mutant runs (which test caught which arithmetic-only change of the kernel), taken on
scratch copies of the tree.

    python scripts/policy_advance_dec_team_checks.py [--cpu-only] [--mutants FILE] [--out profiles/policy_advance_dec_team_checks.txt]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--mutants", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance_dec_team_checks.txt"))
    a = ap.parse_args()
    import numpy as np
    from tests import policy_advance_cases as ac
    from tests import policy_advance_dec_team_cases as atc
    from tests import policy_cases as pc
    from tests import policy_dec_cases as dc
    from tests import policy_dec_team_cases as tc
    lines = ["team receding-horizon advance (dpilqr_policy_advance_dec_team): the cases of tests/policy_dec_team_cases.py, every (item, sample) "
             "one scenario, T = %d, B = %d" % (atc.T, atc.B), "",
             "1. from the CPU reference alone, on the prefix of h steps: share of clamped control entries (u_lim variant), of samples inside the "
             "radius (W variant), of samples without a bound per variant (cap %.2f)" % pc.MAX_UNCHECKED]
    for case in atc.CASES:
        ref = tc.case_ref(case)
        for h in (1, 3):
            f = atc.prefix_figures(case, ref, h)
            lines.append("%-26s h=%d clamped %.4f near %.4f unchecked plain %.4f W %.4f u_lim %.4f  (%d scenarios, %d per workgroup)"
                         % (case.id, h, f["clamped"], f["near"], f["unchecked"]["plain"], f["unchecked"]["W"], f["unchecked"]["u_lim"],
                            atc.B * case.S, 256 // case.k))
    section = 2
    if not a.cpu_only:
        import __graft_entry__ as g
        g.build(verbose=False)
        from tests import test_gpu_policy_advance_dec_team as tg
        lines += ["", "2. on the GPU: per case, variant and h the largest error / bound ratio of J_exec, min_sep, dist_left over the scenarios, "
                  "that scenario's error and its bound max(1e-9, 100 x the reference's own spread), the share of scenarios without a bound; "
                  "X_exec / U_exec against policy_rollout_dec_team's prefix: same bits?"]
        for case in atc.CASES:
            ref, rp, pb, scen = tg.setup(case)
            for v in atc.VARIANTS:
                roll = tg.rollout(case, v)
                for h in atc.HS:
                    st = tg.advance(case, v, h)
                    worst, d, bound, unchecked, failures = tg.worst_against_reference(case, v, h, st, scen)
                    same = bool(np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1]) and np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h]))
                    lines.append("%-26s %-5s h=%d error %.3g bound %.3g ratio %.3g  without a bound %.4f (%d of %d)  beyond their bound %d  prefix same bits: %s"
                                 % (case.id, v, h, d, bound, worst, unchecked / (atc.B * case.S), unchecked, atc.B * case.S, len(failures), same))
        lines += ["", "3. against policy_advance_dec on cases both serve (same inputs): X_exec, U_exec, x_cur, n_done, dist_left, U_next, X_next "
                  "bit for bit?  J_exec and min_sep: largest relative difference (tolerance %.0e)" % pc.TOL_ROLLOUT]
        for case in atc.CROSS:
            ref = dc.case_ref(case)
            rp = atc.repeated(case, ref)
            pb, scen = ac.problem_batch(case, ref.batch, repeat=case.S), ac.scen_of(case, rp["n"])
            n_state = rp["n"] + atc.SPARE
            for v in atc.VARIANTS:
                _, lim = ref.args(v)
                W = tg._state_W(rp["W"], scen, n_state, atc.T) if v == "W" else None
                for h in atc.HS:
                    run = lambda f: tg._host(f(rp["X"], rp["U"], rp["Kc"], rp["masks"], h, tg._nan_state(pb, n_state, atc.T, scen, rp["x0"]),
                                               scen=scen, W=W, u_lim=lim, n_d=atc.N_D))
                    old, new = run(pb.policy_advance_dec), run(pb.policy_advance_dec_team)
                    same = all(np.array_equal(old[f], new[f], equal_nan=True) for f in tg.BITWISE)
                    eJ = float(np.max(np.abs(new["J_exec"][scen] - old["J_exec"][scen]) / np.abs(old["J_exec"][scen])))
                    eS = float(np.max(np.abs(new["min_sep"][scen] - old["min_sep"][scen]) / np.abs(old["min_sep"][scen])))
                    lines.append("%-26s %-5s h=%d the seven fields same bits: %s; J_exec %.2e min_sep %.2e" % (case.id, v, h, same, eJ, eS))
        section = 4
    import kernel_resources
    from tests.policy_dec_wide_cases import kernel_names
    if (kernel_resources.LLVM / "llvm-readelf").exists() and (ROOT / "dpilqr_amd" / "libdpilqr_hip.so").exists():
        lines += ["", "%d. kernel resources of the built library (scripts/kernel_resources.py), no unit flag" % section]
        section += 1
        for r in kernel_resources.resources():
            if r["demangled"] in kernel_names("k_policy_advance_dec_team"):      # the one-word instantiations
                lines.append("%-36s vgpr %3d agpr %3d sgpr %3d spill v %d scratch %d B  static lds %5d B  wg %d"
                             % (r["demangled"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
                                r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"]))
    if a.mutants:
        lines += ["", "%d. mutants: arithmetic-only changes of k_policy_advance_dec_team, each built on a scratch copy of the tree and run against "
                  "tests/test_gpu_policy_advance_dec_team.py (no mutant removes a barrier, a bounds test or an activity test)" % section]
        lines += Path(a.mutants).read_text().rstrip().splitlines()
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
