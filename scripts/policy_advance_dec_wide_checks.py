#!/usr/bin/env python
"""The wide receding-horizon advance on the cases of tests/policy_dec_wide_cases.py (tests/policy_advance_dec_wide_cases.py): the
reference-alone figures that keep the cases honest on the executed prefixes and, with a GPU, the largest measured error of every
case, variant and h as a share of the bound it was held to, the one-word cross-check against policy_advance_dec_team, cost_wide
against the oracle, the kernels' resources in the built library and the register-or-LDS decision for the mask words.  Writes
profiles/policy_advance_dec_wide_checks.txt.  Nothing is asserted here: the tests (tests/test_policy_advance_dec_wide_host.py,
tests/test_gpu_policy_advance_dec_wide.py) hold what this records.  --masks-in-lds FILE appends the resource table of the variant
with the mask words in LDS (built apart, never shipped); --mutants FILE appends a record of mutant runs (which test caught which
arithmetic-only change of the kernel), taken on builds apart from the shipped library.

    python scripts/policy_advance_dec_wide_checks.py [--cpu-only] [--masks-in-lds FILE] [--mutants FILE] [--out FILE]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

ROW = "%-36s vgpr %3d agpr %3d sgpr %3d spill v %d scratch %d B  static lds %5d B  wg %d"


def resource_rows(so_path, stem):
    """The rows of the five kernels recorded as `stem<NS, NC>`, under today's names (tests/policy_dec_wide_cases.py: kernel_names)."""
    import kernel_resources
    from tests.policy_dec_wide_cases import kernel_names
    names = kernel_names(stem)
    return [ROW % (r["demangled"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"],
                   r["group_segment_fixed_size"], r["max_flat_workgroup_size"])
            for r in kernel_resources.resources(so_path) if r["demangled"] in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--masks-in-lds", default=None)
    ap.add_argument("--mutants", default=None)
    ap.add_argument("--resources-of", default=None, help="print the resource rows of the wide advance in this shared library and stop")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_advance_dec_wide_checks.txt"))
    a = ap.parse_args()
    if a.resources_of:
        print("\n".join(resource_rows(a.resources_of, "k_policy_advance_dec_wide")))
        return 0
    import numpy as np
    from tests import policy_advance_dec_wide_cases as awc
    from tests import policy_cases as pc
    from tests import policy_dec_wide_cases as wc
    lines = ["wide receding-horizon advance (dpilqr_policy_advance_dec_wide): the cases of tests/policy_dec_wide_cases.py, every (item, sample) "
             "one scenario, T = %d, B = %d" % (awc.T, awc.B), "",
             "1. from the CPU reference alone, on the prefix of h steps: share of clamped control entries (u_lim variant), of samples inside the "
             "radius (W variant), of samples without a bound per variant (cap %.2f)" % pc.MAX_UNCHECKED]
    for case in awc.CASES:
        ref = wc.case_ref(case)
        for h in (1, 3):
            f = awc.prefix_figures(case, ref, h)
            lines.append("%-24s h=%d clamped %.4f near %.4f unchecked plain %.4f W %.4f u_lim %.4f  (%d scenarios run, %d per workgroup, %d words)"
                         % (case.id, h, f["clamped"], f["near"], f["unchecked"]["plain"], f["unchecked"]["W"], f["unchecked"]["u_lim"],
                            len(awc.kept(case)), 256 // case.k, case.n_words))
    section = 2
    if not a.cpu_only:
        import __graft_entry__ as g
        g.build(verbose=False)
        from tests import test_gpu_policy_advance_dec_wide as tg
        lines += ["", "2. on the GPU: per case, variant and h the largest error of J_exec, min_sep, dist_left over the scenarios AS A SHARE OF ITS BOUND, "
                  "that scenario's error and its bound max(1e-9, 100 x the reference's own spread), the share of scenarios without a bound; "
                  "X_exec / U_exec against policy_rollout_dec_wide's prefix: same bits?"]
        for case in awc.CASES:
            ref, rp, pb, scen = tg.setup(case)
            for v in awc.VARIANTS:
                roll = tg.rollout(case, v)
                for h in awc.HS:
                    st = tg.advance(case, v, h)
                    worst, d, bound, unchecked, failures = tg.worst_against_reference(case, v, h, st, scen, rp)
                    same = bool(np.array_equal(st["X_exec"][scen, :h + 1], roll["X"][:, :h + 1]) and np.array_equal(st["U_exec"][scen, :h], roll["U"][:, :h]))
                    lines.append("%-24s %-5s h=%d share of bound %.3g (error %.3g, bound %.3g)  without a bound %.4f (%d of %d)  beyond their bound %d  "
                                 "prefix same bits: %s" % (case.id, v, h, worst, d, bound, unchecked / rp["n"], unchecked, rp["n"], len(failures), same))
        lines += ["", "3. n_words = 1 against policy_advance_dec_team on the cases of tests/policy_dec_team_cases.py and its cross cases, masks reshaped "
                  "to (B, k, 1): per (variant, h) the fields among the nine that differ (none: bit for bit)"]
        for case, case_ref in tg.ONE_WORD:
            differ = tg.one_word_differences(case, case_ref)
            bad = {key: f for key, f in differ.items() if f}
            lines.append("%-26s k=%-2d %d (variant, h) runs: %s" % (case.id, case.k, len(differ), "all nine fields same bits" if not bad else bad))
        lines += ["", "4. cost_wide against the oracle's Problem.cost at the W variant's reference points (largest relative error; tolerance %.0e), and "
                  "against cost at k <= 64" % pc.TOL_ROLLOUT]
        for case in (awc.CASES[0], awc.CASES[5]):
            ref = wc.case_ref(case)
            pb = awc.problem_batch(case, ref.batch, np.arange(awc.B))
            pts = (0, 1, awc.T - 1)
            X = np.stack([[ref.ref["W"][i][0]["X"][t] for t in pts] for i in range(awc.B)])
            U = np.stack([[ref.ref["W"][i][0]["U"][t] for t in pts] for i in range(awc.B)])
            for terminal in (False, True):
                got = pb.cost_wide(X, U, terminal=terminal).cpu().numpy()
                want = np.array([[float(ref.problems[i].cost(X[i, q], U[i, q], terminal=terminal)) for q in range(len(pts))] for i in range(awc.B)])
                lines.append("%-24s terminal=%-5s %.3g" % (case.id, terminal, float(np.max(np.abs(got - want) / np.abs(want)))))
        from tests import policy_advance_cases as ac
        from tests import policy_dec_team_cases as tc
        for case in (tc.CASES[0], tc.CASES[-1]):
            ref = tc.case_ref(case)
            pb = ac.problem_batch(case, ref.batch)
            same = all(np.array_equal(pb.cost(ref.X[:, :awc.T], ref.U, terminal=t).cpu().numpy(), pb.cost_wide(ref.X[:, :awc.T], ref.U, terminal=t).cpu().numpy())
                       for t in (False, True))
            lines.append("%-26s k=%-2d cost_wide and cost same bits: %s" % (case.id, case.k, same))
        section = 5
    import kernel_resources
    so = ROOT / "dpilqr_amd" / "libdpilqr_hip.so"
    if (kernel_resources.LLVM / "llvm-readelf").exists() and so.exists():
        lines += ["", "%d. kernel resources of the built library (scripts/kernel_resources.py), no unit flag: the wide advance, then the team advance and the wide rollout "
                  "(unchanged against profiles/policy_advance_dec_team_checks.txt and profiles/policy_dec_wide_checks.txt)" % section]
        section += 1
        for stem in ("k_policy_advance_dec_wide", "k_policy_advance_dec_team", "k_policy_rollout_dec_wide"):
            lines += resource_rows(so, stem)
    if a.masks_in_lds:
        lines += ["", "%d. the mask words: registers or LDS.  Shipped: the four truncated words of a lane in REGISTERS (the table above: 0 spilled, 0 B "
                  "scratch in all five instantiations, the team advance's LDS).  The alternative -- the words in LDS, lane tid's word w at w * 256 + tid, "
                  "8 KB more -- built apart from the same source with that one change, for the record:" % section]
        section += 1
        lines += Path(a.masks_in_lds).read_text().rstrip().splitlines()
        lines.append("Neither form spills; the registers were the first choice and leave the LDS as it is, so they were taken.  Not measured: "
                     "the two forms' run time against one another.")
    if a.mutants:
        lines += ["", "%d. mutants: arithmetic-only changes of the wide advance (k_policy_advance_dec_team at four mask words), each built apart from the shipped library, loaded in its place and "
                  "run ONCE against tests/test_gpu_policy_advance_dec_wide.py (no mutant removes a barrier, a bounds test or an activity test; every "
                  "address stays inside the caller's buffers)" % section]
        lines += Path(a.mutants).read_text().rstrip().splitlines()
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
