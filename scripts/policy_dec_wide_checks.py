#!/usr/bin/env python
"""The wide closed-loop rollout's cases (tests/policy_dec_wide_cases.py): the reference-alone figures that keep them honest and,
with a GPU, the largest measured error of every case and variant beside its bound, the n_words = 1 cross-check against
policy_rollout_dec_team, the kernels' resources in the built library, and MUTANTS of the two new kernels with the tests that catch
each.  Writes profiles/policy_dec_wide_checks.txt.  Nothing is asserted here: the tests (tests/test_policy_dec_wide_host.py,
tests/test_gpu_policy_dec_wide.py) hold what this records.

A mutant is one statement of csrc/policy_dec_team.hpp or csrc/frontend_wide.hpp changed in a copy under build/mutants/, that
copy's translation unit compiled and linked with the current objects of the others into dpilqr_amd/variants/ (git-ignored).
Every mutant keeps every address inside the arrays the kernel is given (the reason stands beside each below): they compute
wrong numbers, nothing else.  --build-mutants needs hipcc and no GPU; a run with a GPU then takes each library that is there
through tests/test_gpu_policy_dec_wide.py in a child process of its own (DPILQR_DEBUG_ROUTES=1 DPILQR_LIB=...), under a time
limit, one at a time, and starts nothing more after a child that did not end as pytest ends.

    python scripts/policy_dec_wide_checks.py --build-mutants
    python scripts/policy_dec_wide_checks.py [--cpu-only] [--out profiles/policy_dec_wide_checks.txt]"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
CSRC = ROOT / "dpilqr_amd" / "csrc"
VARIANTS_DIR = ROOT / "dpilqr_amd" / "variants"

# name -> (unit, header, the statement, its replacement, what it does, why it stays inside its arrays)
MUTANTS = {
    "words_reversed": ("tu_policy_dec_wide", "policy_dec_team.hpp",
                       "for (int w = 0; w < NW; ++w)      // word by word, lowest bit first: the members in ascending order",
                       "for (int w = NW - 1; w >= 0; --w)",
                       "the members of the higher words are walked before those of word 0",
                       "the same members (< k) and the same number of blocks (<= kc_max), in another order"),
    "word_offset_dropped": ("tu_policy_dec_wide", "policy_dec_team.hpp",
                            "pos, 64 * w + __ffsll(rem) - 1, 1, kw, AS);",
                            "pos, __ffsll(rem) - 1, 1, kw, AS);",
                            "a member of word w is taken for agent b instead of 64 w + b",
                            "b < 64 and, in word 0, b < k: a row of the sample's own dx"),
    "half_offset_by_every_lane": ("tu_policy_dec_wide", "policy_dec_team.hpp",
                                  "if (2 * dd == k && a >= dd) break;",
                                  "",
                                  "at even k every lane takes the offset k / 2: those pairs count twice",
                                  "the partner a + dd mod k is < k as for every other offset"),
    "rank_in_own_word": ("tu_frontend", "frontend_wide.hpp",
                         "for (int w = 0; w < (i >> 6); ++w) p += __popcll(m[w]);",
                         "",
                         "an owner's rank among its neighbourhood counts the lower members of its own word only",
                         "the rank only shrinks: 0 <= pos < kc still"),
}
TEST_FILE = "tests/test_gpu_policy_dec_wide.py"
FAULT_CODES = {124, 134, 137, 139, -6, -9, -11}


def build_mutants():
    import __graft_entry__ as g
    g.build(need_objects=True, verbose=False)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    VARIANTS_DIR.mkdir(exist_ok=True)
    for name, (unit, header, old, new, _, _) in MUTANTS.items():
        d = ROOT / "build" / "mutants" / name
        d.mkdir(parents=True, exist_ok=True)
        text = (CSRC / header).read_text()
        assert text.count(old) == 1, (name, text.count(old))
        (d / header).write_text(text.replace(old, new))
        shutil.copy(CSRC / (unit + ".hip"), d / (unit + ".hip"))      # its quoted includes find the changed header beside it first
        obj = d / (unit + ".o")
        subprocess.run([hipcc, *g.HIPCC_FLAGS, *g.UNIT_FLAGS.get(unit, []), "-c", "-o", str(obj), str((d / (unit + ".hip")).relative_to(ROOT))],
                       cwd=ROOT, check=True)
        objs = [str(obj if p.stem == unit else g.OBJ_DIR / (p.stem + ".o")) for p in sorted(CSRC.glob("*.hip"))]
        out = VARIANTS_DIR / f"libdpilqr_hip_mutant_{name}.so"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(out), *objs], check=True)
        print("built", out.relative_to(ROOT))
    return 0


def run_mutants(lines, limit):
    lines += ["", "5. mutants (one statement changed; the library linked from the other units' current objects) run through "
              + TEST_FILE + ": the tests that fail"]
    for name, (unit, header, old, new, what, safe) in MUTANTS.items():
        so = VARIANTS_DIR / f"libdpilqr_hip_mutant_{name}.so"
        lines.append(f"{name}: csrc/{header}: {what}  [in bounds: {safe}]")
        if not so.exists():
            lines.append("    not built (python scripts/policy_dec_wide_checks.py --build-mutants)")
            continue
        env = dict(os.environ, DPILQR_DEBUG_ROUTES="1", DPILQR_LIB=str(so))
        try:
            p = subprocess.run([sys.executable, "-m", "pytest", TEST_FILE, "-q", "--tb=no", "-rf", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=limit)
            rc, out = p.returncode, p.stdout
        except subprocess.TimeoutExpired:
            rc, out = 124, ""
        failed = re.findall(r"^FAILED \S+?::(\S+)", out, re.M)
        tail = [ln for ln in out.strip().splitlines() if " passed" in ln or " failed" in ln][-1:]
        lines.append(f"    exit status {rc}; {' '.join(tail).strip('= ')}")
        by_test = {}
        for f in failed:
            by_test.setdefault(f.split("[")[0], []).append(f[f.index("[") + 1:-1] if "[" in f else "")
        for t, ids in by_test.items():
            lines.append(f"    caught by {t}" + (f" [{', '.join(ids)}]" if any(ids) else ""))
        if not failed and rc == 0:
            lines.append("    NOT CAUGHT")
        if rc in FAULT_CODES or rc not in (0, 1):      # not how pytest ends: nothing more is started on the device
            lines.append("    the child did not end as pytest ends: no further mutant is run")
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--build-mutants", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds per mutant")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "policy_dec_wide_checks.txt"))
    a = ap.parse_args()
    if a.build_mutants:
        return build_mutants()
    import numpy as np
    from tests import policy_cases as pc
    from tests import policy_dec_wide_cases as wc
    lines = ["wide closed-loop rollout (dpilqr_policy_rollout_dec_wide): the cases of tests/policy_dec_wide_cases.py, T = %d, B = %d" % (wc.T, wc.B), "",
             "1. from the CPU reference alone: share of clamped control entries (u_lim variant), of samples inside the radius, of samples whose "
             "cost the start moves by a hundredth, of samples without a bound per variant (cap %.2f), the largest finite spread; seconds of the "
             "case's CPU side" % pc.MAX_UNCHECKED]
    for case in wc.CASES:
        t0 = time.perf_counter()
        f = wc.case_ref(case).figures()
        lines.append("%-24s kc_max %d  clamped %.4f near %.4f moved %.4f unchecked plain %.4f W %.4f u_lim %.4f  spread %.2e  (%.1f s)"
                     % (case.id, case.kc_max, f["clamped"], f["near"], f["moved"], f["unchecked"]["plain"], f["unchecked"]["W"],
                        f["unchecked"]["u_lim"], max(f["max_spread"].values()), time.perf_counter() - t0))
    rc = 0
    if not a.cpu_only:
        import __graft_entry__ as g
        g.build(verbose=False)
        from tests import test_gpu_policy_dec_wide as tg
        lines += ["", "2. on the GPU: per case and variant the largest error / bound ratio of X, U, J, min_sep, goal_dist over the samples "
                  "(policy_cases.difference), that sample's error and its bound max(1e-9, 100 x the reference's own spread), samples without a bound"]
        for case in wc.CASES:
            runs = tg.gpu_runs(case)
            for v in tg.VARIANTS:
                worst, d, bound, unchecked, failures = tg.worst_against_reference(case, v, runs[v])
                same = all(np.array_equal(runs[v][key], runs[v + "-nostore"][key]) for key in ("J", "min_sep", "goal_dist"))
                lines.append("%-24s %-5s error %.3g bound %.3g ratio %.3g  unchecked %d of %d  beyond their bound %d  trajectories=False same bits: %s"
                             % (case.id, v, d, bound, worst, unchecked, wc.B * case.S, len(failures), same))
        lines += ["", "3. n_words = 1 against policy_rollout_dec_team (same inputs): the results that differ in any bit, per variant (none: all five "
                  "of X, U, J, min_sep, goal_dist are equal)"]
        for case, case_ref in tg.ONE_WORD:
            differ = tg.one_word_equal(case, case_ref)
            lines.append("%-26s k %2d  " % (case.id, case.k) + "  ".join("%s: %s" % (v, ", ".join(keys) if keys else "none") for v, keys in differ.items()))
    import kernel_resources
    if (kernel_resources.LLVM / "llvm-readelf").exists() and (ROOT / "dpilqr_amd" / "libdpilqr_hip.so").exists():
        lines += ["", "%d. kernel resources of the built library (scripts/kernel_resources.py), no unit flag; the four-word instantiations beside the one-word ones"
                  % (2 if a.cpu_only else 4)]
        shown = wc.kernel_names("k_policy_rollout_dec_wide") + wc.kernel_names("k_policy_rollout_dec_team")
        for r in kernel_resources.resources():
            if r["demangled"] in shown or "k_stitch_policy" in r["demangled"]:
                lines.append("%-36s vgpr %3d agpr %3d sgpr %3d spill v %d scratch %d B  static lds %5d B  wg %d"
                             % (r["demangled"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"],
                                r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"]))
    if not a.cpu_only:
        rc = run_mutants(lines, a.limit)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main())
