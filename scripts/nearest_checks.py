#!/usr/bin/env python
"""Neighbourhoods capped at their m nearest agents on the cases of tests/nearest_cases.py: the figures the CPU alone gives (the cases'
margins, the conditioning of the oracle's capped solves), with a GPU the worst figure every test of tests/test_gpu_nearest.py prints
beside its bound, the kernel's resources in the built library, and -- from --mutants FILE -- the record of the mutant runs.  Writes
profiles/nearest_checks.txt.  Nothing is asserted here: the tests hold what this records.

The figures are the tests' own `[nearest ...]` lines: each test file runs ONCE, in a child process under a time limit, and its lines
are copied; after a fault, an abort or a time limit nothing more is started.
--mutants FILE: a record made apart from the shipped library -- four arithmetic-only changes of csrc/frontend_nearest.hpp (every address
stays inside the caller's buffers, no barrier and no bounds test is touched), each built into a library of its own, loaded in the
shipped one's place (DPILQR_DEBUG_ROUTES=1 DPILQR_LIB=...) and run once against the front-end tests.

--gpu-log FILE: take the GPU section's lines from this saved output of `pytest tests/test_gpu_nearest.py -q -s` (a run on a machine
with a GPU) instead of running the tests here.

    python scripts/nearest_checks.py [--cpu-only] [--gpu-log FILE] [--mutants FILE] [--out FILE]"""
import argparse
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

ROW = "%-28s vgpr %3d agpr %3d sgpr %3d spill v %d s %d scratch %d B  static lds %5d B  wg %d"


def test_lines(path, limit, extra=()):
    """(exit status, the `[nearest ...]` lines, pytest's last line) of one run of a test file"""
    try:
        p = subprocess.run([sys.executable, "-m", "pytest", path, "-q", "-s", "-p", "no:cacheprovider", *extra], cwd=ROOT, capture_output=True,
                           text=True, timeout=limit)
        rc, out = p.returncode, p.stdout
    except subprocess.TimeoutExpired as e:
        rc, out = 124, (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
    lines = [ln for ln in out.splitlines() if ln.startswith("[nearest")]
    tail = [ln for ln in out.splitlines() if re.search(r"\b(passed|failed|error)", ln)][-1:]
    return rc, lines, tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--mutants", default=None)
    ap.add_argument("--gpu-log", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nearest_checks.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build(verbose=False)
    lines = ["neighbourhoods capped at their m nearest agents (dpilqr_dispatch_graph_nearest, csrc/frontend_nearest.hpp): the cases of "
             "tests/nearest_cases.py", "",
             "1. from the CPU alone (tests/test_nearest_cases.py): per case the smallest key gap at the cut and the smallest |key - thr| over 3 scenarios "
             "in both forms (first row; 11 rows), and what a 1e-12 change of U0 does to the oracle's capped distributed solve"]
    rc, got, tail = test_lines("tests/test_nearest_cases.py", 600)
    lines += got + tail
    section = 2
    if not a.cpu_only and rc in (0, 1):
        lines += ["", "2. on the GPU (tests/test_gpu_nearest.py): every test's worst figure beside its bound"]
        if a.gpu_log:
            out = Path(a.gpu_log).read_text().splitlines()
            got, tail = [ln for ln in out if ln.startswith("[nearest")], [ln for ln in out if re.search(r"\b(passed|failed|error)", ln)][-1:]
        else:
            rc, got, tail = test_lines("tests/test_gpu_nearest.py", 540)
        lines += got + tail
        section = 3
        if rc not in (0, 1):
            lines.append(f"exit status {rc}: nothing more was started")
    import kernel_resources
    so = ROOT / "dpilqr_amd" / "libdpilqr_hip.so"
    if (kernel_resources.LLVM / "llvm-readelf").exists() and so.exists():
        lines += ["", "%d. kernel resources of the built library (scripts/kernel_resources.py), no unit flag; the LDS is dynamic: 2 x rows x k doubles "
                  "(77,824 B at k = 256 with 19 rows) + 4 strips of 256 keys (8,192 B) = 86,016 B at most.  k_graph_bits_wide beside them" % section]
        section += 1
        for r in kernel_resources.resources(so):
            if r["demangled"].startswith("k_graph_bits_nearest") or r["demangled"].endswith("k_graph_bits_wide"):
                lines.append(ROW % (r["demangled"], r["vgpr_count"], r["agpr_count"], r["sgpr_count"], r["vgpr_spill_count"], r["sgpr_spill_count"],
                                    r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"]))
        lines.append("no dynamically indexed per-thread array (the keys, words and ranks of a lane are arrays over the template's word count, every "
                     "loop over them fully unrolled); every ballot sits under control flow that is uniform per wavefront (the loop over agents, the "
                     "branch on a popcount of ballots)")
    if a.mutants:
        lines += ["", "%d. mutants: arithmetic-only changes of k_graph_bits_nearest, each built apart from the shipped library, loaded in its place and run "
                  "ONCE against the front-end tests of tests/test_gpu_nearest.py (masks, hand-made, ignore, no-op, position)" % section]
        lines += Path(a.mutants).read_text().rstrip().splitlines()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if rc in (0, 1) else rc


if __name__ == "__main__":
    sys.exit(main())
