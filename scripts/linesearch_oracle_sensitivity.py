#!/usr/bin/env python3
"""The CPU-only measurement behind tests/test_gpu_linesearch.py: for every parametrised case the oracle alone (its own gains
at mu = 1 in place of the GPU's) runs the line search of every checked item, and the table says what the test may rely on --
the rounding sensitivity of the accepted candidate's pass (spread max / p99), the share of items that draw no bound
(spread > 1e-7), the share with a near tie, how the accepted indices are spread and how many searches fail.

    python scripts/linesearch_oracle_sensitivity.py                 # writes profiles/linesearch_oracle_sensitivity.txt
    python scripts/linesearch_oracle_sensitivity.py --gpu-log LOG   # appends the GPU-vs-oracle errors of a pytest -s log

The caps the test asserts (unchecked + tie <= 5 %, acc >= 1 on >= 10 % of the items) are checked here first: a case that
misses one is marked MISS and the exit status is 1."""
import argparse
import multiprocessing as mp
import os
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "profiles" / "linesearch_oracle_sensitivity.txt"


def measure(idx):
    from oracle import oracle as orc
    from tests import linesearch_cases as lc
    case = lc.all_cases()[idx]
    b = lc.make_batch(case)
    al = orc.alphas()
    spreads, accs, ties, unchecked = [], [], 0, 0
    for i in case.checked():
        p = lc.item_problem(b, i)
        X0, _ = p.rollout(b["x0"][i], b["U0"][i])
        K, d = p.backward_pass(X0, b["U0"][i], 1.0)
        ref = lc.ItemRef(p, b["x0"][i], b["U0"][i], K, d, al)
        spreads.append(ref.spread); accs.append(ref.acc)
        if ref.bound is None:
            unchecked += 1
        elif ref.near_tie(ref.bound):
            ties += 1
    n = len(accs)
    accs = np.array(accs); sp = np.array(spreads); fin = sp[np.isfinite(sp)]
    hist = [int((accs == a).sum()) for a in range(-1, 10)]
    excused = (unchecked + ties) / n
    later = float((accs >= 1).mean())
    ok = excused <= 0.05 and (later >= 0.10 or not case.later_candidates_expected())
    return (f"{case.id:34s} {n:4d}  {fin.max() if fin.size else float('nan'):9.2e} {np.percentile(fin, 99) if fin.size else float('nan'):9.2e}"
            f"  {100.0 * unchecked / n:5.1f} {100.0 * ties / n:5.1f}  {100.0 * later:5.1f}  {hist[0]:4d}  "
            + " ".join(f"{h:3d}" for h in hist[1:]) + ("" if ok else "   MISS") + ("" if case.later_candidates_expected() else "   (one linear agent: no floor)"), ok)


def append_gpu(log):
    """Lines `LS_RESULT <case> items=.. ties=.. unchecked=.. worst_err=.. its_bound=.. min_margin=..` of a pytest -s run."""
    rows = re.findall(r"LS_RESULT (\S+) (.*)", Path(log).read_text())
    if not rows:
        sys.exit(f"no LS_RESULT lines in {log}")
    text = OUT.read_text().split("\n# GPU vs oracle")[0].rstrip("\n")
    out = [text, "", "# GPU vs oracle (MI355X, pytest -m gpu tests/test_gpu_linesearch.py): per case the worst relative error of J_last, J, X, U over the",
           "# checked items, that item's bound, and the smallest bound / error ratio of the case (cases below 10 are marked)", ""]
    for cid, rest in rows:
        kv = dict(t.split("=") for t in rest.split())
        mark = "   WITHIN 10x" if float(kv["min_margin"]) < 10.0 else ""
        out.append(f"{cid:34s} items={kv['items']:>4s} ties={kv['ties']:>2s} unchecked={kv['unchecked']:>2s} worst_err={float(kv['worst_err']):9.2e} "
                   f"its_bound={float(kv['its_bound']):9.2e} min_margin={float(kv['min_margin']):9.3g}{mark}")
    OUT.write_text("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-log")
    ap.add_argument("--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    if a.gpu_log:
        return append_gpu(a.gpu_log)
    from oracle import oracle as orc
    from tests import linesearch_cases as lc
    orc.lib()      # built once, before the workers start
    n = len(lc.all_cases())
    with mp.Pool(a.jobs) as pool:
        res = pool.map(measure, range(n), chunksize=1)
    head = ["# scripts/linesearch_oracle_sensitivity.py: the oracle alone on the checked items of every case of tests/test_gpu_linesearch.py",
            "# (oracle gains at mu = 1).  spread: largest relative change of X, U, J of the last evaluated candidate's pass under 1e-15",
            "# relative perturbations of X0, K, d; unch %: spread > 1e-7 (no bound); tie %: a candidate within the item's bound of J0;",
            "# acc>=1 %: items whose first candidate is rejected; fail: all ten rejected; then the items per accepted index 0 .. 9.",
            f"# U0 noise per model: {lc.U0_NOISE}",
            f"# radius {lc.WIDE_RADIUS} instead of 0.6 for clusters of (model: up to k agents) {lc.WIDE_RADIUS_MODELS}; no acc>=1 floor for ONE agent of the",
            f"# linear models {lc.LINEAR_MODELS} (an exactly linear-quadratic problem): see tests/linesearch_cases.py", "",
            f"{'case':34s} {'n':>4s}  {'spr max':>9s} {'spr p99':>9s}  {'unch%':>5s} {'tie%':>5s}  {'acc>=1':>6s}  {'fail':>4s}  "
            + " ".join(f"{i:3d}" for i in range(10))]
    OUT.write_text("\n".join(head + [r[0] for r in res]) + "\n")
    print(OUT.read_text())
    return 0 if all(r[1] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
