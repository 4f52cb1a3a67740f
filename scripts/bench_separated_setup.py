#!/usr/bin/env python
"""Measure the separated scenarios on the device (profiles/separated_setup.txt).  Record only: nothing is gated on these figures.

dpilqr_setup_separate (include/dpilqr_separated_setup.h) on the raw draws of S scenarios of k double integrators, the study's
arguments rel_dist = k, var = k / 2, energy = 5 k (and rel_dist = 8 at k = 256): device events around the one launch, the buffers
allocated and refilled with the raw draws outside the timed span; median of 25 launches after a warm-up, the rounds the sets took
beside it.  Beside each figure:
  draw       dpilqr_trial_inputs alone (no warm start, the same energy) at the same S and k, timed the same way
  host loop  util.random_setup(random=False) per scenario on the host: wall clock over 64 scenarios, given per scenario and
             times S

    python scripts/bench_separated_setup.py [--out profiles/separated_setup.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REPS, HOST_SAMPLE = 25, 64
SHAPES = ((5, 5.0), (65, 65.0), (128, 128.0), (256, 256.0), (256, 8.0))      # (k, rel_dist)


def median_ms(before, launch, reps=REPS):
    """Median of `reps` event-timed calls of launch(), each after before() (untimed), following one warm-up."""
    import torch
    before(); launch(); torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); launch(); b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "separated_setup.txt"))
    args = ap.parse_args()
    import torch
    from dpilqr_amd import _lib, util
    from dpilqr_amd.device import empty, ptr, stream_handle
    _lib.require_gpu()
    L = _lib.load()
    lines = ["separated scenarios: scripts/bench_separated_setup.py on one MI355X", "",
             f"n_s = 4, n_d = 2, var = k / 2, energy = 5 k, seeds 0 .. S - 1; device columns: median of {REPS} event-timed launches after a warm-up [ms]",
             f"{'k':>4} {'rel_dist':>8} {'S':>5} {'rounds':>8} {'separate':>9} {'draw':>8} {'host/scn':>9} {'host loop':>10} {'host/device':>11}"]
    for k, rel_dist in SHAPES:
        var, energy, n = k / 2, 5.0 * k, HOST_SAMPLE
        t0 = time.perf_counter()
        for s in range(n):
            np.random.seed(s)
            util.random_setup(k, 4, is_rotation=False, rel_dist=rel_dist, var=var, n_d=2, random=False, energy=energy)
        host_each = (time.perf_counter() - t0) / n * 1e3
        for S in (1, 64, 1024):
            raw0, rawf = util.random_setup_batch((0, S), k, 4, var, energy=None, wide=True)
            x0, xf, counts = empty((S, 4 * k)), empty((S, 4 * k)), empty((S, 2), torch.int32)

            def refill():
                x0.copy_(raw0); xf.copy_(rawf)

            sep = median_ms(refill, lambda: _lib.check(L.dpilqr_setup_separate(S, k, 4, 2, rel_dist, energy, 256, ptr(x0), ptr(xf), ptr(counts),
                                                                                stream_handle())))
            draw = median_ms(lambda: None, lambda: _lib.check(L.dpilqr_trial_inputs(S, 0, None, k, 4, 2, var, energy, 0, 0, 0, 0.0, ptr(x0), ptr(xf),
                                                                                    None, None, stream_handle())))
            r = counts.cpu().numpy()
            assert (r > 0).all()
            lines.append(f"{k:>4} {rel_dist:>8g} {S:>5} {f'{r.min()}..{r.max()}':>8} {sep:>9.4f} {draw:>8.4f} {host_each:>9.3f} {host_each * S:>10.1f} "
                         f"{host_each * S / (sep + draw):>11.0f}")
    lines += ["", f"host/scn: wall clock of util.random_setup(random=False) per scenario over seeds 0 .. {HOST_SAMPLE - 1}, one pass; host loop = host/scn x S",
              "(extrapolated above 64 scenarios); host/device = host loop / (separate + draw).  The upload a host loop also needs is not in it.",
              "Not measured: counters (none collected), other models, n_d = 3, energies, the Python layer's allocation and the read-back of the counts."]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
