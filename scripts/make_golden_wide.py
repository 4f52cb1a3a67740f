#!/usr/bin/env python
"""Write tests/golden/g11_trial_inputs_wide.npz: what a trial of the Monte-Carlo study draws for teams of more than 64 agents,
from the REAL reference's util.random_setup and NumPy's legacy global stream.

    python scripts/make_golden_wide.py <checkout of the reference>      (or DPILQR_REFERENCE=<checkout>)

The reference's dpilqr/util.py is imported by path and runs the sequence include/dpilqr_swarm_study.h defines:

    np.random.seed(seed)
    x0, xf = util.random_setup(k, n_s, is_rotation=False, var=k / 2, n_d=n_d, random=True, energy=energy)
    U_a = np.random.rand(N, n_u) * 0.01;  U_b = np.random.rand(N, n_u) * 0.01

Cases: (k, n_s, n_d) of CASES, seeds 0 .. 4, energy 10 k / 5 and None, two warm starts of N = 3 steps, n_u = k n_c (n_c = 2 for the
four-state models, 3 for the six-state one).  The four largest cases draw 770 KB of doubles, so the file keeps
  digest[case, energy, seed, array]   two 64-bit words per output array (x0, xf, U_a, U_b): the wrapping sum of the array's bit
                                      patterns and the wrapping sum of pattern * (2 index + 1) -- any changed bit changes both
  full_x0 / full_xf _<k>_<e>          the arrays of seed FULL_SEED themselves, position columns only, for both energies
and one small case in full (SMALL: k = 5, non-consecutive seeds, the largest seed 2^32 - 1).  Arrays and scalars only.
tests/trial_inputs_check.cpp prints the same digests from csrc/trial_inputs.hpp on the host; the GPU tests compare the device's.
"""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "g11_trial_inputs_wide.npz"
CASES = ((65, 4, 2), (129, 4, 2), (255, 6, 3), (256, 6, 3))
SEEDS = (0, 1, 2, 3, 4)
N = 3
WARM_SCALE = 0.01
FULL_SEED = 3
SMALL = dict(k=5, n_s=4, n_d=2, seeds=(7, 3, 4294967295, 100), energy=10.0)


def energies_of(k):
    return (10.0 * k / 5, None)


def digest(a):
    """(sum of the bit patterns, sum of pattern * (2 i + 1)), both modulo 2^64."""
    v = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
    w = np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([v.sum(dtype=np.uint64), (v * w).sum(dtype=np.uint64)], dtype=np.uint64)


def draw(util, k, n_s, n_d, seed, energy):
    n_u = k * (3 if n_s == 6 else 2)
    np.random.seed(seed)
    x0, xf = util.random_setup(k, n_s, is_rotation=False, var=k / 2, n_d=n_d, random=True, energy=energy)
    U_a = np.random.rand(N, n_u) * WARM_SCALE
    U_b = np.random.rand(N, n_u) * WARM_SCALE
    return x0.ravel(), xf.ravel(), U_a, U_b


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DPILQR_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref_dpilqr_util", Path(ref) / "dpilqr" / "util.py")
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    out = dict(cases=np.array(CASES, dtype=np.int32), seeds=np.array(SEEDS, dtype=np.int64), N=np.int32(N),
               warm_scale=np.float64(WARM_SCALE), full_seed=np.int64(FULL_SEED),
               energies=np.array([[e or 0.0 for e in energies_of(k)] for k, _, _ in CASES]), numpy_version=np.array(np.__version__))
    dg = np.zeros((len(CASES), 2, len(SEEDS), 4, 2), dtype=np.uint64)
    for ci, (k, n_s, n_d) in enumerate(CASES):
        for ei, energy in enumerate(energies_of(k)):
            for si, seed in enumerate(SEEDS):
                arrays = draw(util, k, n_s, n_d, seed, energy)
                for ai, a in enumerate(arrays):
                    dg[ci, ei, si, ai] = digest(a)
                if seed == FULL_SEED:
                    out[f"full_x0_{k}_{ei}"] = arrays[0].reshape(k, n_s)[:, :n_d].copy()
                    out[f"full_xf_{k}_{ei}"] = arrays[1].reshape(k, n_s)[:, :n_d].copy()
    out["digest"] = dg
    sm = [draw(util, SMALL["k"], SMALL["n_s"], SMALL["n_d"], seed, SMALL["energy"]) for seed in SMALL["seeds"]]
    out.update(small_case=np.array([SMALL["k"], SMALL["n_s"], SMALL["n_d"]], dtype=np.int32), small_seeds=np.array(SMALL["seeds"], dtype=np.int64),
               small_energy=np.float64(SMALL["energy"]), small_x0=np.stack([d[0] for d in sm]), small_xf=np.stack([d[1] for d in sm]),
               small_Ua=np.stack([d[2] for d in sm]), small_Ub=np.stack([d[3] for d in sm]))
    np.savez(OUT, **out)
    print(f"{OUT.relative_to(ROOT)}: {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
