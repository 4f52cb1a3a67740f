#!/usr/bin/env python
"""Write tests/golden/g12_separated_setup.npz: random scenarios with a minimum separation (random_setup's random=False branch), from
the REAL reference's util.random_setup and NumPy's legacy global stream.

    python scripts/make_golden_separated.py <checkout of the reference>      (or DPILQR_REFERENCE=<checkout>)

The reference's dpilqr/util.py is imported by path.  Every record is

    np.random.seed(seed)
    x0, xf = util.random_setup(k, n_s, is_rotation=False, rel_dist=rel_dist, var=var, n_d=n_d, random=False, energy=energy)

for the shapes of CASES, each with energy 0 (None) and 5 k and the seeds SEEDS.  The file holds arrays only, one entry per record:
  k, n_s, n_d, seed, rel_dist, var, energy     the arguments (energy 0.0: none)
  digest[record, x0 | xf]                      two 64-bit words per array, the digest of scripts/make_golden_wide.py
  rounds[record, starts | goals]               util.separate_locs' round counts on the raw draws (this package's NumPy statement
                                               of the loop -- the reference does not report them)
  x0_<record>, xf_<record>                     the arrays in full where k <= 8
The script asserts what makes the fixture a test of the loop and not only of its first round: util.separate_locs chained as
random_setup chains it reproduces every record bit for bit, every set separates within 64 rounds, every shape of three agents or
more has a set with a round in which only some points move (two points are always flagged together), and some set needs three
rounds or more.
tests/separated_setup_check.cpp prints the same digests from csrc/separated_setup.hpp on the host; the GPU tests compare the device's.
"""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "g12_separated_setup.npz"
# (k, n_d, n_s, rel_dist, var)
CASES = ((2, 2, 4, 2.0, 1.0), (3, 2, 4, 3.0, 1.5), (3, 3, 6, 3.0, 1.5), (5, 2, 4, 5.0, 2.5), (7, 2, 4, 2.0, 3.5), (24, 2, 4, 24.0, 12.0),
         (64, 2, 4, 64.0, 32.0), (65, 2, 4, 65.0, 32.5), (129, 2, 4, 129.0, 64.5), (130, 3, 6, 130.0, 65.0), (256, 2, 4, 256.0, 128.0),
         (256, 2, 4, 8.0, 128.0), (130, 1, 4, 24.0, 65.0))      # the last: one coordinate, whose mean NumPy adds pairwise
SEEDS = (0, 1, 2)
FULL_BELOW = 8
MAX_ROUNDS = 64


def energies_of(k):
    return (None, 5.0 * k)


def digest(a):
    """(sum of the bit patterns, sum of pattern * (2 i + 1)), both modulo 2^64."""
    v = np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)
    w = np.arange(v.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return np.array([v.sum(dtype=np.uint64), (v * w).sum(dtype=np.uint64)], dtype=np.uint64)


def replay(x, rel_dist):
    """separate_locs round by round: (the separated set, its rounds, whether some round moved some but not all points)."""
    from dpilqr_amd.util import separate_locs
    partial, rounds = False, 0
    while True:
        y, r = separate_locs(x, rel_dist, max_iter=1)
        rounds += 1
        if r == 1:
            break
        moved = int((y != x).any(axis=1).sum())
        partial = partial or 0 < moved < len(x)
        x = y
    return y, rounds, partial


def mine(k, n_s, n_d, seed, rel_dist, var, energy):
    """The record from this package's statement of the loop: the raw draws, separate_locs on either set, normalize_energy."""
    from dpilqr_amd.util import normalize_energy, separate_locs
    np.random.seed(seed)
    sets, rounds, partial = [], [], False
    for _ in range(2):
        raw = var * np.random.uniform(-1, 1, (k, n_d))
        x, r = separate_locs(raw, rel_dist)
        _, r_replayed, p = replay(raw, rel_dist)
        assert r == r_replayed
        sets.append(x); rounds.append(r); partial = partial or p
    pad = np.zeros((k, n_s - n_d))
    x0, xf = (np.c_[s, pad].reshape(-1, 1) for s in sets)
    if energy:
        x0, xf = (normalize_energy(x, [n_s] * k, energy, n_d) for x in (x0, xf))
    return x0, xf, rounds, partial


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DPILQR_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref_dpilqr_util", Path(ref) / "dpilqr" / "util.py")
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    cols = {name: [] for name in ("k", "n_s", "n_d", "seed", "rel_dist", "var", "energy")}
    out, dg, rounds = {}, [], []
    for k, n_d, n_s, rel_dist, var in CASES:
        shape_partial = False
        for energy in energies_of(k):
            for seed in SEEDS:
                np.random.seed(seed)
                x0, xf = util.random_setup(k, n_s, is_rotation=False, rel_dist=rel_dist, var=var, n_d=n_d, random=False, energy=energy)
                m0, mf, r, partial = mine(k, n_s, n_d, seed, rel_dist, var, energy)
                assert np.array_equal(x0.view(np.uint64), m0.view(np.uint64)) and np.array_equal(xf.view(np.uint64), mf.view(np.uint64)), \
                    f"separate_locs differs from the reference: k={k} n_d={n_d} seed={seed} energy={energy}"
                assert all(1 <= v <= MAX_ROUNDS for v in r), (k, seed, r)
                shape_partial = shape_partial or partial
                rec = len(dg)
                for name, v in zip(cols, (k, n_s, n_d, seed, rel_dist, var, energy or 0.0)):
                    cols[name].append(v)
                dg.append([digest(x0), digest(xf)]); rounds.append(r)
                if k <= FULL_BELOW:
                    out[f"x0_{rec}"] = x0.ravel().copy(); out[f"xf_{rec}"] = xf.ravel().copy()
        # (two points are always flagged together -- the distance is symmetric -- so a pair has no partial round)
        assert shape_partial or k == 2, f"no set of k={k}, n_d={n_d}, rel_dist={rel_dist} has a round that moves only some points"
    rounds = np.array(rounds, dtype=np.int32)
    assert rounds.max() >= 3, "no set needs three rounds"
    for name in ("k", "n_s", "n_d"):
        out[name] = np.array(cols[name], dtype=np.int32)
    out["seed"] = np.array(cols["seed"], dtype=np.int64)
    for name in ("rel_dist", "var", "energy"):
        out[name] = np.array(cols[name], dtype=np.float64)
    out.update(digest=np.array(dg, dtype=np.uint64), rounds=rounds, numpy_version=np.array(np.__version__))
    np.savez(OUT, **out)
    print(f"{OUT.relative_to(ROOT)}: {OUT.stat().st_size} bytes, {len(dg)} records, rounds {rounds.min()} .. {rounds.max()}")


if __name__ == "__main__":
    main()
