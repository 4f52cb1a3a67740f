"""Shared by tests/test_gpu_policy_dec.py, tests/test_policy_dec_host.py and scripts/policy_dec_sensitivity.py: the cases of
the neighbourhood-sparse closed-loop rollout (dpilqr_policy_rollout_dec), their masks and the CPU side of the check.  Nothing
here touches the GPU.

A policy for the kernel test is the oracle's dense K of tests/policy_cases.py with the blocks outside the agents' masks zeroed:
the reference is then policy_cases.ref_sample fed that masked K, and the bound policy_cases.bound_of of the same +-PERTURB
sensitivity.  Masks per item: item 0 every agent sees everyone, item 1 every agent is alone, item 2 seeded random masks,
asymmetric and of mixed sizes, the largest smaller than k (so that the items 1 and 2 alone have a true kc_max below k).

sigma and radius are those of the same cases in tests/policy_cases.py, kept: the masked references were run on the CPU with
those values first, and they meet the conditions of tests/test_policy_dec_host.py unchanged (figures:
profiles/policy_dec_sensitivity.txt, written by scripts/policy_dec_sensitivity.py)."""
import numpy as np

from tests import linesearch_cases as lc
from tests import policy_cases as pc

T, B = pc.T, pc.B

CASES = [
    pc.Case("dec-dint4_uni4-k5-S53", [0, 3, 0, 3, 3], 53, 0.3, 0.6, weights="per_item", seed=2),
    pc.Case("dec-quad6-k10-S26", [4] * 10, 26, 0.6, 0.15, seed=4),
    pc.Case("dec-bike5-k3-S5", [lc.BIKE] * 3, 5, 0.3, lc.WIDE_RADIUS, seed=3),
    pc.Case("dec-quad6_human6-k3-S6", [4, 5, 4], 6, 0.3, 1.5, n_dims=[3, 2, 3], weights="per_agent", seed=5),
    pc.Case("dec-dint4-k1-S9", [0], 9, 0.3, 0.6, seed=7),
]
IDS = [c.id for c in CASES]


def popcount(m):
    return bin(int(m)).count("1")


def members(mask, k):
    return [j for j in range(k) if (int(mask) >> j) & 1]


def make_masks(case):
    """(B, k) uint64: item 0 full, item 1 alone, item 2 seeded random -- asymmetric, at least two sizes, none of them k."""
    k = case.k
    full = (1 << k) - 1
    masks = np.zeros((B, k), dtype=np.uint64)
    masks[0] = full
    masks[1] = [1 << a for a in range(k)]
    if k == 1:
        masks[2] = 1
        return masks
    rng = np.random.default_rng(7700 + case.seed)
    while True:
        row = [(1 << a) | sum(1 << j for j in range(k) if j != a and rng.random() < 0.5) for a in range(k)]
        sizes = {popcount(m) for m in row}
        asym = any((row[a] >> j) & 1 and not (row[j] >> a) & 1 for a in range(k) for j in range(k))
        if asym and max(sizes) < k and (len(sizes) >= 2 or k == 2) and max(sizes) >= 2:
            masks[2] = row
            return masks


def mask_gains(K, masks, ns, nc):
    """K (B, T, n_u, n_x) with the blocks (agent a's rows, agent j's columns) zeroed where bit j of masks[b][a] is clear."""
    Bn, k = masks.shape
    Km = np.array(K, dtype=np.float64, copy=True)
    for b in range(Bn):
        for a in range(k):
            for j in range(k):
                if not (int(masks[b, a]) >> j) & 1:
                    Km[b, :, a * nc:(a + 1) * nc, j * ns:(j + 1) * ns] = 0.0
    return Km


def compact_gains(K, masks, ns, nc, kc_max, fill=np.nan):
    """Kc (B, T, k, n_c, kc_max * n_s): agent a's rows of K, the columns its members in ascending order, the rest `fill`."""
    Bn, k = masks.shape
    Tn = K.shape[1]
    Kc = np.full((Bn, Tn, k, nc, kc_max * ns), fill, dtype=np.float64)
    for b in range(Bn):
        for a in range(k):
            for p, j in enumerate(members(masks[b, a], k)):
                Kc[b, :, a, :, p * ns:(p + 1) * ns] = K[b, :, a * nc:(a + 1) * nc, j * ns:(j + 1) * ns]
    return Kc


class DecCaseRef(pc.CaseRef):
    """policy_cases.CaseRef with the masked gains in place of the dense ones: the same variants, limits, sensitivities and
    conditions, all computed by the inherited methods from self.K."""

    def __init__(self, case):
        self.case, self.batch = case, pc.make_batch(case)
        b = self.batch
        self.masks = make_masks(case)
        self.X, self.K_dense = pc.nominal_and_gains(b)
        self.K = mask_gains(self.K_dense, self.masks, case.ns, case.nc)
        self.U = b["U0"]
        self.problems = [pc.item_problem(b, i) for i in range(B)]
        self.ref, self.spread = {}, {}
        self._run("plain")
        allU = np.stack([[self.ref["plain"][i][s]["U"] for s in range(case.S)] for i in range(B)])
        flat = allU.reshape(-1, allU.shape[-1])
        self.u_lim = np.stack([np.quantile(flat, pc.QUANTILES[0], axis=0), np.quantile(flat, pc.QUANTILES[1], axis=0)])
        self._run("W"); self._run("u_lim")
        self.J_nom = np.array([pc.ref_sample(self.problems[i], b, i, self.X[i], self.U[i], self.K[i], self.X[i][0])["J"] for i in range(B)])

    def true_kc_max(self, items):
        return max(popcount(m) for i in items for m in self.masks[i])


_REFS = {}


def case_ref(case):
    """Computed once per case and shared (never modified) by the tests that need it."""
    if case.id not in _REFS:
        _REFS[case.id] = DecCaseRef(case)
    return _REFS[case.id]
