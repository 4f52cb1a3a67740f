"""Shared by tests/test_gpu_policy_dec_team.py, tests/test_policy_dec_team_host.py and scripts/policy_dec_team_checks.py: the cases
of the team closed-loop rollout (dpilqr_policy_rollout_dec_team, csrc/policy_dec_team.hpp) and the CPU side of their check.
Nothing here touches the GPU.

Everything is tests/policy_cases.py's and tests/policy_dec_cases.py's, imported: Case, make_batch, make_masks, mask_gains,
compact_gains, DecCaseRef (the reference is policy_cases.ref_sample fed the dense oracle gains with the off-mask blocks
zeroed), the per-sample bound bound_of(spread) = max(1e-9, 100 spread) and the cap MAX_UNCHECKED.  The one thing of its own is
a vectorised `separation`: policy_cases.separation walks the k (k - 1) / 2 pairs in Python, 2016 of them at k = 64, once per
step of every reference and sensitivity run -- the k = 64 reference took 18 s that way.  TeamCaseRef runs the same samples
with the vectorised one (the same distances; the minimum does not depend on the order), and tests/test_policy_dec_team_host.py
holds it equal to policy_cases.separation on a state of every case.

The shapes are the smallest at which THIS kernel can go wrong (a thread per (sample, agent), floor(256 / k) samples per
workgroup, one 64-bit mask word); sigma and radius were set on the CPU reference alone so that every case meets the conditions
of tests/test_policy_dec_host.py::test_case_conditions:
  team-dint4_uni4-k21-S13  the first k past policy_rollout_dec's limit; 12 samples per workgroup, so the second workgroup holds
                           one; samples straddle wavefronts; per-item weights
  team-car3-k21-S3         the three-state family, n_x = 63
  team-quad6-k21-S13       the six-state family, n_dims = 3
  team-quad12-k21-S2       the twelve-state step, n_x = 252: the register peak
  team-dint4-k33-S8        odd k: 7 samples per workgroup, 25 idle lanes
  team-dint4-k64-S5        mask bit 63 (the full mask is -1 as int64), even k (the offset k / 2), 4 samples per workgroup,
                           n_x = 256: beyond any centralised kernel
Settings that did NOT meet the conditions: 33 quadcopters at any of six (sigma, radius) pairs (a quarter of the samples draw no
bound, or fewer than half move); quadcopter / human mixes at k = 21 and k = 33 (a third or more of the samples draw no bound).
Mixed n_dims is therefore covered by the cross-check against policy_rollout_dec on dec-quad6_human6-k3-S6 instead."""
import numpy as np

from tests import policy_cases as pc
from tests import policy_dec_cases as dc

T, B = pc.T, pc.B

CASES = [
    pc.Case("team-dint4_uni4-k21-S13", [0, 3] * 10 + [0], 13, 0.3, 0.3, weights="per_item", seed=21),
    pc.Case("team-car3-k21-S3", [2] * 21, 3, 0.2, 0.15, seed=22),
    pc.Case("team-quad6-k21-S13", [4] * 21, 13, 0.6, 0.06, seed=62),
    pc.Case("team-quad12-k21-S2", [7] * 21, 2, 0.05, 0.6, seed=25),
    pc.Case("team-dint4-k33-S8", [0] * 33, 8, 0.3, 0.3, seed=53),
    pc.Case("team-dint4-k64-S5", [0] * 64, 5, 0.3, 0.3, seed=24),
]
IDS = [c.id for c in CASES]
# the cases of tests/policy_dec_cases.py both kernels serve that the cross-check runs: mixed models, and mixed n_dims
CROSS = [c for c in dc.CASES if c.id in ("dec-dint4_uni4-k5-S53", "dec-quad6_human6-k3-S6")]


def separation(x, k, ns, n_dims):
    """policy_cases.separation, all pairs at once."""
    if k == 1:
        return np.inf
    xs = np.asarray(x).reshape(k, ns)
    nd = np.asarray(n_dims)
    i, j = np.triu_indices(k, 1)
    pair_nd = np.full(i.shape, 2) if len(set(n_dims)) == 1 else np.minimum(nd[i], nd[j])
    width = int(pair_nd.max())
    diff = (xs[i, :width] - xs[j, :width]) * (np.arange(width)[None, :] < pair_nd[:, None])
    return float(np.min(np.sqrt(np.sum(diff ** 2, axis=1))))


def ref_sample(p, batch, i, X, U, K, x0, W=None, u_lim=None):
    """policy_cases.ref_sample, statement for statement, with the vectorised separation."""
    step, cost = pc._step_cost(p)
    k, n_dims = len(batch["models"]), batch["n_dims"]
    ns = X.shape[1] // k
    Tn = U.shape[0]
    Xs = np.zeros((Tn + 1, X.shape[1])); Us = np.zeros_like(U)
    Xs[0] = x0
    J, sep = 0.0, separation(Xs[0], k, ns, n_dims)
    for t in range(Tn):
        u = U[t] + K[t] @ (Xs[t] - X[t])
        if u_lim is not None:
            u = np.where(u < u_lim[0], u_lim[0], np.where(u > u_lim[1], u_lim[1], u))
        Us[t] = u
        J += cost(Xs[t], u)
        Xs[t + 1] = step(Xs[t], u)
        if W is not None:
            Xs[t + 1] += W[t]
        sep = min(sep, separation(Xs[t + 1], k, ns, n_dims))
    J += cost(Xs[-1], np.zeros(U.shape[1]), terminal=True)
    e = (Xs[-1] - batch["xf"][i]).reshape(k, ns)
    goal = np.array([np.sqrt(np.sum(e[a, :n_dims[a]] ** 2)) for a in range(k)])
    return dict(X=Xs, U=Us, J=J, min_sep=sep, goal_dist=goal)


class TeamCaseRef(dc.DecCaseRef):
    """policy_dec_cases.DecCaseRef -- masks, masked gains, variants, limits, sensitivities, conditions -- whose samples are run
    by this module's ref_sample."""

    def _run(self, variant):
        b, S = self.batch, self.case.S
        W, lim = self.args(variant)
        self.ref[variant] = [[None] * S for _ in range(B)]
        self.spread[variant] = np.zeros((B, S))
        for i in range(B):
            p = self.problems[i]
            for s in range(S):
                Ws = None if W is None else W[i, s]
                r = ref_sample(p, b, i, self.X[i], self.U[i], self.K[i], b["x0s"][i, s], Ws, lim)
                self.ref[variant][i][s] = r
                sp = 0.0
                for sg in (1.0, -1.0):
                    e = sg * pc.lc.PERTURB
                    q = ref_sample(p, b, i, self.X[i] * (1 + e), self.U[i] * (1 - e), self.K[i] * (1 - e), b["x0s"][i, s] * (1 + e), Ws, lim)
                    sp = max(sp, pc.difference(q, r))
                self.spread[variant][i, s] = sp


_REFS = {}


def case_ref(case):
    """Computed once per case and shared (never modified) by the tests that need it."""
    if case.id not in _REFS:
        _REFS[case.id] = TeamCaseRef(case)
    return _REFS[case.id]
