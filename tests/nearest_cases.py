"""Shared by tests/test_nearest_cases.py (no GPU), tests/test_nearest_host.py, tests/test_gpu_nearest.py and the scripts under
scripts/ that record them: neighbourhoods capped at their m nearest agents (include/dpilqr_nearest.h).  One scenario generator, the
cases, three hand-made scenarios, a brute-force reference of the definition that shares no code with
dpilqr_amd.distributed.nearest_neighbourhoods, and the oracle's capped distributed solve.  Nothing here touches the GPU.

A scenario: k agents on a square lattice of side ceil(sqrt(k)) and spacing 0.9 with a planar jitter of uniform(-0.05, 0.05); the
goal is the start plus a planar uniform(-0.15, 0.15); X is the straight line from start to goal over 11 rows (all of them sampled),
its first row alone the N = 1 form.  The proximity cost's radius is 0.5 and the GRAPH's radius 4.0, an argument of its own: the
teams are near-cliques (uncapped neighbourhood sizes 6, 61-64, 58-65, 70-130 and 70-229 for k = 6, 64, 65, 130 and 256) while no
two agents ever come inside the cost's radius (the smallest separation over the rows is above 0.59), so the solves stay benign.
Scenario 0 is as generated; scenarios 1 .. S - 1 move every start and goal by a further planar uniform(-0.03, 0.03).
Q = diag(1, 1, 0, 0), R = I, Qf = 1000 I, dt 0.1, double integrators (tests/swarm_cases.py).
"""
import functools
import math

import numpy as np

from oracle import oracle as orc
from tests import swarm_cases as sw

SPACING, JITTER, GOAL_MOVE, EXTRA_JITTER = 0.9, 0.05, 0.15, 0.03
COST_RADIUS, GRAPH_RADIUS, DT = 0.5, 4.0, 0.1
ROWS = 11
S = 3
NS, NC = 4, 2
N_LQR_ITER = sw.N_LQR_ITER
MARGIN = 1e-9      # the smallest |key - thr| and key gap at the cut a case may have: a condition on the cases, not a tolerance


class Case:
    """k agents, the cap m; T and S_solve where the case is also solved (tests/test_gpu_nearest.py), policy where it is run in
    closed loop ('wide' or True)."""

    def __init__(self, k, m, T=None, S_solve=None, policy=None):
        self.k, self.m, self.T, self.S_solve, self.policy = k, m, T, S_solve, policy
        self.ns, self.nc, self.model, self.n_d = NS, NC, 0, 2
        self.n_words = (k + 63) // 64

    @property
    def id(self):
        return f"k{self.k}-m{self.m}"


CASES = [
    Case(6, 1), Case(6, 3, T=10, policy=True),             # the narrow route, policy=True
    Case(64, 4, T=8, S_solve=2, policy="wide"), Case(64, 8),      # one full word; uncapped, n_x = 256 is beyond the solver
    Case(65, 4, T=10, S_solve=3, policy="wide"),           # two words
    Case(130, 5, T=8, S_solve=2),                          # three words; uncapped, this team is refused
    Case(256, 2), Case(256, 64),                           # the front end only
]
SOLVE_CASES = [c for c in CASES if c.S_solve]
POLICY_CASES = [c for c in CASES if c.policy]
IDS = [c.id for c in CASES]


@functools.lru_cache(maxsize=None)
def scenario(k):
    """x0 (S, k * 4), xf (S, k * 4), X (S, ROWS, k * 4): the straight lines from start to goal."""
    side = math.ceil(math.sqrt(k))
    p = np.array([[SPACING * (a % side), SPACING * (a // side)] for a in range(k)], dtype=np.float64)
    p = p + np.random.default_rng(9000 + k).uniform(-JITTER, JITTER, size=(k, 2))
    g = p + np.random.default_rng(1 + k).uniform(-GOAL_MOVE, GOAL_MOVE, size=(k, 2))
    extra = np.random.default_rng(9500 + k).uniform(-EXTRA_JITTER, EXTRA_JITTER, size=(S - 1, 2, k, 2))
    x0, xf = np.zeros((S, k, NS)), np.zeros((S, k, NS))
    x0[:, :, :2], xf[:, :, :2] = p, g
    x0[1:, :, :2] += extra[:, 0]; xf[1:, :, :2] += extra[:, 1]
    x0, xf = x0.reshape(S, -1), xf.reshape(S, -1)
    X = x0[:, None, :] + np.linspace(0.0, 1.0, ROWS)[None, :, None] * (xf - x0)[:, None, :]
    for a in (x0, xf, X):
        a.setflags(write=False)
    return x0, xf, X


def keys_of(X, k, ns):
    """key (k, k): min over the sampled rows of sqrt(dx*dx + dy*dy), row after row with `d < key` (a NaN never wins); +inf on
    the diagonal."""
    X = np.atleast_2d(X)
    N = X.shape[0]
    P = X[0:N + 1:max(N // 10, 1)].reshape(-1, k, ns)
    key = np.full((k, k), np.inf)
    for r in range(P.shape[0]):
        dx, dy = P[r, :, None, 0] - P[r, None, :, 0], P[r, :, None, 1] - P[r, None, :, 1]
        with np.errstate(invalid="ignore"):
            d = np.sqrt(dx * dx + dy * dy)
            key = np.where(d < key, d, key)
    np.fill_diagonal(key, np.inf)
    return key


def reference(X, k, ns, radius, m):
    """The definition by brute force for one scenario: per agent, every other agent with key < 2 radius as a (key, j) tuple,
    sorted; more than m members: the first m - 1 are kept.  Returns graph {i: sorted members}, dropped (k,), uncapped sizes (k,),
    the smallest gap between the last kept and the first dropped key (inf where no cap bites), the smallest |key - thr|."""
    key = keys_of(X, k, ns)
    thr = 2 * radius
    graph, dropped, sizes, gap = {}, np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32), np.inf
    for i in range(k):
        cand = sorted((float(key[i, j]), j) for j in range(k) if j != i and key[i, j] < thr)
        sizes[i] = len(cand) + 1
        if sizes[i] > m:
            if m > 1:
                gap = min(gap, cand[m - 1][0] - cand[m - 2][0])
            cand = cand[:m - 1]
        graph[i] = sorted([i] + [j for _, j in cand])
        dropped[i] = sizes[i] - len(graph[i])
    off = key[np.isfinite(key)]
    return graph, dropped, sizes, gap, float(np.min(np.abs(off - thr))) if off.size else np.inf


def masks_of(graph, k):
    return [sw.mask_of(graph[i]) for i in range(k)]


def derive(masks, ignore=None):
    """rep, size of one scenario's masks by the host definitions: the first agent with an identical mask (ignored agents: -1, 0
    and never a representative)."""
    k = len(masks)
    rep, size = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
    for i, m_ in enumerate(masks):
        if ignore is not None and ignore[i]:
            rep[i], size[i] = -1, 0
            continue
        rep[i] = next(j for j in range(i + 1) if masks[j] == m_ and not (ignore is not None and ignore[j]))
        size[i] = bin(m_).count("1")
    return rep, size


# ---- hand-made scenarios: dict(name, k, m, radius, X (N, k * 4)); every other agent sits far away on the line y = 50
def _hand(name, k, m, radius, P):
    """P (N, k, 2) planar positions -> the scenario"""
    X = np.zeros((P.shape[0], k, NS)); X[:, :, :2] = P
    return dict(name=name, k=k, m=m, radius=radius, X=X.reshape(P.shape[0], -1))


def _far(k):
    return np.array([[3.0 * (a + 1), 50.0] for a in range(k)])


def hand_scenarios():
    out = []
    # 1. exact ties: coordinates are multiples of 0.25, agent `c` at the origin with four neighbours at distance exactly 0.5 in
    # any arithmetic (0.25 + 0 under the root); m = 3 keeps the two LOWEST indices.  Once with the tied agents 1 .. 4, once with
    # them at 63 .. 66: the winners 63 and 64 sit on either side of the word boundary.
    for name, k, c, tied in (("ties-k6", 6, 0, (1, 2, 3, 4)), ("ties-k70", 70, 0, (63, 64, 65, 66)), ("ties-k70-rev", 70, 69, (66, 65, 64, 63))):
        P = _far(k)
        P[c] = (0.0, 0.0)
        for j, xy in zip(tied, ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5))):
            P[j] = xy
        out.append(_hand(name, k, 3, 0.6, P[None]))      # (threshold 1.2: the opposite agents, exactly 1.0 apart, are well inside)
    # 2. the smallest distance on a later sampled row decides the cut: agent 1 rests 0.6 from agent 0, agent 2 starts 0.9 away, passes
    # at 0.3 on row 7 and leaves again; m = 2: agent 0 keeps agent 2 (min over the rows), row 0 alone would keep agent 1
    k, N = 5, 11
    P = np.tile(_far(k)[None], (N, 1, 1))
    P[:, 0] = (0.0, 0.0); P[:, 1] = (0.6, 0.0)
    P[:, 2, 0] = 0.0; P[:, 2, 1] = [0.9, 0.85, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.45, 0.7, 0.95]
    out.append(_hand("later-row", k, 2, 0.5, P))
    # 3. the cap bites for some agents only: five agents bunched up (neighbourhoods of 5 > m = 3), a pair and a loner (kept as they are);
    # once with the bunch across the word boundary
    bunch = np.array([(0.0, 0.0), (0.31, 0.02), (-0.05, 0.37), (0.42, 0.45), (-0.33, -0.21)])
    for name, k, idx in (("partial-k9", 9, (0, 1, 2, 3, 4)), ("partial-k67", 67, (62, 63, 64, 65, 66))):
        P = _far(k)
        P[list(idx)] = bunch
        pair = [a for a in range(k) if a not in idx][:2]
        P[pair[1]] = P[pair[0]] + (0.0, 0.55)
        out.append(_hand(name, k, 3, 0.5, P[None]))
    return out


HAND = hand_scenarios()
HAND_IDS = [h["name"] for h in HAND]


# ---- the oracle's capped distributed solve
def oracle_problem(k, xf, T):
    Q = np.zeros((NS, NS)); Q[0, 0] = Q[1, 1] = 1.0
    return orc.Problem([0] * k, [2] * k, xf, Q, np.eye(NC), 1000.0 * np.eye(NS), COST_RADIUS, DT, T)


def oracle_capped_solve(prob, X, U, graph, n_lqr_iter=N_LQR_ITER, tol=1e-3):
    """oracle.solve_distributed with the graph given: one sub-problem per agent over graph[i], the agent's own columns kept."""
    X = np.atleast_2d(X); k, ns, nc, T = prob.k, prob.n_s, prob.n_c, U.shape[0]
    prob = prob.with_T(T)
    X_dec = np.zeros((T + 1, k * ns)); U_dec = np.zeros((T, k * nc))
    for i in range(k):
        idx = graph[i]
        r = prob.subproblem(idx).solve(np.concatenate([X[0, a * ns:(a + 1) * ns] for a in idx]),
                                       np.concatenate([U[:, a * nc:(a + 1) * nc] for a in idx], axis=1), n_lqr_iter, tol)
        pos = idx.index(i)
        X_dec[:, i * ns:(i + 1) * ns] = r["X"][:, pos * ns:(pos + 1) * ns]
        U_dec[:, i * nc:(i + 1) * nc] = r["U"][:, pos * nc:(pos + 1) * nc]
    return X_dec, U_dec, prob.rollout(X[0], U_dec)[1]


@functools.lru_cache(maxsize=None)
def oracle_solve(case_index, s, du=0.0):
    """The oracle's capped distributed solve of scenario s of CASES[case_index] from (its first row, U0 = du): X_dec, U_dec, J_full,
    graph, dropped."""
    case = CASES[case_index]
    x0, xf, _ = scenario(case.k)
    graph, dropped, _, _, _ = reference(x0[s][None], case.k, NS, GRAPH_RADIUS, case.m)
    U0 = np.zeros((case.T, case.k * NC)) + du
    return oracle_capped_solve(oracle_problem(case.k, xf[s], case.T), x0[s][None], U0, graph) + (graph, dropped)
