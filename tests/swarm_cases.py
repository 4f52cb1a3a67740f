"""Shared by tests/test_swarm_cases.py (no GPU) and tests/test_gpu_swarm.py: teams of more than 64 agents for the distributed
path -- one scenario generator, the cases, and the CPU side of the checks (the oracle's distributed solves, computed once per
case and scenario and shared).  Nothing here touches the GPU.

A scenario: agents on a square lattice of spacing 3.0 with side ceil(sqrt(k)), agent a at (3 (a % side), 3 (a // side)) -- far
beyond the graph's threshold 2 * 0.5 of one another -- and then, so that neighbourhoods span the words of a multi-word mask:
  partners           agent 64 + q sits `offset` to the right of agent q, for q < min(6, k - 64): every such pair shares ONE
                     neighbourhood with a member on either side of bit 64 (quirk Q11 merges the two sub-problems)
  asymmetric triple  for k > 66, agent 63 sits `offset` above agent 10 and agent k - 1 `offset` below it: at offset 0.6 the two are
                     1.2 apart, so agent 10's neighbourhood {10, 63, k - 1} is a triple neither member shares
Velocities and headings are zero, the goal is the start plus a uniform(-0.4, 0.4) planar move.  Q = diag(1, 1, 0, ...), R = I,
Qf = 1000 I, radius 0.5 (the cost's and the graph's), dt 0.1.
"""
import functools
import math

import numpy as np

from oracle import oracle as orc

SPACING, RADIUS, DT = 3.0, 0.5, 0.1
OFFSET_SOLVE, OFFSET_ROLLOUT = 0.6, 0.4      # 0.6: neighbours (< 1.0) outside the cost's radius; 0.4: inside it
S = 3
JITTER = 0.15
N_LQR_ITER = 30
G_ACC = 9.80665
MODEL_DIMS = {0: (4, 2), 3: (4, 2), 4: (6, 3), 7: (12, 4)}


class Case:
    def __init__(self, k, model, T, n_d=2, solve=True):
        self.k, self.model, self.T, self.n_d, self.solve = k, model, T, n_d, solve
        self.ns, self.nc = MODEL_DIMS[model]
        self.n_words = (k + 63) // 64

    @property
    def id(self):
        return f"k{self.k}-m{self.model}-T{self.T}"


CASES = [
    Case(65, 0, 10),                          # DoubleIntDynamics4D: one pair across the boundary
    Case(70, 3, 10),                          # UnicycleDynamics4D: agent k - 1 = 69 is the triple's, partner 64 + 5 gives way
    Case(130, 0, 8),                          # three words
    Case(66, 4, 8, n_d=3, solve=False),       # QuadcopterDynamics6D, n_dims = 3 everywhere: quirk Q5 (planar distances all the same)
    Case(256, 0, 4, solve=False),             # the largest team: front end and rollout only
]
SOLVE_CASES = [c for c in CASES if c.solve]


def positions(k, offset):
    side = math.ceil(math.sqrt(k))
    p = np.array([[SPACING * (a % side), SPACING * (a // side)] for a in range(k)], dtype=np.float64)
    for q in range(min(6, k - 64)):
        p[64 + q] = p[q] + [offset, 0.0]
    if k > 66:
        p[63] = p[10] + [0.0, offset]
        p[k - 1] = p[10] - [0.0, offset]
    return p


def scenario(case, offset):
    """x0 (S, n_x) -- scenario 0 as generated, the others with N(0, 0.15) planar jitter --, xf (n_x,), U0 (T, n_u)."""
    k, ns, nc = case.k, case.ns, case.nc
    rng = np.random.default_rng(7000 + k)
    x0 = np.zeros((k, ns)); x0[:, :2] = positions(k, offset)
    xf = x0.copy(); xf[:, :2] += rng.uniform(-0.4, 0.4, size=(k, 2))
    x0s = np.tile(x0[None], (S, 1, 1))
    x0s[1:, :, :2] += rng.normal(scale=JITTER, size=(S - 1, k, 2))
    U0 = np.zeros((case.T, k * nc))
    if case.model == 4:
        U0[:, 0::nc] = G_ACC              # gravity compensation: hover
    return x0s.reshape(S, k * ns), xf.reshape(-1), U0


def weights(case):
    ns, nc = case.ns, case.nc
    Q = np.zeros((ns, ns)); Q[0, 0] = Q[1, 1] = 1.0
    return Q, np.eye(nc), 1000.0 * np.eye(ns)


def oracle_problem(case, xf):
    Q, R, Qf = weights(case)
    return orc.Problem([case.model] * case.k, [case.n_d] * case.k, xf, Q, R, Qf, RADIUS, DT, case.T)


def mask_of(members):
    return sum(1 << int(j) for j in members)


def words_to_masks(bits):
    """(..., n_words) int64 words -> object array (...) of Python ints: word w, bit b = agent 64 w + b."""
    w = np.ascontiguousarray(bits).view(np.uint64)
    out = np.zeros(w.shape[:-1], dtype=object)
    for i in range(w.shape[-1]):
        out = out + (w[..., i].astype(object) << (64 * i))
    return out


@functools.lru_cache(maxsize=None)
def oracle_solve(case_index, s, du=0.0):
    """oracle.solve_distributed of scenario s of CASES[case_index] from (x0, U0 + du): X_dec, U_dec, J_full, graph."""
    case = CASES[case_index]
    x0s, xf, U0 = scenario(case, OFFSET_SOLVE)
    return orc.solve_distributed(oracle_problem(case, xf), x0s[s][None], U0 + du, RADIUS, n_lqr_iter=N_LQR_ITER)


def cluster_table(graph):
    """{cluster size: agents with a neighbourhood of that size}, members whose neighbourhood spans bit 64, distinct neighbourhoods"""
    sizes = {}
    for v in graph.values():
        sizes[len(v)] = sizes.get(len(v), 0) + 1
    spanning = sum(1 for v in graph.values() if len({j // 64 for j in v}) > 1)
    return sizes, spanning, len({tuple(v) for v in graph.values()})
