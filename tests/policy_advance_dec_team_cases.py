"""Shared by tests/test_policy_advance_dec_team_host.py, tests/test_gpu_policy_advance_dec_team.py and
scripts/policy_advance_dec_team_checks.py: the team receding-horizon advance (dpilqr_policy_advance_dec_team,
csrc/policy_advance_dec_team.hpp) on the cases of tests/policy_dec_team_cases.py, which are imported and not changed.  Every
(item i, sample s) of a case becomes ONE scenario q = i * S + s whose plan is item i's (X, U_ff, Kc, masks), repeated, as
tests/policy_advance_cases.py does it for the smaller advances.  Nothing here touches the GPU.

The shapes are the smallest at which THIS kernel can go wrong (a thread per (item, agent), floor(256 / k) items per workgroup,
one 64-bit mask word): the first k past policy_advance_dec's limit (21: 12 items per workgroup, 39 scenarios, so the fourth
workgroup holds three), odd k with idle lanes (33), mask bit 63 and four items per workgroup with a last workgroup of three
(64, 15 scenarios), every family's step with the register peak at twelve states.

The CPU side is the prefix of the cases' own reference (policy_dec_team_cases.ref_sample): policy_advance_cases.prefix and
prefix_figures, statement for statement, with the team module's vectorised separation (2016 pairs per state at k = 64).  The
bound of a scenario is policy_cases.bound_of of the sample's own sensitivity.

The loop's problem is the placement of tests/test_gpu_policy_dec_team.py, restated: 24 double integrators (n_x = 96), two
scenarios with clusters of several sizes."""
import numpy as np

from tests import policy_advance_cases as ac
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc
from tests.golden_util import relerr

T, B = pc.T, pc.B
N_D, SPARE, HS = ac.N_D, ac.SPARE, ac.HS
CASES, IDS, CROSS = tc.CASES, tc.IDS, tc.CROSS
VARIANTS = ("plain", "W", "u_lim")


def repeated(case, ref, fill=np.nan):
    """Host arrays of the case's B * S scenarios: plans, compact gains (`fill` past every neighbourhood), masks, starts, and W as
    (scenarios, T, n_x)."""
    b, S = ref.batch, case.S
    rep = lambda a: np.repeat(np.asarray(a), S, axis=0)
    Kc = dc.compact_gains(ref.K, ref.masks, case.ns, case.nc, case.k, fill=fill)
    return dict(X=rep(ref.X), U=rep(ref.U), Kc=rep(Kc), masks=rep(ref.masks), x0=b["x0s"].reshape(B * S, -1).copy(),
                W=b["W"].reshape(B * S, T, -1).copy(), n=B * S)


def prefix(case, ref, variant, i, s, h):
    """policy_advance_cases.prefix with the vectorised separation: J of the first h steps (one addition per step), the smallest
    separation over the states 0 .. h, the distance left at state h over N_D coordinates."""
    r, b = ref.ref[variant][i][s], ref.batch
    _, cost = pc._step_cost(ref.problems[i])
    J = 0.0
    for t in range(h):
        J = J + cost(r["X"][t], r["U"][t])
    sep = min(tc.separation(r["X"][t], case.k, case.ns, case.n_dims) for t in range(h + 1))
    e = (r["X"][h] - b["xf"][i]).reshape(case.k, case.ns)[:, :N_D]
    return J, sep, np.sqrt(np.sum(e * e, axis=1))


def prefix_figures(case, ref, h):
    """policy_advance_cases.prefix_figures with the vectorised separation."""
    S = case.S
    Us = np.stack([[ref.ref["u_lim"][i][s]["U"][:h] for s in range(S)] for i in range(B)])
    clamped = float(np.mean((Us == ref.u_lim[0]) | (Us == ref.u_lim[1])))
    near = float(np.mean([[min(tc.separation(ref.ref["W"][i][s]["X"][t], case.k, case.ns, case.n_dims) for t in range(h + 1))
                           < ref.batch["radius"] for s in range(S)] for i in range(B)]))
    unchecked = {v: ref.unchecked_fraction(v) for v in VARIANTS}
    return dict(clamped=clamped, near=near, unchecked=unchecked)


def scenario_error(st, q, J, sep, left):
    """The largest relative error of scenario q's J_exec, min_sep and dist_left in the host state `st` against the prefix."""
    d = max(abs(st["J_exec"][q] - J) / max(abs(J), 1e-300), relerr(st["dist_left"][q], left))
    if np.isinf(sep) or np.isinf(st["min_sep"][q]):
        return d if st["min_sep"][q] == sep else np.inf
    return max(d, abs(st["min_sep"][q] - sep) / max(abs(sep), 1e-300))


# ---- the loop's problem: 24 double integrators, the placement of tests/test_gpu_policy_dec_team.py
K_AG, NS, NC, DT = 24, 4, 2, 0.1
RADIUS, PROX_RADIUS = 0.5, 0.5
Q, R, QF = np.diag([1.0, 1.0, 0.5, 0.5]), np.eye(NC), 100.0 * np.eye(NS)
S_LOOP, N_LOOP, H_LOOP, L_LOOP = 2, 12, 2, 4      # two scenarios, horizon 12, two steps a round, four steps: two rounds
SIZES = [[2, 3, 3, 3, 2, 4, 4, 4, 4, 2, 2] + [1] * 13, [6] * 6 + [2] * 6 + [1] * 12]


def placement():
    """Agents closer than 2 RADIUS = 1 are neighbours.  Scenario 0: a chain of five (0.8 apart: sizes 2, 3, 3, 3, 2), a square of
    four (0.5: 4 each), a pair (0.6) and thirteen loners on a grid far away.  Scenario 1: a cluster of six (a centre and a
    pentagon of radius 0.5 around it), three pairs and twelve loners."""
    far = lambda i: [10.0 + 4.0 * (i % 5), 10.0 + 4.0 * (i // 5)]
    s0 = [[0.8 * i, 0.0] for i in range(5)] + [[0.0, 5.0], [0.5, 5.0], [0.0, 5.5], [0.5, 5.5]] + [[5.0, 0.0], [5.6, 0.0]]
    s0 += [far(i) for i in range(K_AG - len(s0))]
    s1 = [[0.0, 3.0]] + [[0.5 * np.cos(2 * np.pi * i / 5), 3.0 + 0.5 * np.sin(2 * np.pi * i / 5)] for i in range(5)]
    s1 += [[6.0, 0.0], [6.7, 0.0], [0.0, 8.0], [0.0, 8.7], [8.0, 8.0], [8.5, 8.5]]
    s1 += [far(i) for i in range(K_AG - len(s1))]
    pos = np.array([s0, s1])
    rng = np.random.default_rng(2424)
    goal = pos + rng.uniform(0.6, 1.4, size=pos.shape) * rng.choice([-1.0, 1.0], size=pos.shape)
    states = lambda p: np.concatenate([p, np.zeros_like(p)], axis=2).reshape(S_LOOP, -1)
    return states(pos), states(goal)


def loop_problem(xf):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(DT) for _ in range(K_AG)])
    costs = [dp.ReferenceCost(xf[NS * i:NS * (i + 1)], Q, R, QF, i) for i in range(K_AG)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([NS] * K_AG, PROX_RADIUS, [2] * K_AG)))


def loop_inputs():
    """Starts (the placement), goals, warm starts and the plant's disturbance, drawn as tests/policy_cases.py draws it."""
    x0, xf = placement()
    rng = np.random.default_rng(5151)
    U0 = rng.random((S_LOOP, N_LOOP, K_AG * NC)) * 0.01
    W = pc.W_SCALE * rng.normal(size=(S_LOOP, L_LOOP, K_AG * NS))
    return x0, xf, U0, W
