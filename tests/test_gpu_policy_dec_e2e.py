"""The distributed closed loop end to end: solve_scenarios_distributed(policy=True) -> the stitch of gains
(dpilqr_dispatch_stitch_policy) -> DistributedPolicy.rollout (dpilqr_policy_rollout_dec), on three hand-placed scenarios of four
agents (DoubleIntDynamics4D and UnicycleDynamics4D, T = 12) whose neighbourhoods have 4; 2, 3, 2, 1; and 1 members.

  stitch      Kc and U_ff against a NumPy gather of the bucket tensors read back (audit=True): gathered entries exactly equal,
              columns past a neighbourhood zero, U_ff within 1e-12 relative and equal to U_dec where the scenario is one cluster
  definition  five perturbed starts per scenario against a NumPy loop of u_i = U^i[pos] + K^i[pos] (x_{C_i} - X^i), unfolded, with
              K^i the ORACLE's backward pass at the GPU's sub-problem solutions; the bound is policy_cases.bound_of of the
              reference's own change under +-PERTURB relative perturbations of the starts, X^i, U^i and K^i
  invariants  a radius that joins everyone: the centralised policy_rollout at the stitched trajectory, within that bound;
              a radius that joins no one: every agent's columns equal its own k = 1 closed loop
  closed_loop_distributed returns scenario 0's numbers."""
import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests import policy_cases as pc

pytestmark = pytest.mark.gpu

K_AG, NS, NC, T, DT = 4, 4, 2, 12, 0.1
MODELS = [0, 3, 0, 3]
N_DIMS = [2] * K_AG
RADIUS, PROX_RADIUS, MU = 0.5, 0.5, 1.0
N_STARTS = 5
Q, R, QF = np.diag([1.0, 1.0, 0.5, 0.5]), np.eye(NC), 100.0 * np.eye(NS)

POS0 = np.array([[[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [0.5, 0.5]],          # one cluster of four
                 [[0.0, 0.0], [0.8, 0.0], [1.6, 0.0], [5.0, 5.0]],          # a chain 0 - 1 - 2 and a loner: sizes 2, 3, 2, 1
                 [[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 4.0]]])         # nobody near anybody
GOAL = np.array([[[1.5, 1.5], [-1.0, 1.5], [1.5, -1.0], [-1.0, -1.0]],
                 [[1.6, 0.5], [1.1, 1.0], [0.0, 0.5], [4.0, 4.0]],          # (agent 1 off the chain's mirror axis: a unicycle at
                                                                            # rest there, its goal abeam, has controls of rounding size)
                 [[1.0, 1.0], [3.0, 1.0], [1.0, 3.0], [3.0, 3.0]]])
S = POS0.shape[0]


def _states(pos):
    x = np.zeros((S, K_AG, NS))
    x[:, :, :2] = pos
    return x.reshape(S, -1)


X0, XF = _states(POS0), _states(GOAL)


def _problem(xf=XF[0]):
    import dpilqr_amd as dp
    dp._reset_ids()
    mk = {0: dp.DoubleIntDynamics4D, 3: dp.UnicycleDynamics4D}
    dyn = dp.MultiDynamicalModel([mk[m](DT) for m in MODELS])
    costs = [dp.ReferenceCost(xf[NS * i:NS * (i + 1)], Q, R, QF, i) for i in range(K_AG)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([NS] * K_AG, PROX_RADIUS, N_DIMS)))


def _members(mask):
    return [j for j in range(K_AG) if (int(mask) >> j) & 1]


def test_the_scenarios_have_the_cluster_sizes_they_are_placed_for():
    """On the CPU, with the package's own NumPy graph function."""
    from dpilqr_amd.distributed import define_inter_graph_threshold
    sizes = [[len(v) for v in define_inter_graph_threshold(X0[s][None], RADIUS, [NS] * K_AG, list(range(K_AG))).values()] for s in range(S)]
    assert sizes == [[4, 4, 4, 4], [2, 3, 2, 1], [1, 1, 1, 1]]


def _owners(bits):
    """(bucket size, slot, members, pos) of every (s, i): representatives in (s, i) order inside their size's bucket."""
    count, slot_of = {}, {}
    for s in range(S):
        for i in range(K_AG):
            key = (s, int(bits[s, i]))
            if key not in slot_of:
                kc = len(_members(bits[s, i]))
                slot_of[key] = count.get(kc, 0)
                count[kc] = slot_of[key] + 1
    out = {}
    for s in range(S):
        for i in range(K_AG):
            mem = _members(bits[s, i])
            out[s, i] = (len(mem), slot_of[s, int(bits[s, i])], mem, mem.index(i))
    return out


_SOLVED = {}


def solved(radius=RADIUS):
    if radius not in _SOLVED:
        import dpilqr_amd as dp
        X_dec, U_dec, J, info = dp.solve_scenarios_distributed(_problem(), X0[:, None, :], np.zeros((S, T, K_AG * NC)), radius, xf=XF,
                                                               audit=True, policy=True, policy_mu=MU, n_lqr_iter=20)
        pol = info["policy"]
        _SOLVED[radius] = dict(X_dec=X_dec, U_dec=U_dec, info=info, pol=pol, bits=info["cluster_bits"].astype(np.uint64),
                               Kc=pol.Kc.cpu().numpy(), U_ff=pol.U_ff.cpu().numpy())
    return _SOLVED[radius]


def test_stitch_against_numpy():
    r = solved()
    aud, bits = r["info"]["audit"], r["bits"]
    assert sorted(aud) == [1, 2, 3, 4] and r["pol"].kc_max == 4
    assert np.array_equal(r["pol"].bits.cpu().numpy().astype(np.uint64), bits)
    assert np.array_equal(r["pol"].X_dec.cpu().numpy(), r["X_dec"])
    own = _owners(bits)
    Kc, U_ff = r["Kc"], r["U_ff"]
    assert Kc.shape == (S, T, K_AG, NC, 4 * NS) and U_ff.shape == (S, T, K_AG * NC)
    for (s, i), (kc, slot, mem, pos) in own.items():
        Xi, Ui, Ki = aud[kc]["X"][slot], aud[kc]["U"][slot], aud[kc]["K"][slot]
        assert Ki.shape == (T, kc * NC, kc * NS)
        assert np.array_equal(Kc[s, :, i, :, :kc * NS], Ki[:, pos * NC:(pos + 1) * NC, :]), (s, i)
        assert (Kc[s, :, i, :, kc * NS:] == 0.0).all(), (s, i)
        cols = np.concatenate([np.arange(j * NS, (j + 1) * NS) for j in mem])
        assert np.array_equal(r["X_dec"][s][:, i * NS:(i + 1) * NS], Xi[:, pos * NS:(pos + 1) * NS])
        want = Ui[:, pos * NC:(pos + 1) * NC] + np.einsum("tcj,tj->tc", Ki[:, pos * NC:(pos + 1) * NC, :], r["X_dec"][s][:T, cols] - Xi[:T])
        got = U_ff[s][:, i * NC:(i + 1) * NC]
        assert np.max(np.abs(want)) > 0.1, (s, i)      # a genuine control: the relative bound below has a scale to stand on
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (s, i, np.max(np.abs(got - want)))
    assert np.array_equal(U_ff[0], r["U_dec"][0])            # one cluster: the folded term is K . 0
    assert not np.array_equal(U_ff[1], r["U_dec"][1])        # the chain: the neighbours' predictions differ from the stitch


def _full_problem(s):
    return lc.orc.Problem(MODELS, N_DIMS, XF[s], np.broadcast_to(Q, (K_AG, NS, NS)), np.broadcast_to(R, (K_AG, NC, NC)),
                          np.broadcast_to(QF, (K_AG, NS, NS)), PROX_RADIUS, DT, T)


def _sub_policies(r, s, gains="oracle"):
    """Per agent of scenario s: (members' state columns, pos, X^i, U^i, K^i), K^i the oracle's backward pass at the GPU's
    sub-problem solution."""
    aud, own = r["info"]["audit"], _owners(r["bits"])
    subs = []
    for i in range(K_AG):
        kc, slot, mem, pos = own[s, i]
        Xi, Ui = aud[kc]["X"][slot], aud[kc]["U"][slot]
        p = lc.orc.Problem([MODELS[j] for j in mem], [N_DIMS[j] for j in mem], aud[kc]["xf"][slot], np.broadcast_to(Q, (kc, NS, NS)),
                           np.broadcast_to(R, (kc, NC, NC)), np.broadcast_to(QF, (kc, NS, NS)), PROX_RADIUS, DT, T)
        Ki, _ = p.backward_pass(Xi, Ui, MU)
        cols = np.concatenate([np.arange(j * NS, (j + 1) * NS) for j in mem])
        subs.append((cols, pos, Xi, Ui, np.asarray(Ki)))
    return subs


def ref_definition(p, s, subs, x0, W=None, u_lim=None, e=0.0):
    """Definition (1), unfolded; e: the relative perturbation of the sensitivity runs."""
    n, m = K_AG * NS, K_AG * NC
    Xs = np.zeros((T + 1, n)); Us = np.zeros((T, m))
    Xs[0] = x0 * (1 + e)
    J, sep = 0.0, pc.separation(Xs[0], K_AG, NS, N_DIMS)
    for t in range(T):
        u = np.zeros(m)
        for i, (cols, pos, Xi, Ui, Ki) in enumerate(subs):
            rows = slice(pos * NC, (pos + 1) * NC)
            u[i * NC:(i + 1) * NC] = Ui[t, rows] * (1 - e) + (Ki[t, rows, :] * (1 - e)) @ (Xs[t][cols] - Xi[t] * (1 + e))
        if u_lim is not None:
            u = np.where(u < u_lim[0], u_lim[0], np.where(u > u_lim[1], u_lim[1], u))
        Us[t] = u
        J += float(p.cost(Xs[t], u))
        Xs[t + 1] = p.step(Xs[t], u)
        if W is not None:
            Xs[t + 1] += W[t]
        sep = min(sep, pc.separation(Xs[t + 1], K_AG, NS, N_DIMS))
    J += float(p.cost(Xs[-1], np.zeros(m), True))
    err = (Xs[-1] - XF[s]).reshape(K_AG, NS)
    return dict(X=Xs, U=Us, J=J, min_sep=sep, goal_dist=np.sqrt(np.sum(err[:, :2] ** 2, axis=1)))


def _starts():
    from dpilqr_amd.util import perturbed_starts
    return np.stack([perturbed_starts(X0[s], [NS] * K_AG, N_STARTS, var=0.2, seed=40 + s) for s in range(S)])


def _check(got, r, x0s, W=None, u_lim=None):
    worst, unchecked = 0.0, 0
    for s in range(S):
        p, subs = _full_problem(s), _sub_policies(r, s)
        for q in range(N_STARTS):
            Wq = None if W is None else W[s, q]
            ref = ref_definition(p, s, subs, x0s[s, q], Wq, u_lim)
            spread = max(pc.difference(ref_definition(p, s, subs, x0s[s, q], Wq, u_lim, e=sg * lc.PERTURB), ref) for sg in (1.0, -1.0))
            bound = pc.bound_of(spread)
            if bound is None:
                unchecked += 1
                continue
            g = dict(X=got["X"][s, q], U=got["U"][s, q], J=float(got["J"][s, q]), min_sep=float(got["min_sep"][s, q]),
                     goal_dist=got["goal_dist"][s, q])
            d = pc.difference(g, ref)
            print(f"scenario {s} start {q}: difference {d:.3g}, bound {bound:.3g}")
            worst = max(worst, d / bound)
            assert d <= bound, (s, q, d, bound)
    assert unchecked <= pc.MAX_UNCHECKED * S * N_STARTS, unchecked
    return worst


def test_against_the_definition():
    r = solved()
    x0s = _starts()
    got = {k_: v.cpu().numpy() for k_, v in r["pol"].rollout(x0s, trajectories=True).items()}
    _check(got, r, x0s)
    rng = np.random.default_rng(5)
    W = pc.W_SCALE * rng.normal(size=(S, N_STARTS, T, K_AG * NS))
    flat = got["U"].reshape(-1, K_AG * NC)
    u_lim = np.stack([np.quantile(flat, pc.QUANTILES[0], axis=0), np.quantile(flat, pc.QUANTILES[1], axis=0)])
    got2 = {k_: v.cpu().numpy() for k_, v in r["pol"].rollout(x0s, W=W, u_lim=u_lim, trajectories=True).items()}
    assert np.mean((got2["U"] == u_lim[0]) | (got2["U"] == u_lim[1])) > 0.10
    _check(got2, r, x0s, W, u_lim)
    short = r["pol"].rollout(x0s, W=W, u_lim=u_lim)
    assert set(short) == {"J", "min_sep", "goal_dist"} and all(np.array_equal(short[k_].cpu().numpy(), got2[k_]) for k_ in short)


def test_a_radius_that_joins_everyone_is_the_centralised_closed_loop():
    r = solved(radius=50.0)
    assert (r["bits"] == 15).all() and sorted(r["info"]["audit"]) == [4]
    assert np.array_equal(r["U_ff"], r["U_dec"])
    x0s = _starts()
    got = {k_: v.cpu().numpy() for k_, v in r["pol"].rollout(x0s, trajectories=True).items()}
    K = r["info"]["audit"][4]["K"]
    cen = {k_: v.cpu().numpy() for k_, v in r["pol"].batch().policy_rollout(r["X_dec"], r["U_dec"], K, x0s, trajectories=True).items()}
    unchecked = 0
    for s in range(S):
        p, subs = _full_problem(s), _sub_policies(r, s)
        for q in range(N_STARTS):
            ref = ref_definition(p, s, subs, x0s[s, q])
            bound = pc.bound_of(max(pc.difference(ref_definition(p, s, subs, x0s[s, q], e=sg * lc.PERTURB), ref) for sg in (1.0, -1.0)))
            if bound is None:
                unchecked += 1
                continue
            g, c = ({k_: (float(o[k_][s, q]) if k_ in ("J", "min_sep") else o[k_][s, q]) for k_ in o} for o in (got, cen))
            assert pc.difference(g, c) <= bound, (s, q, pc.difference(g, c), bound)
    assert unchecked <= pc.MAX_UNCHECKED * S * N_STARTS, unchecked


def test_a_radius_that_joins_no_one_is_every_agent_alone():
    import dpilqr_amd as dp
    r = solved(radius=1e-3)
    assert all(int(r["bits"][s, i]) == 1 << i for s in range(S) for i in range(K_AG)) and sorted(r["info"]["audit"]) == [1]
    x0s = _starts()
    got = {k_: v.cpu().numpy() for k_, v in r["pol"].rollout(x0s, trajectories=True).items()}
    a = r["info"]["audit"][1]                      # the twelve one-agent sub-problems in (s, i) order
    models = np.array([[MODELS[i]] for s in range(S) for i in range(K_AG)], dtype=np.int32)
    pb1 = dp.ProblemBatch(models, np.full((S * K_AG, 1), 2, dtype=np.int32), a["xf"], Q, R, QF, PROX_RADIUS, DT, T)
    own = {k_: v.cpu().numpy() for k_, v in pb1.policy_rollout(a["X"], a["U"], a["K"], x0s.reshape(S, N_STARTS, K_AG, NS).transpose(0, 2, 1, 3)
                                                                   .reshape(S * K_AG, N_STARTS, NS), trajectories=True).items()}
    for s in range(S):
        for i in range(K_AG):
            assert np.array_equal(got["X"][s][:, :, i * NS:(i + 1) * NS], own["X"][s * K_AG + i]), (s, i)
            assert np.array_equal(got["U"][s][:, :, i * NC:(i + 1) * NC], own["U"][s * K_AG + i]), (s, i)
            assert np.array_equal(got["goal_dist"][s][:, i], own["goal_dist"][s * K_AG + i][:, 0]), (s, i)


def test_closed_loop_distributed_returns_scenario_zero():
    import dpilqr_amd as dp
    r = solved()
    x0s = _starts()
    got = {k_: v.cpu().numpy() for k_, v in r["pol"].rollout(x0s, trajectories=True).items()}
    one = dp.closed_loop_distributed(_problem(XF[0]), X0[0][None], np.zeros((T, K_AG * NC)), RADIUS, x0s[0], mu=MU, trajectories=True,
                                     n_lqr_iter=20)
    assert np.array_equal(one["X_dec"], r["X_dec"][0]) and np.array_equal(one["U_dec"], r["U_dec"][0])
    for key in ("J", "min_sep", "goal_dist", "X", "U"):
        assert np.array_equal(one[key], got[key][0]), key
