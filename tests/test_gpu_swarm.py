"""Distributed solves for teams of more than 64 agents, on the GPU (cases: tests/swarm_cases.py; what the oracle alone says about
them: tests/test_swarm_cases.py).

  masks      the multi-word neighbourhood masks, rep, size, order, slot of ScenarioFrontEnd against the host definitions, scenario
             by scenario, exactly -- from the scenarios' states and from trajectories whose rows are sampled
  one word   teams of at most 64 agents on the wide entries (n_words = 1): the narrow entries' arrays, bit for bit
  rollout    ProblemBatch.rollout_wide against oracle.Problem.rollout within the project's rollout tolerance TOL_ROLLOUT (its sums
             have a fixed shape of their own, so dpilqr_rollout's bits are not expected), and against dpilqr_rollout where both serve
  solves     solve_scenarios_distributed / solve_distributed against oracle.solve_distributed within TOL_SOLVE, every agent of
             every scenario (tests/test_swarm_cases.py: the oracle moves by < 1e-9 under a 1e-12 perturbation of these cases)
Every test prints its worst figure next to its tolerance (profiles/swarm_checks.txt records them)."""
import itertools

import numpy as np
import pytest

from tests import swarm_cases as sw
from tests.golden_util import relerr
from tests.policy_cases import TOL_ROLLOUT
from tests.test_host_logic import MODEL_CLASSES, problem_from

pytestmark = pytest.mark.gpu
TOL_SOLVE = 1e-5          # tests/test_gpu_parity.py
TOL_DIST = 1e-14          # min_sep / goal_dist from the device's own trajectory: the same sums of squares, a few ulp for the root


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


def dp_problem(dp, case, xf):
    Q, R, Qf = sw.weights(case)
    k, ns = case.k, case.ns
    ids = [100 + i for i in range(k)]
    dyn = dp.MultiDynamicalModel([MODEL_CLASSES[case.model](sw.DT, id_) for id_ in ids])
    refs = [dp.ReferenceCost(xf[i * ns:(i + 1) * ns], Q.copy(), R.copy(), Qf.copy(), id_) for i, id_ in enumerate(ids)]
    return dp.ilqrProblem(dyn, dp.GameCost(refs, dp.ProximityCost([ns] * k, sw.RADIUS, [case.n_d] * k)))


def host_masks(dp, prob, Xs):
    """define_inter_graph_threshold per scenario -> [S][k] masks as Python ints (bit j = agent j)"""
    ids = prob.ids
    out = []
    for X in Xs:
        g = dp.define_inter_graph_threshold(np.atleast_2d(X), sw.RADIUS, prob.game_cost.x_dims, ids)
        out.append([sw.mask_of(ids.index(int(j)) for j in g[id_]) for id_ in ids])
    return out


def check_front_end(fe, masks):
    """bits, rep, size, order, slot, the bucket starts and counts against the host definitions (tests/test_gpu_api.py:
    test_front_end_on_device_equals_per_scenario_host_graphs), exactly."""
    S, k = fe.S, fe.k
    bits = fe.bits.cpu().numpy().reshape(S, k, -1)
    assert bits.shape[2] == (fe.n_words if fe.wide else 1)
    dev = sw.words_to_masks(bits)
    rep = fe.rep.cpu().numpy().reshape(S, k); size = fe.size.cpu().numpy().reshape(S, k)
    order = fe.order.cpu().numpy(); slot = fe.slot.cpu().numpy().reshape(-1)
    n_unique = 0
    for s in range(S):
        assert list(dev[s]) == masks[s], s
        first = {}
        for i, m in enumerate(masks[s]):
            first.setdefault(m, i)
            assert rep[s, i] == first[m] and size[s, i] == bin(m).count("1"), (s, i)
            n_unique += first[m] == i
    assert int(fe.counts.sum()) == n_unique
    pos = 0
    for kc in range(1, k + 1):
        want = [s * k + i for s in range(S) for i in range(k) if rep[s, i] == i and size[s, i] == kc]
        assert list(order[pos:pos + len(want)]) == want and fe.counts[kc] == len(want) and fe.starts[kc] == pos, kc
        assert [slot[e] for e in want] == list(range(len(want))), kc
        pos += len(want)
    is_rep = rep.reshape(-1) == np.tile(np.arange(k), S)
    assert (slot[~is_rep] == -1).all()
    return n_unique


@pytest.mark.parametrize("case", sw.CASES, ids=lambda c: c.id)
def test_masks_and_buckets_equal_the_host_definitions(dp, case):
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
    prob = dp_problem(dp, case, xf)
    U0s = np.tile(U0[None], (sw.S, 1, 1))
    fe = ScenarioFrontEnd(describe(prob), x0s[:, None, :], U0s, sw.RADIUS, None)
    assert fe.wide and fe.n_words == case.n_words and tuple(fe.bits.shape) == (sw.S * case.k, case.n_words)
    masks = host_masks(dp, prob, x0s[:, None, :])
    n_unique = check_front_end(fe, masks)
    assert sum(len({j // 64 for j in range(case.k) if (m >> j) & 1}) > 1 for m in masks[0]) >= 2      # words are crossed
    # trajectories of 23 rows: every second row is sampled (slice(0, 24, 2)).  The agents drift up to 2.5 in x and y and meet one
    # another on the way; agent k - 2 visits agent 20 on row 5 alone (not sampled), agent k - 3 agent 21 on row 6 alone (sampled)
    rng = np.random.default_rng(50 + case.k)
    N, k = 23, case.k
    drift = np.zeros((sw.S, k, case.ns)); drift[:, :, :2] = rng.uniform(-2.5, 2.5, size=(sw.S, k, 2))
    Xt = (x0s[:, None, :] + np.linspace(0.0, 1.0, N)[None, :, None] * drift.reshape(sw.S, 1, -1)).reshape(sw.S, N, k, case.ns)
    Xt[:, 5, k - 2, :2] = Xt[:, 5, 20, :2] + [0.3, 0.0]
    Xt[:, 6, k - 3, :2] = Xt[:, 6, 21, :2] + [0.3, 0.0]
    Xt = Xt.reshape(sw.S, N, -1)
    fe_t = ScenarioFrontEnd(describe(prob), Xt, U0s, sw.RADIUS, None)
    masks_t = host_masks(dp, prob, Xt)
    n_unique_t = check_front_end(fe_t, masks_t)
    # fewer than twenty rows are all sampled: the first 19 (at k = 256 their positions take more than 64 KiB of LDS), the rest
    fe_19 = ScenarioFrontEnd(describe(prob), Xt[:, :19], U0s, sw.RADIUS, None)
    masks_19 = host_masks(dp, prob, Xt[:, :19])
    check_front_end(fe_19, masks_19)
    masks_rest = host_masks(dp, prob, Xt[:, 19:])
    every_row = [[a | b for a, b in zip(m19, mr)] for m19, mr in zip(masks_19, masks_rest)]
    assert masks_t != masks and masks_t != every_row      # the rows matter, and so does their sampling
    for s in range(sw.S):
        assert not (masks_t[s][20] >> (k - 2)) & 1 and (every_row[s][20] >> (k - 2)) & 1 and (masks_t[s][21] >> (k - 3)) & 1
    print(f"\n[swarm masks {case.id}] exact: {sw.S} x {case.k} masks of {case.n_words} words; distinct neighbourhoods "
          f"{n_unique} (states), {n_unique_t} (sampled trajectories)")


def _one_word_scenarios(dp, golden):
    """(problem, X (S, 1, n_x), U (S, T, n_u)): 64 double integrators with bit 63 in use, and G5's ten quadcopters"""
    case = sw.Case(64, 0, 5)
    x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
    x = x0s.reshape(sw.S, 64, 4)
    x[:, 63, :2] = x[:, 0, :2] + [0.0, 0.6]; x[:, 62, :2] = x[:, 0, :2] - [0.0, 0.6]      # agent 0's triple reaches bit 63
    x[:, 40, :2] = x[:, 41, :2] + [0.6, 0.0]                                               # and one shared neighbourhood (Q11)
    yield dp_problem(dp, case, xf), x.reshape(sw.S, 1, -1), np.tile(U0[None], (sw.S, 1, 1))
    z = golden("g5_dispatch"); tag = "quad10"
    k, ns = int(z[tag + "_k"]), int(z[tag + "_n_s"])
    rng = np.random.default_rng(3)
    x0 = np.tile(z[tag + "_x0"].reshape(1, -1), (9, 1)); x0[1:, 0::ns] += rng.normal(scale=0.15, size=(8, k))
    yield problem_from(z, tag + "_"), x0[:, None, :], np.tile(z[tag + "_U0"][None], (9, 1, 1))


def test_one_word_wide_entries_reproduce_the_narrow_entries(dp, golden):
    import torch
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    for prob, X, U in _one_word_scenarios(dp, golden):
        d = describe(prob)
        fn = ScenarioFrontEnd(d, X, U, sw.RADIUS, None)
        fw = ScenarioFrontEnd(d, X, U, sw.RADIUS, None, wide=True)
        assert not fn.wide and fw.wide and fw.n_words == 1 and tuple(fw.bits.shape) == (fn.S * fn.k, 1)
        if fn.k == 64:
            assert int((fn.bits.cpu().numpy().view(np.uint64) >> np.uint64(63)).sum()) >= 2      # bit 63 is in use
        for name in ("bits", "rep", "size", "order", "slot", "bstart", "bcount"):
            a, b = getattr(fn, name).cpu().numpy().reshape(-1), getattr(fw, name).cpu().numpy().reshape(-1)
            if name == "order":      # the sort fills the first n_unique entries
                a, b = a[:int(fn.counts.sum())], b[:int(fw.counts.sum())]
            assert np.array_equal(a, b), name
        gen = torch.Generator(device="cpu").manual_seed(5)
        solved_n, solved_w = {}, {}
        for kc in fn.sizes():
            (pn, x0n, U0n), (pw, x0w, U0w) = fn.bucket(kc), fw.bucket(kc)
            assert torch.equal(x0n, x0w) and torch.equal(U0n, U0w) and torch.equal(pn._xf, pw._xf), kc
            cnt = int(fn.counts[kc])
            Xs = torch.rand((cnt, fn.T + 1, kc * fn.n_s), generator=gen, dtype=torch.float64).to(x0n.device)
            Us = torch.rand((cnt, fn.T, kc * fn.n_c), generator=gen, dtype=torch.float64).to(x0n.device)
            solved_n[kc] = solved_w[kc] = (Xs, Us, 0, cnt)
        (Xn, Un), (Xw, Uw) = fn.stitch(solved_n), fw.stitch(solved_w)
        assert torch.equal(Xn, Xw) and torch.equal(Un, Uw) and bool((Xn != 0).any())
    print("\n[swarm one word] wide entries with n_words = 1: bits, rep, size, order, slot, buckets, gathers, stitch equal the narrow entries' bit for bit")


def _planar_min_sep(X, k, ns):
    """min over rows and pairs of the planar distance, as the kernel sums it: (0 + dx dx) + dy dy, then one root"""
    P = X.reshape(X.shape[0], k, ns)[:, :, :2]
    i, j = np.triu_indices(k, 1)
    d = P[:, i, :] - P[:, j, :]
    return float(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min()))


@pytest.mark.parametrize("case", sw.CASES, ids=lambda c: c.id)
def test_rollout_wide_against_the_oracle(dp, case):
    k, ns, nc, T = case.k, case.ns, case.nc, case.T
    x0s, xf, U0 = sw.scenario(case, sw.OFFSET_ROLLOUT)
    rng = np.random.default_rng(900 + k)
    U = U0[None] + 0.5 * rng.normal(size=(sw.S, T, k * nc))
    if ns >= 6:      # heights differ: with one n_dims for every agent the distances are planar all the same (quirk Q5)
        x0s = x0s.copy(); x0s.reshape(sw.S, k, ns)[:, :, 2] += 0.3 * rng.normal(size=(sw.S, k))
    Q, R, Qf = sw.weights(case)
    pb = dp.ProblemBatch([case.model] * k, [case.n_d] * k, xf[None], Q, R, Qf, sw.RADIUS, sw.DT, T, B=sw.S)
    r = {key: v.cpu().numpy() for key, v in pb.rollout_wide(x0s, U).items()}
    again = pb.rollout_wide(x0s, U, trajectories=False)
    assert "X" not in again and np.array_equal(again["J"].cpu().numpy(), r["J"])      # X = NULL; the same bits run after run
    po = sw.oracle_problem(case, xf)
    worst = dict(X=0.0, J=0.0, sep=0.0, goal=0.0)
    n_prox = 0      # scenarios whose proximity cost is in play (the jitter can take a pair of partners apart)
    for s in range(sw.S):
        Xo, Jo = po.rollout(x0s[s], U[s])
        prox = sum(po.prox_cost(Xo[t]) for t in range(T + 1))
        assert prox > 0.0 or s > 0      # scenario 0, as generated: the partners start inside the radius, pairs across a word boundary pay
        n_prox += prox > 0.0
        worst["X"] = max(worst["X"], relerr(r["X"][s], Xo)); worst["J"] = max(worst["J"], abs(r["J"][s] - Jo) / abs(Jo))
        sep = _planar_min_sep(r["X"][s], k, ns)
        worst["sep"] = max(worst["sep"], abs(r["min_sep"][s] - sep) / sep)
        e = (r["X"][s][-1] - xf).reshape(k, ns)[:, :case.n_d]
        g2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        goal = np.sqrt(g2 + e[:, 2] * e[:, 2] if case.n_d == 3 else g2)
        worst["goal"] = max(worst["goal"], float(np.max(np.abs(r["goal_dist"][s] - goal) / goal)))
        if ns >= 6:      # Q5: not the distance over three coordinates
            P3 = r["X"][s].reshape(T + 1, k, ns)[:, :, :3]
            i, j = np.triu_indices(k, 1)
            assert abs(np.sqrt(((P3[:, i] - P3[:, j]) ** 2).sum(-1)).min() - sep) > 1e-6
    print(f"\n[swarm rollout {case.id}] vs oracle: X {worst['X']:.2e}, J {worst['J']:.2e} (tol {TOL_ROLLOUT:.0e}); vs NumPy on the device's X: "
          f"min_sep {worst['sep']:.2e}, goal_dist {worst['goal']:.2e} (tol {TOL_DIST:.0e})")
    assert n_prox >= 2
    assert worst["X"] < TOL_ROLLOUT and worst["J"] < TOL_ROLLOUT
    assert worst["sep"] < TOL_DIST and worst["goal"] < TOL_DIST


@pytest.mark.parametrize("name,models,n_dims,dt", [("quad12_human12-k20", [7, 8] * 10, [3, 2] * 10, 0.05),
                                                   ("dint4_uni4-k5", [0, 3, 0, 3, 3], [2] * 5, 0.1),
                                                   ("dint4-k1", [0], [2], 0.1)])
def test_rollout_wide_against_dpilqr_rollout(dp, name, models, n_dims, dt):
    """Where both entries serve a team they agree to rounding: mixed models, mixed n_dims (pairs over min(n_dims_i, n_dims_j)
    coordinates), per-agent weights, per-item goals; a lone agent has no pair (min_sep = +inf)."""
    k, T, B = len(models), 6, 4
    ns, nc = sw.MODEL_DIMS.get(models[0], (12, 4))
    rng = np.random.default_rng(len(name))
    xf = rng.normal(size=(B, k * ns)) * 0.8; x0 = rng.normal(size=(B, k * ns)) * 0.8
    x0.reshape(B, k, ns)[:, :, 3:] *= 0.02
    U = 0.5 * rng.normal(size=(B, T, k * nc))
    if ns == 12:      # near hover (tests/policy_cases.py)
        U = U * 1e-4; U[:, :, 3::4] += sw.G_ACC * 63.0 / 2000.0
    draw = lambda n, s: np.stack([np.diag(rng.uniform(0.5, 2.0, n)) * s + 0.05 * s * rng.normal(size=(n, n)) for _ in range(k)])
    pb = dp.ProblemBatch(models, n_dims, xf, draw(ns, 1.0), draw(nc, 1.0), draw(ns, 100.0), 0.9, dt, T)
    Xr, Jr = pb.rollout(x0, U)
    r = pb.rollout_wide(x0, U)
    Xr, Jr, Xw, Jw = Xr.cpu().numpy(), Jr.cpu().numpy(), r["X"].cpu().numpy(), r["J"].cpu().numpy()
    eX, eJ = relerr(Xw, Xr), float(np.max(np.abs(Jw - Jr) / np.abs(Jr)))
    sep = r["min_sep"].cpu().numpy()
    if k == 1:
        assert np.isinf(sep).all() and (sep > 0).all()
    else:
        nd = np.minimum.outer(np.array(n_dims), np.array(n_dims))
        for b in range(B):
            P = Xw[b].reshape(T + 1, k, ns)
            want = min(np.sqrt(sum((P[:, i, c] - P[:, j, c]) * (P[:, i, c] - P[:, j, c]) for c in range(nd[i, j])).min())
                       for i, j in itertools.combinations(range(k), 2))
            assert abs(sep[b] - want) < TOL_DIST * want, (b, sep[b], want)
        assert sep.min() < 0.9      # pairs inside the radius: the proximity cost is in play
    print(f"\n[swarm rollout {name}] rollout_wide vs dpilqr_rollout: X {eX:.2e}, J {eJ:.2e} (tol {TOL_ROLLOUT:.0e})")
    assert eX < TOL_ROLLOUT and eJ < TOL_ROLLOUT


@pytest.mark.parametrize("case", sw.SOLVE_CASES, ids=lambda c: c.id)
def test_distributed_solves_against_the_oracle(dp, case):
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    ci = sw.CASES.index(case)
    k, S = case.k, sw.S
    x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
    prob = dp_problem(dp, case, xf)
    U0s = np.tile(U0[None], (S, 1, 1))
    Xd, Ud, Jf, info = solve_scenarios_distributed(prob, x0s[:, None, :], U0s, sw.RADIUS, n_lqr_iter=sw.N_LQR_ITER)
    assert info["cluster_bits"].shape == (S, k, case.n_words) and max(info["sizes"]) <= 6
    dev_masks = sw.words_to_masks(info["cluster_bits"])
    worst = [0.0, 0.0]
    for s in range(S):
        Xo, Uo, Jo, graph = sw.oracle_solve(ci, s)
        assert list(dev_masks[s]) == [sw.mask_of(graph[i]) for i in range(k)], s
        ns, nc = case.ns, case.nc
        for i in range(k):      # every agent of every scenario, against its own columns
            worst[0] = max(worst[0], relerr(Xd[s][:, i * ns:(i + 1) * ns], Xo[:, i * ns:(i + 1) * ns]),
                           relerr(Ud[s][:, i * nc:(i + 1) * nc], Uo[:, i * nc:(i + 1) * nc]))
        worst[0] = max(worst[0], abs(Jf[s] - Jo) / abs(Jo))
    # the receding-horizon pattern: a second call seeded with the first result (the graph from sampled trajectory rows)
    Xd2, Ud2, Jf2, info2 = solve_scenarios_distributed(prob, Xd, Ud, sw.RADIUS, n_lqr_iter=sw.N_LQR_ITER)
    po = sw.oracle_problem(case, xf)
    dev_masks2 = sw.words_to_masks(info2["cluster_bits"])
    for s in range(S):
        Xo, Uo, Jo, graph = sw.orc.solve_distributed(po, Xd[s], Ud[s], sw.RADIUS, n_lqr_iter=sw.N_LQR_ITER)
        assert list(dev_masks2[s]) == [sw.mask_of(graph[i]) for i in range(k)], s
        worst[1] = max(worst[1], relerr(Xd2[s], Xo), relerr(Ud2[s], Uo), abs(Jf2[s] - Jo) / abs(Jo))
    # the one-scenario entry: the same sub-problem solves, the same stitch, the same full-team rollout
    Xs, Us, Js, si = dp.solve_distributed(prob, x0s[0].reshape(1, -1), U0, sw.RADIUS, verbose=False, n_lqr_iter=sw.N_LQR_ITER)
    print(f"\n[swarm solve {case.id}] vs oracle.solve_distributed, worst agent of {S} scenarios: first call {worst[0]:.2e}, seeded second "
          f"call {worst[1]:.2e} (tol {TOL_SOLVE:.0e}); sub-problems {info['n_unique']} of {info['n_subproblems']}, sizes {info['sizes']}")
    assert worst[0] < TOL_SOLVE and worst[1] < TOL_SOLVE
    assert np.array_equal(Xs, Xd[0]) and np.array_equal(Us, Ud[0]) and Js == Jf[0]
    assert set(si) == set(prob.ids) and [prob.ids.index(int(j)) for j in si[prob.ids[10]][1]] == sw.oracle_solve(ci, 0)[3][10]


def test_refusals_on_the_device(dp):
    """policy=True and shard= are not built for a wide team; a cluster of more than 64 agents is refused before any solve, by size
    and count; beyond 256 agents nothing is."""
    from dpilqr_amd.dispatch import ScenarioFrontEnd, solve_scenarios_distributed
    from dpilqr_amd.lowering import describe
    case = sw.CASES[0]
    x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
    prob = dp_problem(dp, case, xf)
    U0s = np.tile(U0[None], (sw.S, 1, 1))
    with pytest.raises(ValueError, match="policy=True is not built for teams of more than 64 agents"):
        solve_scenarios_distributed(prob, x0s[:, None, :], U0s, sw.RADIUS, policy=True)
    with pytest.raises(ValueError, match="shard= is not built for teams of more than 64 agents"):
        solve_scenarios_distributed(prob, x0s[:, None, :], U0s, sw.RADIUS, shard=(0, 1))
    # all 65 agents of scenario 1 within the threshold of one another: one neighbourhood of 65, shared by all (one sub-problem)
    crowd = x0s.copy(); crowd.reshape(sw.S, case.k, case.ns)[1, :, :2] *= 0.01
    with pytest.raises(ValueError, match="at most 64 agents; this team has 1 sub-problem of cluster size 65"):
        ScenarioFrontEnd(describe(prob), crowd[:, None, :], U0s, sw.RADIUS, None)
    pb = dp.ProblemBatch([0] * 65, [2] * 65, xf[None], *sw.weights(case), sw.RADIUS, sw.DT, case.T)
    with pytest.raises(Exception, match="exceeds 64"):      # the narrow rollout keeps its limit
        pb.rollout(x0s[:1], U0s[:1])
