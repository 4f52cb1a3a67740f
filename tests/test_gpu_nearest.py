"""Neighbourhoods capped at their m nearest agents (dpilqr_dispatch_graph_nearest, csrc/frontend_nearest.hpp), on the GPU (cases:
tests/nearest_cases.py; what the CPU alone says about them: tests/test_nearest_cases.py).

  masks        bits, rep, size, order, slot, bucket starts and counts and `dropped` of ScenarioFrontEnd(max_cluster=m) against the
               brute-force reference and the host definitions, exactly -- from the states (N = 1) and from 11 sampled rows; the
               hand-made scenarios (exact ties on either side of bit 64, a later row deciding the cut, a cap that bites for some);
               `ignore`
  no-op        with m = min(k, 64) on the sparse swarms of tests/swarm_cases.py all seven arrays equal dispatch_graph_wide's, and
               for k <= 64 with n_words = 1 dispatch_graph's, bit for bit
  position     a scenario gives the same arrays alone as in a batch; guard words around bits and dropped stay untouched; a NaN
               position in one scenario changes no other
  solves       solve_scenarios_distributed(max_cluster=m) against the oracle's capped distributed solve within TOL_SOLVE, every
               agent of every scenario; without the cap the k = 130 team is refused and the k = 64 team fails in the solver
  closed loop  policy.rollout against the NumPy definition of the distributed policy on the device's Kc, U_ff and bits within
               bound_of(spread) (tests/policy_cases.py); solve_rhc_closed_loop(wide=True, max_cluster=4) on the 64-agent near-clique
Every test prints its worst figure next to its bound (profiles/nearest_checks.txt records them)."""
import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests import nearest_cases as nc
from tests import policy_cases as pc
from tests import policy_dec_wide_cases as wc
from tests import swarm_cases as sw
from tests import test_gpu_swarm as tgs
from tests.golden_util import relerr

pytestmark = pytest.mark.gpu
TOL_SOLVE = 1e-5          # tests/test_gpu_swarm.py; its ground here: tests/test_nearest_cases.py::test_capped_solves_are_insensitive_to_rounding
GUARD = -0x0123456789ABCDEF
ARRAYS = ("bits", "rep", "size", "order", "slot", "bstart", "bcount")


@pytest.fixture(scope="module")
def dp():
    import dpilqr_amd
    from dpilqr_amd import _lib
    _lib.require_gpu()
    return dpilqr_amd


def front_end(dp, k, X, radius, m, ignore=None, wide=None):
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    case = nc.Case(k, m or 1)
    prob = tgs.dp_problem(dp, case, np.zeros(k * nc.NS))
    X = np.asarray(X)
    return ScenarioFrontEnd(describe(prob), X, np.zeros((X.shape[0], 2, k * nc.NC)), radius, None, ignore, wide=wide, max_cluster=m)


def arrays(fe):
    out = {name: getattr(fe, name).cpu().numpy().reshape(-1) for name in ARRAYS}
    out["order"] = out["order"][:int(fe.counts.sum())]      # the sort fills the first n_unique entries
    if fe.dropped is not None:
        out["dropped"] = fe.dropped.cpu().numpy().reshape(-1)
    return out


def check_capped(fe, X, k, radius, m):
    """Every array of the front end against the reference masks and the host definitions; returns the agents the cap bit."""
    refs = [nc.reference(X[s], k, nc.NS, radius, m) for s in range(len(X))]
    tgs.check_front_end(fe, [nc.masks_of(r[0], k) for r in refs])
    dropped = fe.dropped.cpu().numpy().reshape(len(X), k)
    assert np.array_equal(dropped, np.stack([r[1] for r in refs]))
    assert int(fe.size.max()) <= m
    return int((dropped > 0).sum())


@pytest.mark.parametrize("case", nc.CASES, ids=nc.IDS)
def test_masks_buckets_and_dropped_equal_the_host_reference(dp, case):
    x0, _, X = nc.scenario(case.k)
    k, m = case.k, case.m
    fe = front_end(dp, k, x0[:, None, :], nc.GRAPH_RADIUS, m)
    assert fe.wide == (k > 64) and tuple(fe.bits.shape) == ((nc.S * k, case.n_words) if k > 64 else (nc.S * k,)) and fe.max_cluster == m
    bites = check_capped(fe, x0[:, None, :], k, nc.GRAPH_RADIUS, m)
    fe_rows = front_end(dp, k, X, nc.GRAPH_RADIUS, m)      # 11 rows, all sampled: the key is the minimum over them
    bites_rows = check_capped(fe_rows, X, k, nc.GRAPH_RADIUS, m)
    if k <= 64:      # the same team on the wide entries' word layout: the same arrays
        fw = front_end(dp, k, X, nc.GRAPH_RADIUS, m, wide=True)
        assert tuple(fw.bits.shape) == (nc.S * k, 1) and all(np.array_equal(a, b) for a, b in zip(arrays(fe_rows).values(), arrays(fw).values()))
    print(f"\n[nearest masks {case.id}] exact: {nc.S} x {k} masks of {case.n_words} words, rep, size, order, slot, buckets, dropped; the cap bit "
          f"{bites} (states) and {bites_rows} (11 rows) of {nc.S * k} agents (0 differences, 0 allowed)")
    assert bites > 0 and bites_rows > 0


@pytest.mark.parametrize("hand", nc.HAND, ids=nc.HAND_IDS)
def test_hand_made_scenarios(dp, hand):
    k, m = hand["k"], hand["m"]
    fe = front_end(dp, k, hand["X"][None], hand["radius"], m)
    bites = check_capped(fe, hand["X"][None], k, hand["radius"], m)
    print(f"\n[nearest hand-made {hand['name']}] exact: masks and dropped equal the reference (0 differences, 0 allowed); the cap bit {bites} agents")
    assert bites > 0


def test_ignored_agents_stay_candidates(dp):
    k, m = 65, 4
    x0, _, X = nc.scenario(k)
    ignore = [1 if i in (0, 7, 64) else 0 for i in range(k)]
    fe, fi = front_end(dp, k, X, nc.GRAPH_RADIUS, m), front_end(dp, k, X, nc.GRAPH_RADIUS, m, ignore=ignore)
    a, b = arrays(fe), arrays(fi)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["dropped"], b["dropped"])      # the masks do not know `ignore`
    masks = sw.words_to_masks(fi.bits.cpu().numpy().reshape(nc.S, k, -1))
    for s in range(nc.S):
        rep, size = nc.derive(list(masks[s]), ignore)
        assert np.array_equal(b["rep"].reshape(nc.S, k)[s], rep) and np.array_equal(b["size"].reshape(nc.S, k)[s], size)
    assert (b["rep"].reshape(nc.S, k)[:, [0, 7, 64]] == -1).all() and any((int(masks[0][i]) >> 64) & 1 for i in range(k) if i != 64)
    print("\n[nearest ignore] exact: ignored agents get rep -1 and size 0 and stay members of the others' capped neighbourhoods")


def test_a_cap_that_never_bites_is_todays_graph(dp, golden):
    from dpilqr_amd.dispatch import ScenarioFrontEnd
    from dpilqr_amd.lowering import describe
    n = 0
    for case in sw.CASES:      # sparse swarms: neighbourhoods of at most 6
        x0s, xf, U0 = sw.scenario(case, sw.OFFSET_SOLVE)
        d = describe(tgs.dp_problem(dp, case, xf))
        U0s = np.tile(U0[None], (sw.S, 1, 1))
        rng = np.random.default_rng(50 + case.k)
        drift = np.zeros((sw.S, case.k, case.ns)); drift[:, :, :2] = rng.uniform(-2.5, 2.5, size=(sw.S, case.k, 2))
        Xt = x0s[:, None, :] + np.linspace(0.0, 1.0, 23)[None, :, None] * drift.reshape(sw.S, 1, -1)      # every second row is sampled
        for X in (x0s[:, None, :], Xt):
            fw = ScenarioFrontEnd(d, X, U0s, sw.RADIUS, None)
            fc = ScenarioFrontEnd(d, X, U0s, sw.RADIUS, None, max_cluster=64)
            a, b = arrays(fw), arrays(fc)
            assert fc.max_cluster == 64 and not b.pop("dropped").any() and all(np.array_equal(a[key], b[key]) for key in ARRAYS), case.id
            n += 1
    for prob, X, U in tgs._one_word_scenarios(dp, golden):      # k <= 64, n_words = 1: the narrow entry's arrays
        d = describe(prob)
        fn = ScenarioFrontEnd(d, X, U, sw.RADIUS, None)
        fc = ScenarioFrontEnd(d, X, U, sw.RADIUS, None, max_cluster=64)
        a, b = arrays(fn), arrays(fc)
        assert not fn.wide and not fc.wide and fc.max_cluster == fn.k and fn.bits.shape == fc.bits.shape
        assert not b.pop("dropped").any() and all(np.array_equal(a[key], b[key]) for key in ARRAYS)
        n += 1
    print(f"\n[nearest no-op] m = min(k, 64) on {n} sparse batches: bits, rep, size, order, slot, bucket starts and counts equal the uncapped "
          "entries' bit for bit (0 differences, 0 allowed)")


def _raw(dp, k, X, radius, m, guard=False):
    """The C entry itself on X (S, N, n_x): host copies of the eight arrays; guard=True: bits and dropped sit between guard words."""
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import device, ptr, stream_handle, to_dev
    S, N = X.shape[0], X.shape[1]
    nw = (k + 63) // 64
    Xd, rad = to_dev(X), to_dev(np.full(S, radius))
    g = 3 if guard else 0
    bits = torch.full((S * k * nw + 2 * g,), GUARD, dtype=torch.int64, device=device())
    dropped = torch.full((S * k + 2 * g,), -77, dtype=torch.int32, device=device())
    rep, size, order, slot = (torch.full((S * k,), -5, dtype=torch.int32, device=device()) for _ in range(4))
    bstart, bcount = (torch.full((k + 1,), -5, dtype=torch.int32, device=device()) for _ in range(2))
    _lib.check(_lib.load().dpilqr_dispatch_graph_nearest(S, N, k, nc.NS, ptr(Xd), ptr(rad), 1, None, m, bits.data_ptr() + 8 * g, ptr(rep), ptr(size),
                                                         ptr(order), ptr(slot), ptr(bstart), ptr(bcount), dropped.data_ptr() + 4 * g, nw,
                                                         stream_handle()))
    torch.cuda.synchronize()
    out = dict(bits=bits, dropped=dropped, rep=rep, size=size, order=order, slot=slot, bstart=bstart, bcount=bcount)
    out = {key: v.cpu().numpy() for key, v in out.items()}
    if guard:
        for key, fill in (("bits", GUARD), ("dropped", -77)):
            assert (out[key][:g] == fill).all() and (out[key][-g:] == fill).all(), key
            out[key] = out[key][g:-g]
    return out


@pytest.mark.parametrize("k,m", [(65, 4), (256, 2), (6, 3)])
def test_position_independence_guards_and_nan(dp, k, m):
    _, _, X = nc.scenario(k)
    nw = (k + 63) // 64
    whole = _raw(dp, k, X, nc.GRAPH_RADIUS, m, guard=True)
    for s in range(nc.S):      # a scenario alone: the same words, dropped, rep and size
        alone = _raw(dp, k, X[s:s + 1], nc.GRAPH_RADIUS, m, guard=True)
        assert np.array_equal(alone["bits"], whole["bits"].reshape(nc.S, -1)[s]) and np.array_equal(alone["dropped"], whole["dropped"].reshape(nc.S, k)[s])
        assert np.array_equal(alone["rep"], whole["rep"].reshape(nc.S, k)[s]) and np.array_equal(alone["size"], whole["size"].reshape(nc.S, k)[s])
    # another order of the batch
    swapped = _raw(dp, k, X[[2, 0, 1]], nc.GRAPH_RADIUS, m)
    assert np.array_equal(swapped["bits"].reshape(nc.S, -1), whole["bits"].reshape(nc.S, -1)[[2, 0, 1]])
    # NaN positions in scenario 1 (one agent on one row; one agent on every row; every agent): the other scenarios keep their bits
    for poison in ("row", "agent", "all"):
        Xn = np.array(X).reshape(nc.S, nc.ROWS, k, nc.NS)
        if poison == "row":
            Xn[1, 3, k // 2, :2] = np.nan
        elif poison == "agent":
            Xn[1, :, k // 2, :2] = np.nan
        else:
            Xn[1] = np.nan
        got = _raw(dp, k, Xn.reshape(nc.S, nc.ROWS, -1), nc.GRAPH_RADIUS, m, guard=True)
        for key, per in (("bits", k * nw), ("dropped", k), ("rep", k), ("size", k)):
            assert np.array_equal(got[key].reshape(nc.S, per)[[0, 2]], whole[key].reshape(nc.S, per)[[0, 2]]), (poison, key)
        masks = sw.words_to_masks(got["bits"].view(np.int64).reshape(nc.S, k, nw))[1]
        ref = nc.reference(Xn[1].reshape(nc.ROWS, -1), k, nc.NS, nc.GRAPH_RADIUS, m)
        assert list(masks) == nc.masks_of(ref[0], k) and np.array_equal(got["dropped"].reshape(nc.S, k)[1], ref[1]), poison      # a NaN is never near
        if poison != "row":
            assert masks[k // 2] == 1 << (k // 2)
    print(f"\n[nearest position k{k}-m{m}] exact: a scenario alone and in another place gives the same arrays; guard words untouched; a NaN "
          "scenario changes no other (0 differences, 0 allowed)")


def _solve_inputs(dp, case, S):
    x0, xf, _ = nc.scenario(case.k)
    prob = tgs.dp_problem(dp, case, xf[0])
    return prob, x0[:S, None, :], np.zeros((S, case.T, case.k * nc.NC)), xf[:S]


@pytest.mark.parametrize("case", nc.SOLVE_CASES, ids=lambda c: c.id)
def test_capped_distributed_solves_against_the_oracle(dp, case):
    from dpilqr_amd import _lib
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    ci, k, S = nc.CASES.index(case), case.k, case.S_solve
    prob, X, U0s, xf = _solve_inputs(dp, case, S)
    # the new ground: without the cap the k = 130 team is refused by the front end, the k = 64 team by the solver (n_x = 244 .. 256)
    if k == 130:
        with pytest.raises(ValueError, match="a sub-problem has at most 64 agents; this team has"):
            solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, xf=xf, n_lqr_iter=nc.N_LQR_ITER)
    if k == 64:
        with pytest.raises(_lib.DpilqrError) as err:
            solve_scenarios_distributed(prob, X[:1], U0s[:1], nc.GRAPH_RADIUS, xf=xf[:1], n_lqr_iter=nc.N_LQR_ITER, concurrent=False)
        print(f"\n[nearest solve {case.id}] uncapped: {err.value}")
        assert err.value.code == _lib.EUNSUPPORTED
    Xd, Ud, Jf, info = solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, xf=xf, max_cluster=case.m, n_lqr_iter=nc.N_LQR_ITER)
    assert info["max_cluster"] == case.m and max(info["sizes"]) <= case.m and info["n_dropped"].shape == (S, k) and info["n_dropped"].dtype == np.int32
    assert info["cluster_bits"].shape == ((S, k, case.n_words) if k > 64 else (S, k))
    dev_masks = sw.words_to_masks(info["cluster_bits"].reshape(S, k, -1))
    worst = 0.0
    ns, nc_ = nc.NS, nc.NC
    for s in range(S):
        Xo, Uo, Jo, graph, dropped = nc.oracle_solve(ci, s)
        assert list(dev_masks[s]) == nc.masks_of(graph, k) and np.array_equal(info["n_dropped"][s], dropped), s
        for i in range(k):      # every agent of every scenario, against its own columns
            worst = max(worst, relerr(Xd[s][:, i * ns:(i + 1) * ns], Xo[:, i * ns:(i + 1) * ns]), relerr(Ud[s][:, i * nc_:(i + 1) * nc_], Uo[:, i * nc_:(i + 1) * nc_]))
        worst = max(worst, abs(Jf[s] - Jo) / abs(Jo))
    print(f"\n[nearest solve {case.id}] vs the oracle's capped distributed solve, worst agent of {S} scenarios: {worst:.2e} (tol {TOL_SOLVE:.0e}); "
          f"sub-problems {info['n_unique']} of {info['n_subproblems']}, sizes {info['sizes']}, members dropped {int(info['n_dropped'].sum())}")
    assert worst < TOL_SOLVE
    if k == 65:      # the one-scenario entry prunes its host graph the same way: the same sub-problem solves, stitch and rollout
        Xs, Us, Js, si = dp.solve_distributed(prob, X[0], U0s[0], nc.GRAPH_RADIUS, verbose=False, max_cluster=case.m, n_lqr_iter=nc.N_LQR_ITER)
        assert relerr(Xs, Xd[0]) < TOL_SOLVE and relerr(Us, Ud[0]) < TOL_SOLVE
        assert [prob.ids.index(int(j)) for j in si[prob.ids[10]][1]] == nc.oracle_solve(ci, 0)[3][10]


def test_options_compose_with_the_cap(dp):
    """ignore_ids, audit, device_out and shard= (the narrow pack / scatter path) on capped masks, k = 6, m = 3."""
    import torch
    from dpilqr_amd.dispatch import solve_scenarios_distributed
    case = nc.CASES[1]
    prob, X, U0s, xf = _solve_inputs(dp, case, nc.S)
    kw = dict(xf=xf, max_cluster=case.m, n_lqr_iter=nc.N_LQR_ITER)
    Xd, Ud, Jf, info = solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, audit=True, **kw)
    assert sorted(info["audit"]) == [3] and info["audit"][3]["X"].shape[0] == info["sizes"][3]
    Xt, Ut, Jt, info_t = solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, device_out=True, **kw)
    assert isinstance(Xt, torch.Tensor) and np.array_equal(Xt.cpu().numpy(), Xd) and isinstance(info_t["n_dropped"], np.ndarray)
    fe, solved, info_s = solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, shard=(0, 1), **kw)
    rows, n_rows = fe.pack_rows(solved, pad_to=nc.S * case.k)
    Xr, Ur = fe.scatter_rows(rows)
    assert n_rows == nc.S * case.k and np.array_equal(Xr.cpu().numpy(), Xd) and np.array_equal(Ur.cpu().numpy(), Ud)
    assert np.array_equal(info_s["n_dropped"], info["n_dropped"])
    Xi, Ui, Ji, info_i = solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, ignore_ids=[prob.ids[2]], **kw)
    cols = np.r_[0:8, 12:24]
    assert np.array_equal(info_i["cluster_bits"], info["cluster_bits"]) and not Xi[:, :, 8:12].any() and relerr(Xi[:, :, cols], Xd[:, :, cols]) < 1e-9
    print("\n[nearest options] exact: audit, device_out, shard=(0, 1) through pack_rows / scatter_rows and ignore_ids on capped masks")


# ---- closed loop
N_STARTS = 2
_POLICY = {}


def policy_run(dp, case):
    """solve_scenarios_distributed(policy=..., max_cluster=m) of a policy case, once: S = 2 scenarios."""
    if case.id not in _POLICY:
        prob, X, U0s, xf = _solve_inputs(dp, case, 2)
        X_dec, U_dec, J, info = dp.solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, xf=xf, policy=case.policy, policy_mu=pc.MU,
                                                               max_cluster=case.m, n_lqr_iter=nc.N_LQR_ITER)
        _POLICY[case.id] = dict(prob=prob, X=X, xf=xf, X_dec=X_dec, U_dec=U_dec, info=info, pol=info["policy"])
    return _POLICY[case.id]


def _definition(case, r, s, x0, W=None, u_lim=None, e=0.0):
    """The distributed policy's definition in NumPy (tests/policy_dec_wide_cases.py: ref_sample) on the device's Kc, U_ff and bits"""
    k = case.k
    pol = r["pol"]
    words = pol.bits.cpu().numpy().reshape(2, k, -1).view(np.uint64)[s]
    idx, used = wc.gather_index(wc.members_of(words, k), nc.NS, pol.kc_max)
    batch = dict(models=[0] * k, n_dims=[2] * k, xf=r["xf"])
    p = nc.oracle_problem(k, r["xf"][s], case.T)
    return wc.ref_sample(p, batch, s, pol.X_dec[s].cpu().numpy() * (1 + e), pol.U_ff[s].cpu().numpy() * (1 - e), pol.Kc[s].cpu().numpy() * (1 - e),
                         idx, used, x0 * (1 + e), W, u_lim)


@pytest.mark.parametrize("case", nc.POLICY_CASES, ids=lambda c: c.id)
def test_closed_loop_rollout_of_a_capped_policy(dp, case):
    k, T = case.k, case.T
    r = policy_run(dp, case)
    pol = r["pol"]
    assert pol.kc_max <= case.m and pol.wide == (case.policy == "wide")
    want = [nc.masks_of(nc.reference(r["X"][s], k, nc.NS, nc.GRAPH_RADIUS, case.m)[0], k) for s in range(2)]
    assert [list(row) for row in sw.words_to_masks(pol.bits.cpu().numpy().reshape(2, k, -1))] == want      # the capped masks
    rng = np.random.default_rng(900 + k)
    scale = np.zeros((k, nc.NS)); scale[:, :2] = 0.05
    x0s = r["X"][:, 0][:, None, :] + rng.normal(size=(2, N_STARTS, k * nc.NS)) * scale.reshape(-1)
    host = lambda out: {key: v.cpu().numpy() for key, v in out.items()}
    got = host(pol.rollout(x0s, trajectories=True))
    W = pc.W_SCALE * np.random.default_rng(5).normal(size=(2, N_STARTS, T, k * nc.NS))
    flat = got["U"].reshape(-1, k * nc.NC)
    u_lim = np.stack([np.quantile(flat, pc.QUANTILES[0], axis=0), np.quantile(flat, pc.QUANTILES[1], axis=0)])
    got2 = host(pol.rollout(x0s, W=W, u_lim=u_lim, trajectories=True))
    assert np.mean((got2["U"] == u_lim[0]) | (got2["U"] == u_lim[1])) > 0.10
    worst, unchecked = None, 0
    for g, Wv, lim in ((got, None, None), (got2, W, u_lim)):
        for s in range(2):
            for q in range(N_STARTS):
                Wq = None if Wv is None else Wv[s, q]
                ref = _definition(case, r, s, x0s[s, q], Wq, lim)
                spread = max(pc.difference(_definition(case, r, s, x0s[s, q], Wq, lim, e=sg * lc.PERTURB), ref) for sg in (1.0, -1.0))
                bound = pc.bound_of(spread)
                if bound is None:
                    unchecked += 1
                    continue
                d = pc.difference(dict(X=g["X"][s, q], U=g["U"][s, q], J=float(g["J"][s, q]), min_sep=float(g["min_sep"][s, q]),
                                       goal_dist=g["goal_dist"][s, q]), ref)
                if worst is None or d / bound >= worst[0]:
                    worst = (d / bound, d, bound)
                assert d <= bound, (s, q, d, bound)
    print(f"\n[nearest closed loop {case.id}] policy.rollout vs the definition on the device's Kc, U_ff, bits: worst share of its bound {worst[0]:.3g} "
          f"(difference {worst[1]:.3g}, bound {worst[2]:.3g}); kc_max {pol.kc_max} (cap {case.m}); samples without a bound {unchecked} of {4 * N_STARTS}")
    assert unchecked <= pc.MAX_UNCHECKED * 4 * N_STARTS


def test_receding_horizon_loop_on_the_64_agent_near_clique(dp):
    """solve_rhc_closed_loop(centralized=False, wide=True, max_cluster=4): two rounds for two scenarios of a team whose uncapped
    rounds are refused; the first executed prefix is policy_rollout_dec_wide of the first round's policy, bit for bit (the
    advance's documented property)."""
    case = nc.CASES[2]
    assert (case.k, case.m) == (64, 4)
    prob, X, U0s, xf = _solve_inputs(dp, case, 2)
    x0 = X[:, 0]
    kw = dict(n_lqr_iter=nc.N_LQR_ITER)
    out = dp.solve_rhc_closed_loop(prob, x0, case.T, radius=nc.GRAPH_RADIUS, xf=xf, U0=U0s, centralized=False, wide=True, max_cluster=4, max_steps=4,
                                   step_size=2, dist_converge=1e-3, **kw)
    assert (out["n_rounds"] == 2).all() and not out["converged"].any() and all(x.shape == (5, 256) for x in out["X"])
    _, _, _, info = dp.solve_scenarios_distributed(prob, X, U0s, nc.GRAPH_RADIUS, xf=xf, policy="wide", policy_mu=0.0, max_cluster=4, device_out=True, **kw)
    roll = info["policy"].rollout(x0[:, None, :], trajectories=True)
    Xr, Ur = roll["X"].cpu().numpy()[:, 0], roll["U"].cpu().numpy()[:, 0]
    same = all(np.array_equal(out["X"][s][:3], Xr[s][:3]) and np.array_equal(out["U"][s][:2], Ur[s][:2]) for s in range(2))
    print(f"\n[nearest loop k64-m4] two rounds of two scenarios; first executed prefix equals policy_rollout_dec_wide of the first round's policy bit for "
          f"bit: {same}; realised J {out['J']}")
    assert same and np.isfinite(out["J"]).all()
    from dpilqr_amd import _lib
    with pytest.raises(_lib.DpilqrError):      # without the cap the first round's solve is refused
        dp.solve_rhc_closed_loop(prob, x0[:1], case.T, radius=nc.GRAPH_RADIUS, xf=xf[:1], U0=U0s[:1], centralized=False, wide=True, max_steps=4,
                                 step_size=2, dist_converge=1e-3, **kw)
