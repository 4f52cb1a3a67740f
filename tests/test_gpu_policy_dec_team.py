"""The team closed-loop rollout (dpilqr_policy_rollout_dec_team, csrc/policy_dec_team.hpp) on the GPU.

  reference   per case of tests/policy_dec_team_cases.py and variant (plain, W, u_lim), every sample against the CPU reference
              (policy_cases.ref_sample's loop fed the masked dense gains) within its own bound bound_of(spread); the kernel gets
              the compact gains with every unused column NaN; with / without stored trajectories
  cross       on two cases both kernels serve (mixed models; mixed n_dims) against policy_rollout_dec fed the same inputs: X, U
              and goal_dist bit for bit (the same products in the same order, the same step), J and min_sep within the
              project's rollout tolerance (the team kernel sums a stage cost agent by agent)
  position    an item gives the same bits at another place in the batch and with another number of samples, a run repeated
              gives the same bits, guard rows around every output are untouched, an item of NaN poisons only itself, NaN in the
              never-read columns changes nothing
  end to end  24 double integrators (n_x = 96), two scenarios of mixed cluster sizes: solve_scenarios_distributed(policy=True)
              -> DistributedPolicy.rollout against the definition unfolded from the audited sub-problem solutions with the
              ORACLE's gains; closed_loop_distributed returns scenario 0; a radius that joins no one is every agent alone."""
import numpy as np
import pytest

from tests import linesearch_cases as lc
from tests import policy_cases as pc
from tests import policy_dec_cases as dc
from tests import policy_dec_team_cases as tc

pytestmark = pytest.mark.gpu

B, T = pc.B, pc.T
VARIANTS = ["plain", "W", "u_lim"]


def _pb(case, b, items=None):
    import dpilqr_amd as dp
    sel = (lambda a: a) if items is None else (lambda a: a[items])
    if case.weights == "per_item":
        Q, R, Qf = sel(b["Q"]), sel(b["R"]), sel(b["Qf"])
    else:
        Q, R, Qf = b["Q"], b["R"], b["Qf"]
    return dp.ProblemBatch(b["models"], b["n_dims"], sel(b["xf"]), Q, R, Qf, b["radius"], b["dt"], T)


def _host(r):
    return {k_: t.cpu().numpy() for k_, t in r.items()}


_RUNS = {}


def gpu_runs(case):
    """The case's launches, once."""
    if case.id not in _RUNS:
        ref = tc.case_ref(case)
        b, k, ns, nc = ref.batch, case.k, case.ns, case.nc
        pb = _pb(case, b)
        Kc = dc.compact_gains(ref.K, ref.masks, ns, nc, k)
        assert np.isnan(Kc).any()
        out = {}
        for v in VARIANTS:
            W, lim = ref.args(v)
            out[v] = _host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
            out[v + "-nostore"] = _host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim))
        _RUNS[case.id] = out
    return _RUNS[case.id]


def worst_against_reference(case, variant, got):
    """(largest error / bound, largest error, its bound, unchecked samples, failures) over the case's samples."""
    ref = tc.case_ref(case)
    worst, at, unchecked, failures = 0.0, (0.0, 0.0), 0, []
    for i in range(B):
        for s in range(case.S):
            bound = pc.bound_of(ref.spread[variant][i, s])
            if bound is None:
                unchecked += 1
                continue
            g = dict(X=got["X"][i, s], U=got["U"][i, s], J=float(got["J"][i, s]), min_sep=float(got["min_sep"][i, s]),
                     goal_dist=got["goal_dist"][i, s])
            d = pc.difference(g, ref.ref[variant][i][s])
            if d / bound >= worst:
                worst, at = d / bound, (d, bound)
            if not d <= bound:
                failures.append((i, s, d, bound))
    return worst, at[0], at[1], unchecked, failures


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_against_reference(case, variant):
    got = gpu_runs(case)[variant]
    worst, d, bound, unchecked, failures = worst_against_reference(case, variant, got)
    print(f"{case.id} {variant}: worst error / bound {worst:.3g} (error {d:.3g}, bound {bound:.3g}), unchecked {unchecked} of {B * case.S}")
    assert unchecked <= pc.MAX_UNCHECKED * B * case.S, (unchecked, B * case.S)
    assert not failures, failures[:5]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_not_storing_trajectories_changes_nothing(case, variant):
    runs = gpu_runs(case)
    a, b_ = runs[variant], runs[variant + "-nostore"]
    assert set(a) == {"X", "U", "J", "min_sep", "goal_dist"} and set(b_) == {"J", "min_sep", "goal_dist"}
    for key in b_:
        assert np.array_equal(a[key], b_[key]), key


@pytest.mark.parametrize("case", tc.CROSS, ids=[c.id for c in tc.CROSS])
def test_against_the_old_kernel(case):
    ref = dc.case_ref(case)
    b, k = ref.batch, case.k
    pb = _pb(case, b)
    Kc = dc.compact_gains(ref.K, ref.masks, case.ns, case.nc, k)
    for v in VARIANTS:
        W, lim = ref.args(v)
        old = _host(pb.policy_rollout_dec(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
        new = _host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=W, u_lim=lim, trajectories=True))
        assert set(old) == set(new)
        for key in ("X", "U", "goal_dist"):
            assert np.array_equal(old[key], new[key]), (v, key)
        eJ = np.max(np.abs(new["J"] - old["J"]) / np.abs(old["J"]))
        eS = np.max(np.abs(new["min_sep"] - old["min_sep"]) / np.abs(old["min_sep"]))
        print(f"{case.id} {v}: J {eJ:.2e}, min_sep {eS:.2e} (tol {pc.TOL_ROLLOUT:.0e})")
        assert np.isfinite(old["J"]).all() and eJ <= pc.TOL_ROLLOUT and eS <= pc.TOL_ROLLOUT, (v, eJ, eS)


# ---- position independence
POS_CASE = tc.CASES[0]      # 21 mixed agents, per-item weights, 12 samples per workgroup


def _guarded(S, k, n, m, Bn):
    """Outputs with a guard row before and after, handed to the C entry directly: (views, whole buffers)."""
    import torch
    from dpilqr_amd.device import device
    shapes = dict(X=(Bn * S, T + 1, n), U=(Bn * S, T, m), J=(Bn * S,), min_sep=(Bn * S,), goal_dist=(Bn * S, k))
    whole = {key: torch.full((sh[0] + 2,) + sh[1:], -7.25, dtype=torch.float64, device=device()) for key, sh in shapes.items()}
    return {key: w[1:-1] for key, w in whole.items()}, whole


def test_position_independence_and_guards():
    import torch
    from dpilqr_amd import _lib
    from dpilqr_amd.device import ptr, stream_handle, to_dev
    case = POS_CASE
    ref = tc.case_ref(case)
    b, k, ns, nc, S = ref.batch, case.k, case.ns, case.nc, case.S
    n, m = k * ns, k * nc
    full = gpu_runs(case)["W"]
    Kc = dc.compact_gains(ref.K, ref.masks, ns, nc, k)
    # a run repeated: the same bits
    again = _host(_pb(case, b).policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, b["x0s"], W=b["W"], trajectories=True))
    for key in full:
        assert np.array_equal(full[key], again[key]), key
    # item 2 at place 0 of a batch of two, five of its samples in another order: another chunk, another workgroup, another S
    items, smp = [2, 0], [12, 3, 0, 7, 11]
    r = _host(_pb(case, b, items).policy_rollout_dec_team(ref.X[items], ref.U[items], Kc[items], ref.masks[items], b["x0s"][items][:, smp],
                                                          W=b["W"][items][:, smp], trajectories=True))
    for key in full:
        assert np.array_equal(r[key], full[key][items][:, smp]), key
    # guard rows around every output, through the C entry
    pb = _pb(case, b)
    view, whole = _guarded(S, k, n, m, B)
    dev = [to_dev(a) for a in (ref.X, ref.U, Kc, b["x0s"], b["W"])]
    bits = torch.from_numpy(ref.masks.view(np.int64)).to(dev[0].device)
    _lib.check(pb._lib.dpilqr_policy_rollout_dec_team(pb._d, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), k, ptr(bits), S, ptr(dev[3]), ptr(dev[4]),
                                                      None, ptr(view["X"]), ptr(view["U"]), ptr(view["J"]), ptr(view["min_sep"]),
                                                      ptr(view["goal_dist"]), stream_handle()))
    torch.cuda.synchronize()
    for key, w in whole.items():
        h = w.cpu().numpy()
        assert (h[0] == -7.25).all() and (h[-1] == -7.25).all(), key
        assert np.array_equal(h[1:-1].reshape(full[key].shape), full[key]), key


def test_nan_poisons_only_its_item_and_unread_columns_nothing():
    case = POS_CASE
    ref = tc.case_ref(case)
    b, k, ns, nc = ref.batch, case.k, case.ns, case.nc
    full = gpu_runs(case)["u_lim"]
    pb = _pb(case, b)
    # the never-read columns: NaN (the runs above), zero, and huge -- the same bits
    for fill in (0.0, 1e300):
        r = _host(pb.policy_rollout_dec_team(ref.X, ref.U, dc.compact_gains(ref.K, ref.masks, ns, nc, k, fill=fill), ref.masks, b["x0s"],
                                             u_lim=ref.u_lim, trajectories=True))
        for key in full:
            assert np.array_equal(r[key], full[key]), (fill, key)
    assert all(np.isfinite(full[key]).all() for key in full)
    # item 1 poisoned
    Kc = dc.compact_gains(ref.K, ref.masks, ns, nc, k)
    x0s = b["x0s"].copy()
    Kc[1] = np.nan; x0s[1] = np.nan
    r = _host(pb.policy_rollout_dec_team(ref.X, ref.U, Kc, ref.masks, x0s, u_lim=ref.u_lim, trajectories=True))
    for key in full:
        assert np.array_equal(r[key][[0, 2]], full[key][[0, 2]]), key
    assert np.isnan(r["J"][1]).all() and np.isnan(r["X"][1]).all()


# ---- end to end: 24 double integrators
K_AG, NS, NC, DT = 24, 4, 2, 0.1
N_DIMS = [2] * K_AG
RADIUS, PROX_RADIUS, MU = 0.5, 0.5, 1.0
N_STARTS = 3
Q, R, QF = np.diag([1.0, 1.0, 0.5, 0.5]), np.eye(NC), 100.0 * np.eye(NS)
S_E2E = 2


def _placement():
    """Agents closer than 2 RADIUS = 1 are neighbours.  Scenario 0: a chain of five (0.8 apart: sizes 2, 3, 3, 3, 2), a square of
    four (0.5: 4 each), a pair (0.6) and thirteen loners on a grid far away.  Scenario 1: a cluster of six (a centre and a
    pentagon of radius 0.5 around it: the longest chord is 0.95), three pairs and twelve loners.  The sizes are asserted below, on
    the CPU."""
    far = lambda i: [10.0 + 4.0 * (i % 5), 10.0 + 4.0 * (i // 5)]
    s0 = [[0.8 * i, 0.0] for i in range(5)] + [[0.0, 5.0], [0.5, 5.0], [0.0, 5.5], [0.5, 5.5]] + [[5.0, 0.0], [5.6, 0.0]]
    s0 += [far(i) for i in range(K_AG - len(s0))]
    s1 = [[0.0, 3.0]] + [[0.5 * np.cos(2 * np.pi * i / 5), 3.0 + 0.5 * np.sin(2 * np.pi * i / 5)] for i in range(5)]
    s1 += [[6.0, 0.0], [6.7, 0.0], [0.0, 8.0], [0.0, 8.7], [8.0, 8.0], [8.5, 8.5]]
    s1 += [far(i) for i in range(K_AG - len(s1))]
    pos = np.array([s0, s1])
    rng = np.random.default_rng(2424)
    goal = pos + rng.uniform(0.6, 1.4, size=pos.shape) * rng.choice([-1.0, 1.0], size=pos.shape)
    return pos, goal


def _states(pos):
    x = np.zeros((S_E2E, K_AG, NS))
    x[:, :, :2] = pos
    return x.reshape(S_E2E, -1)


POS0, GOAL = _placement()
X0, XF = _states(POS0), _states(GOAL)
SIZES = [[2, 3, 3, 3, 2, 4, 4, 4, 4, 2, 2] + [1] * 13, [6] * 6 + [2] * 6 + [1] * 12]


def _problem(xf=XF[0]):
    import dpilqr_amd as dp
    dp._reset_ids()
    dyn = dp.MultiDynamicalModel([dp.DoubleIntDynamics4D(DT) for _ in range(K_AG)])
    costs = [dp.ReferenceCost(xf[NS * i:NS * (i + 1)], Q, R, QF, i) for i in range(K_AG)]
    return dp.ilqrProblem(dyn, dp.GameCost(costs, dp.ProximityCost([NS] * K_AG, PROX_RADIUS, N_DIMS)))


def _members(mask):
    return [j for j in range(K_AG) if (int(mask) >> j) & 1]


def test_the_scenarios_have_the_cluster_sizes_they_are_placed_for():
    """On the CPU, with the package's own NumPy graph function."""
    from dpilqr_amd.distributed import define_inter_graph_threshold
    sizes = [[len(v) for v in define_inter_graph_threshold(X0[s][None], RADIUS, [NS] * K_AG, list(range(K_AG))).values()] for s in range(S_E2E)]
    assert sizes == SIZES
    assert K_AG * NS == 96 and len({kc for row in sizes for kc in row}) >= 4      # beyond n_x = 60; mixed sizes


def _owners(bits):
    """(bucket size, slot, members, pos) of every (s, i): representatives in (s, i) order inside their size's bucket."""
    count, slot_of = {}, {}
    for s in range(S_E2E):
        for i in range(K_AG):
            key = (s, int(bits[s, i]))
            if key not in slot_of:
                kc = len(_members(bits[s, i]))
                slot_of[key] = count.get(kc, 0)
                count[kc] = slot_of[key] + 1
    out = {}
    for s in range(S_E2E):
        for i in range(K_AG):
            mem = _members(bits[s, i])
            out[s, i] = (len(mem), slot_of[s, int(bits[s, i])], mem, mem.index(i))
    return out


_SOLVED = {}


def solved(radius=RADIUS):
    if radius not in _SOLVED:
        import dpilqr_amd as dp
        X_dec, U_dec, J, info = dp.solve_scenarios_distributed(_problem(), X0[:, None, :], np.zeros((S_E2E, T, K_AG * NC)), radius, xf=XF,
                                                               audit=True, policy=True, policy_mu=MU, n_lqr_iter=20)
        pol = info["policy"]
        _SOLVED[radius] = dict(X_dec=X_dec, U_dec=U_dec, info=info, pol=pol, bits=info["cluster_bits"].astype(np.uint64))
    return _SOLVED[radius]


def _full_problem(s):
    return lc.orc.Problem([0] * K_AG, N_DIMS, XF[s], np.broadcast_to(Q, (K_AG, NS, NS)), np.broadcast_to(R, (K_AG, NC, NC)),
                          np.broadcast_to(QF, (K_AG, NS, NS)), PROX_RADIUS, DT, T)


def _sub_policies(r, s):
    """Per agent of scenario s: (members' state columns, pos, X^i, U^i, K^i), K^i the oracle's backward pass at the GPU's
    sub-problem solution."""
    aud, own = r["info"]["audit"], _owners(r["bits"])
    subs, cache = [], {}
    for i in range(K_AG):
        kc, slot, mem, pos = own[s, i]
        Xi, Ui = aud[kc]["X"][slot], aud[kc]["U"][slot]
        if (kc, slot) not in cache:
            p = lc.orc.Problem([0] * kc, [2] * kc, aud[kc]["xf"][slot], np.broadcast_to(Q, (kc, NS, NS)), np.broadcast_to(R, (kc, NC, NC)),
                               np.broadcast_to(QF, (kc, NS, NS)), PROX_RADIUS, DT, T)
            cache[kc, slot] = np.asarray(p.backward_pass(Xi, Ui, MU)[0])
        cols = np.concatenate([np.arange(j * NS, (j + 1) * NS) for j in mem])
        subs.append((cols, pos, Xi, Ui, cache[kc, slot]))
    return subs


def ref_definition(p, s, subs, x0, W=None, u_lim=None, e=0.0):
    """The definition, unfolded: u_i = U^i[pos] + K^i[pos] (x_{C_i} - X^i); e: the relative perturbation of the sensitivity runs."""
    n, m = K_AG * NS, K_AG * NC
    Xs = np.zeros((T + 1, n)); Us = np.zeros((T, m))
    Xs[0] = x0 * (1 + e)
    J, sep = 0.0, tc.separation(Xs[0], K_AG, NS, N_DIMS)
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
        sep = min(sep, tc.separation(Xs[t + 1], K_AG, NS, N_DIMS))
    J += float(p.cost(Xs[-1], np.zeros(m), True))
    err = (Xs[-1] - XF[s]).reshape(K_AG, NS)
    return dict(X=Xs, U=Us, J=J, min_sep=sep, goal_dist=np.sqrt(np.sum(err[:, :2] ** 2, axis=1)))


def _starts():
    from dpilqr_amd.util import perturbed_starts
    return np.stack([perturbed_starts(X0[s], [NS] * K_AG, N_STARTS, var=0.2, seed=70 + s) for s in range(S_E2E)])


def _check(got, r, x0s, W=None, u_lim=None):
    unchecked = 0
    for s in range(S_E2E):
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
            assert d <= bound, (s, q, d, bound)
    assert unchecked <= pc.MAX_UNCHECKED * S_E2E * N_STARTS, unchecked


def test_end_to_end_against_the_definition():
    r = solved()
    assert sorted(r["info"]["audit"]) == [1, 2, 3, 4, 6] and r["pol"].kc_max == 6
    assert [[dc.popcount(v) for v in row] for row in r["bits"]] == SIZES
    x0s = _starts()
    got = _host(r["pol"].rollout(x0s, trajectories=True))
    assert got["X"].shape == (S_E2E, N_STARTS, T + 1, 96)
    _check(got, r, x0s)
    rng = np.random.default_rng(5)
    W = pc.W_SCALE * rng.normal(size=(S_E2E, N_STARTS, T, K_AG * NS))
    flat = got["U"].reshape(-1, K_AG * NC)
    u_lim = np.stack([np.quantile(flat, pc.QUANTILES[0], axis=0), np.quantile(flat, pc.QUANTILES[1], axis=0)])
    got2 = _host(r["pol"].rollout(x0s, W=W, u_lim=u_lim, trajectories=True))
    assert np.mean((got2["U"] == u_lim[0]) | (got2["U"] == u_lim[1])) > 0.10
    _check(got2, r, x0s, W, u_lim)
    short = _host(r["pol"].rollout(x0s, W=W, u_lim=u_lim))
    assert set(short) == {"J", "min_sep", "goal_dist"} and all(np.array_equal(short[k_], got2[k_]) for k_ in short)


def test_closed_loop_distributed_returns_scenario_zero():
    import dpilqr_amd as dp
    r = solved()
    x0s = _starts()
    got = _host(r["pol"].rollout(x0s, trajectories=True))
    one = dp.closed_loop_distributed(_problem(XF[0]), X0[0][None], np.zeros((T, K_AG * NC)), RADIUS, x0s[0], mu=MU, trajectories=True,
                                     n_lqr_iter=20)
    assert np.array_equal(one["X_dec"], r["X_dec"][0]) and np.array_equal(one["U_dec"], r["U_dec"][0])
    for key in ("J", "min_sep", "goal_dist", "X", "U"):
        assert np.array_equal(one[key], got[key][0]), key


def test_a_radius_that_joins_no_one_is_every_agent_alone():
    import dpilqr_amd as dp
    r = solved(radius=1e-3)
    assert all(int(r["bits"][s, i]) == 1 << i for s in range(S_E2E) for i in range(K_AG)) and sorted(r["info"]["audit"]) == [1]
    x0s = _starts()
    got = _host(r["pol"].rollout(x0s, trajectories=True))
    a = r["info"]["audit"][1]                      # the one-agent sub-problems in (s, i) order
    n1 = S_E2E * K_AG
    pb1 = dp.ProblemBatch(np.zeros((n1, 1), dtype=np.int32), np.full((n1, 1), 2, dtype=np.int32), a["xf"], Q, R, QF, PROX_RADIUS, DT, T)
    own = _host(pb1.policy_rollout(a["X"], a["U"], a["K"], x0s.reshape(S_E2E, N_STARTS, K_AG, NS).transpose(0, 2, 1, 3).reshape(n1, N_STARTS, NS),
                                   trajectories=True))
    for s in range(S_E2E):
        for i in range(K_AG):
            assert np.array_equal(got["X"][s][:, :, i * NS:(i + 1) * NS], own["X"][s * K_AG + i]), (s, i)
            assert np.array_equal(got["U"][s][:, :, i * NC:(i + 1) * NC], own["U"][s * K_AG + i]), (s, i)
            assert np.array_equal(got["goal_dist"][s][:, i], own["goal_dist"][s * K_AG + i][:, 0]), (s, i)
